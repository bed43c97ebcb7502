// rip_color_tables.hpp -- the constant tables of the colour stages: gamma LUT, 8-bit Lab / HSV tables, vignetting mask plane.
#pragma once
#include <cstdint>
#include <vector>

namespace rip {

// ---------------------------------------------------------------------------------------------
// Constant tables
// ---------------------------------------------------------------------------------------------
// gamma_correction.cpp:35-43
void build_gamma_lut(double k, uint8_t lut[256]);

// 8-bit Lab (OpenCV 4.2 imgproc/color_lab.cpp initLabTabs, RGB2Lab_b, Lab2RGBinteger) and
// 8-bit HSV (color_hsv.cpp RGB2HSV_b) tables.
struct ColorTables {
  uint16_t srgb_gamma[256];   // sRGBGammaTab_b
  uint16_t cbrt[3072];        // LabCbrtTab_b
  uint16_t lab_to_yf[512];    // LabToYF_b: {y, ify} pairs
  uint16_t inv_gamma[4096];   // sRGBInvGammaTab_b
  int32_t fwd[9];             // BGR -> XYZ/white, Q12, memory order B,G,R per row
  int32_t inv[9];             // XYZ -> B,G,R rows, Q12
  int32_t sdiv[256], hdiv180[256];
};
const ColorTables& color_tables();  // built once

// vignetting_correction.cpp:32-63: the float mask plane (rows x cols, tightly packed), evaluated with the
// reference's operation order (sqrt, pow(r, 2), pow(r, 4) in double); uploaded once per geometry / parameter set
void build_vignette_mask(int rows, int cols, double scale, double a2, double a4, std::vector<float>& mask, int fp_contract = 0);

}  // namespace rip
