// The pinhole distortion models through the C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp), without a device
// (RIP_DEVICE=-1): setUndistortionDistortionCoefficients forwards the whole vector, the two coefficient getters return a
// 1 x n Mat with n = 4 / 5 / 8 by model, and the new camera matrix follows the model.
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

static bool row_equals(const Mat& m, const std::vector<double>& want) {
  if (m.rows != 1 || m.cols != (int)want.size() || !m.isFloat64()) return false;
  for (int i = 0; i < m.cols; i++)
    if (m.at<double>(0, i) != want[i]) return false;
  return true;
}

int main() {
  RawImagePipeline proc(false, "", "", "");
  const int w = 200, h = 136;
  proc.setUndistortionImageSize(w, h);
  proc.setUndistortionCameraMatrix({0.6 * w, 0, 0.49431 * w, 0, 0.5994 * w, 0.48593 * h, 0, 0, 1});
  const std::vector<double> d8 = {0.9, 0.25, 3e-4, -2e-4, 0.01, 1.25, 0.55, 0.05};
  const std::vector<double> d5(d8.begin(), d8.begin() + 5), d4(d8.begin(), d8.begin() + 4);

  // any other model: four values, as before
  proc.setUndistortionDistortionModel("equidistant");
  proc.setUndistortionDistortionCoefficients(d8);
  if (!row_equals(proc.getDistDistortionCoefficients(), d4)) return fail("equidistant reports 4 coefficients");
  if (!row_equals(proc.getRectDistortionCoefficients(), {0, 0, 0, 0})) return fail("equidistant rect coefficients");
  const double fisheye_fx = proc.getRectCameraMatrix().at<double>(0, 0);

  // rational_polynomial: all eight arrive
  proc.setUndistortionDistortionModel("rational_polynomial");
  if (!row_equals(proc.getDistDistortionCoefficients(), d8)) return fail("rational_polynomial reports the 8 values given");
  if (!row_equals(proc.getRectDistortionCoefficients(), std::vector<double>(8, 0.0))) return fail("rational_polynomial rect coefficients");
  const double rational_fx = proc.getRectCameraMatrix().at<double>(0, 0);
  if (!(rational_fx > 0) || rational_fx == fisheye_fx) return fail("the new camera matrix follows the model");

  // plumb_bob: five, k4..k6 are not part of the model
  proc.setUndistortionDistortionModel("plumb_bob");
  if (!row_equals(proc.getDistDistortionCoefficients(), d5)) return fail("plumb_bob reports 5 coefficients");
  const double with_k456 = proc.getRectCameraMatrix().at<double>(0, 0);
  proc.setUndistortionDistortionCoefficients(d5);
  if (!row_equals(proc.getDistDistortionCoefficients(), d5)) return fail("plumb_bob with 5 values");
  if (proc.getRectCameraMatrix().at<double>(0, 0) != with_k456) return fail("plumb_bob ignores k4..k6");
  if (!row_equals(proc.getRectDistortionCoefficients(), std::vector<double>(5, 0.0))) return fail("plumb_bob rect coefficients");

  // radtan: four given, five reported with k3 = 0
  proc.setUndistortionDistortionModel("radtan");
  proc.setUndistortionDistortionCoefficients(d4);
  std::vector<double> d4k3 = d4;
  d4k3.push_back(0.0);
  if (!row_equals(proc.getDistDistortionCoefficients(), d4k3)) return fail("radtan reports 5 coefficients with k3 = 0");

  bool threw = false;
  try {
    proc.setUndistortionDistortionCoefficients({0.1, 0.2, 0.3});
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw) return fail("fewer than 4 coefficients are refused");
  if (!row_equals(proc.getDistDistortionCoefficients(), d4k3)) return fail("a refused setter changes nothing");
  std::printf("pinhole facade OK\n");
  return 0;
}
