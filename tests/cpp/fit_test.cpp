// The window and the fit modes of the resize stage through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputRoi,
// setOutputFit, setOutputPad, getOutputWindow and their refusals, and the known answers of PARITY.md "Resize: window and fit".
// No device needed.  Built as C++14 like the reference.
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <cstring>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

static bool is(const int v[4], int a, int b, int c, int d) { return v[0] == a && v[1] == b && v[2] == c && v[3] == d; }

int main() {
  RawImagePipeline proc(false, "", "", "");
  proc.setFlip(false);
  proc.setUndistortion(false);
  int x = -1, y = -1, w = -1, h = -1, b = -1, g = -1, r = -1, src[4], dst[4];
  proc.getOutputRoi(x, y, w, h);
  proc.getOutputPad(b, g, r);
  if (x || y || w || h || proc.getOutputFit() != "stretch" || b != 114 || g != 114 || r != 114) return fail("defaults");
  proc.getOutputWindow(2048, 2448, 1, "bayer_rggb8", src, dst);
  if (!is(src, 0, 0, 2448, 2048) || !is(dst, 0, 0, 2448, 2048)) return fail("the window of a default handle");
  proc.setOutputSize(640, 480);
  proc.setOutputFit("crop");
  proc.getOutputWindow(2048, 2448, 1, "bayer_rggb8", src, dst);
  if (!is(src, 0, 106, 2448, 1836) || !is(dst, 0, 0, 640, 480)) return fail("the known answer of crop");
  proc.setOutputFit("letterbox");
  proc.getOutputWindow(2048, 2448, 1, "bayer_rggb8", src, dst);
  if (!is(src, 0, 0, 2448, 2048) || !is(dst, 33, 0, 574, 480)) return fail("the known answer of letterbox");
  int rows = 0, cols = 0;
  Mat K, P;
  proc.getOutputCameraInfo(2048, 2448, 1, "bayer_rggb8", rows, cols, K, P);
  if (rows != 480 || cols != 640) return fail("the delivered size under letterbox");
  for (const char* bad : {"", "Letterbox", "pad", "fill", "crop "}) {
    try {
      proc.setOutputFit(bad);
      return fail("invalid fit accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("\"letterbox\"") == std::string::npos) return fail("the message does not name the rule");
    }
    if (proc.getOutputFit() != "letterbox") return fail("fit changed by a refused call");
  }
  proc.setOutputPad(1, 2, 3);
  try {
    proc.setOutputPad(0, 256, 0);
    return fail("invalid pad accepted");
  } catch (const std::invalid_argument&) {
  }
  proc.getOutputPad(b, g, r);
  if (b != 1 || g != 2 || r != 3) return fail("pad changed by a refused call");
  proc.setOutputRoi(8, 4, 100, 50);
  try {
    proc.setOutputRoi(0, 0, 0, 5);
    return fail("invalid roi accepted");
  } catch (const std::invalid_argument&) {
  }
  proc.getOutputRoi(x, y, w, h);
  if (x != 8 || y != 4 || w != 100 || h != 50) return fail("roi changed by a refused call");
  try {
    proc.getOutputWindow(53, 108, 1, "bayer_rggb8", src, dst);  // y + height = 54 > 53
    return fail("a window outside the image accepted");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("does not lie inside") == std::string::npos) return fail("the refusal does not name the rule");
  }
  proc.setOutputSize(0, 0);
  proc.getOutputCameraInfo(54, 108, 1, "bayer_rggb8", rows, cols, K, P);
  if (rows != 50 || cols != 100) return fail("a window without a target delivers the window");
  std::printf("fit host OK\n");
  return 0;
}
