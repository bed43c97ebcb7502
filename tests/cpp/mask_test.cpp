// Valid-pixel masks through include/raw_image_pipeline/raw_image_pipeline.hpp: setRectMask / getRectMaskMode, getRectMask and
// getOutputMask -- defaults and refusals without a device ("host"), and the two masks of a small undistorted frame on one ("gpu").
// Built as C++14 like the reference.
// usage: mask_test host | mask_test gpu <calibration.yaml> <width> <height> <out.bin>
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

#ifdef RIP_HAVE_OPENCV
static Mat make_u8(int rows, int cols, int channels) { return Mat(rows, cols, CV_8UC(channels)); }
#else
static Mat make_u8(int rows, int cols, int channels) { return Mat(rows, cols, channels); }
#endif

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

static int host() {
  RawImagePipeline proc(false, "", "", "");
  proc.setUndistortion(false);
  if (proc.getRectMaskMode() != "off") return fail("the default mode");
  Mat empty = proc.getRectMask();
  if (empty.rows != 0 || empty.cols != 0) return fail("the rect mask of a fresh object is not empty");
  try {
    proc.getOutputMask(72, 136, 1, "bayer_rggb8");
    return fail("an output mask under the mode off");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("'off'") == std::string::npos) return fail("the refusal does not name the mode");
  }
  for (const char* bad : {"on", "Coverage", "", "binary"}) {
    try {
      proc.setRectMask(bad);
      return fail("an unknown mode accepted");
    } catch (const std::invalid_argument&) {
    }
  }
  if (proc.getRectMaskMode() != "off") return fail("a refused mode changed the setting");
  for (const char* mode : {"coverage", "valid", "off", "valid"}) {
    proc.setRectMask(mode);
    if (proc.getRectMaskMode() != mode) return fail("the getter does not return what was set");
  }
  if (proc.getRectMask().rows != 0) return fail("a rect mask without a frame");
  // the geometry is refused exactly where rip_query_output refuses it; with a good one the call needs a device for the bytes
  proc.setOutputRoi(100, 0, 64, 32);
  try {
    proc.getOutputMask(72, 136, 1, "bayer_rggb8");
    return fail("a window outside the image accepted");
  } catch (const std::invalid_argument&) {
  }
  proc.setOutputRoi(0, 0, 0, 0);
  try {
    proc.getOutputMask(72, 136, 1, "bayer_rggb8");
    return fail("mask bytes without a device");
  } catch (const std::invalid_argument&) {
    return fail("the device refusal is reported as an invalid argument");
  } catch (const std::exception&) {
  }
  std::printf("mask host OK\n");
  return 0;
}

static int gpu(const char* calibration, int w, int h, const char* out_path) {
  RawImagePipeline proc(false, "", calibration, "");
  proc.setDebayer(false);
  proc.setFlip(false);
  proc.setWhiteBalance(false);
  proc.setColorCalibration(false);
  proc.setGammaCorrection(false);
  proc.setVignettingCorrection(false);
  proc.setColorEnhancer(false);
  proc.setUndistortion(true);
  proc.setUndistortionBalance(1.0);
  proc.setUndistortionFovScale(1.0);
  proc.setRectMask("coverage");
  Mat frame = make_u8(h, w, 1);
  std::memset(frame.data, 255, (size_t)h * w);
  std::string enc = "mono8";
  Mat out = proc.process(frame, enc);
  Mat coverage = proc.getRectMask();
  if (coverage.rows != h || coverage.cols != w || coverage.channels() != 1) return fail("the rect mask's geometry");
  // the mask is what the pipeline delivers for a white frame
  if (std::memcmp(coverage.data, out.data, (size_t)h * w) != 0) return fail("the rect mask differs from the undistorted white frame");
  proc.setOutputSize(w / 2, h / 2);
  proc.setOutputFit("letterbox");
  proc.setOutputRoi(0, 0, w, h / 2);
  Mat delivered = proc.getOutputMask(h, w, 1, "mono8");
  if (delivered.rows != h / 2 || delivered.cols != w / 2) return fail("the output mask's geometry");
  proc.setRectMask("valid");
  Mat valid = proc.getRectMask();
  std::FILE* f = std::fopen(out_path, "wb");
  if (!f) return fail("cannot write the output file");
  std::fwrite(coverage.data, 1, (size_t)h * w, f);
  std::fwrite(valid.data, 1, (size_t)h * w, f);
  std::fwrite(delivered.data, 1, (size_t)(h / 2) * (w / 2), f);
  std::fclose(f);
  std::printf("mask gpu OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "host") == 0) return host();
  if (argc == 6 && std::strcmp(argv[1], "gpu") == 0) return gpu(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), argv[5]);
  std::printf("usage: mask_test host | mask_test gpu <calibration.yaml> <width> <height> <out.bin>\n");
  return 2;
}
