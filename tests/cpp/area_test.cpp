// The interpolation of the resize stage through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputInterpolation /
// getOutputInterpolation, the refusals of "area" through getOutputCameraInfo and the unchanged camera matrices.  No device needed.
// Built as C++14 like the reference.
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <cstring>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

int main() {
  RawImagePipeline proc(false, "", "", "");
  proc.setFlip(false);
  proc.setUndistortion(false);
  if (proc.getOutputInterpolation() != "linear") return fail("default interpolation");
  proc.setOutputInterpolation("area");
  if (proc.getOutputInterpolation() != "area") return fail("getter");
  for (const char* bad : {"", "Area", "cubic", "nearest", "area "}) {
    try {
      proc.setOutputInterpolation(bad);
      return fail("invalid name accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("\"linear\" or \"area\"") == std::string::npos) return fail("the message does not name the rule");
    }
    if (proc.getOutputInterpolation() != "area") return fail("interpolation changed by a refused call");
  }
  int h = 0, w = 0;
  Mat K, P, K2, P2;
  proc.setOutputSize(320, 256);
  proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
  if (h != 256 || w != 320) return fail("geometry under area");
  proc.setOutputInterpolation("linear");
  proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K2, P2);
  if (std::memcmp(K.data, K2.data, 9 * sizeof(double)) != 0 || std::memcmp(P.data, P2.data, 12 * sizeof(double)) != 0) return fail("camera matrices differ");
  proc.setOutputSize(1281, 1024);  // linear enlarges, area refuses
  proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
  if (w != 1281) return fail("linear upscale");
  proc.setOutputInterpolation("area");
  try {
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    return fail("an upscale accepted under area");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("downscale") == std::string::npos) return fail("the refusal does not name the rule");
  }
  proc.setOutputSize(1280, 1024);  // F's own size: the identity under either name
  proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
  if (h != 1024 || w != 1280) return fail("identity under area");
  std::printf("area host OK\n");
  return 0;
}
