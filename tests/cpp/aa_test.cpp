// The antialiased filters of the resize stage through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputInterpolation /
// getOutputInterpolation take "linear_aa" and "cubic_aa", the plain names stay refused, the factor-64 refusal comes through
// getOutputCameraInfo and the camera matrices are the linear ones.  No device needed.  Built as C++14 like the reference.
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
  for (const char* name : {"linear_aa", "cubic_aa"}) {
    proc.setOutputInterpolation(name);
    if (proc.getOutputInterpolation() != name) return fail("getter");
    for (const char* bad : {"", "cubic", "nearest", "lanczos", "linear_AA", "cubic_aa ", "bicubic"}) {
      try {
        proc.setOutputInterpolation(bad);
        return fail("invalid name accepted");
      } catch (const std::invalid_argument& e) {
        const std::string msg = e.what();
        if (msg.find("\"linear\" or \"area\"") == std::string::npos || msg.find("\"linear_aa\" or \"cubic_aa\"") == std::string::npos)
          return fail("the message does not name the rule");
      }
      if (proc.getOutputInterpolation() != name) return fail("interpolation changed by a refused call");
    }
    int h = 0, w = 0;
    Mat K, P, K2, P2;
    proc.setOutputSize(320, 256);
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    if (h != 256 || w != 320) return fail("geometry under an antialiased filter");
    proc.setOutputInterpolation("linear");
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K2, P2);
    if (std::memcmp(K.data, K2.data, 9 * sizeof(double)) != 0 || std::memcmp(P.data, P2.data, 12 * sizeof(double)) != 0) return fail("camera matrices differ");
    proc.setOutputInterpolation(name);
    proc.setOutputSize(1281, 1030);  // an upscale is accepted
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    if (w != 1281 || h != 1030) return fail("upscale");
    proc.setOutputSize(20, 16);  // exactly 64 on both axes
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    if (w != 20 || h != 16) return fail("a factor of 64");
    proc.setOutputSize(20, 15);  // 1024 rows to 15: beyond 64
    try {
      proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
      return fail("a factor above 64 accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("64") == std::string::npos) return fail("the refusal does not name the rule");
    }
    proc.setOutputSize(1280, 1024);  // F's own size: the identity under any name
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    if (h != 1024 || w != 1280) return fail("identity");
  }
  std::printf("aa host OK\n");
  return 0;
}
