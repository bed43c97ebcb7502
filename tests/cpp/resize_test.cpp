// The resize stage through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputSize / getOutputSize /
// getOutputCameraInfo, and -- with a device -- frames of the target size through process / apply / submit / collect.
// Built as C++14 like the reference.
// usage: resize_test host | resize_test gpu <width> <height> <target width> <target height> <out.bin>
//   gpu writes the native result of one Bayer frame, its resized result and the resized rgb8 result back to back
//   (w*h*3, tw*th*3, tw*th*3 bytes)
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <cstring>
#include <fstream>

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

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  RawImagePipeline proc(false, "", "", "");
  proc.setFlip(false);
  proc.setWhiteBalance(false);
  proc.setColorCalibration(false);
  proc.setGammaCorrection(true);
  proc.setGammaCorrectionMethod("custom");
  proc.setGammaCorrectionK(0.8);
  proc.setVignettingCorrection(false);
  proc.setColorEnhancer(false);
  proc.setUndistortion(false);
  int tw = -1, th = -1;
  proc.getOutputSize(tw, th);
  if (tw != 0 || th != 0) return fail("default size");
  proc.setOutputSize(640, 512);
  proc.getOutputSize(tw, th);
  if (tw != 640 || th != 512) return fail("size getter");
  const int bad[4][2] = {{0, 512}, {640, 0}, {-1, -1}, {16385, 16}};
  for (const auto& b : bad) {
    try {
      proc.setOutputSize(b[0], b[1]);
      return fail("invalid size accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("16384") == std::string::npos) return fail("the message does not name the rule");
    }
    proc.getOutputSize(tw, th);
    if (tw != 640 || th != 512) return fail("size changed by a refused call");
  }
  {
    int h = 0, w = 0;
    Mat K, P;
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    if (h != 512 || w != 640 || K.rows != 3 || K.cols != 3 || P.rows != 3 || P.cols != 4) return fail("camera info geometry");
    Mat K0 = proc.getDistCameraMatrix();
    const double* k = reinterpret_cast<const double*>(K.data);
    const double* k0 = reinterpret_cast<const double*>(K0.data);
    if (k[0] != k0[0] * 0.5 || k[2] != 0.5 * (k0[2] + 0.5) - 0.5 || k[4] != k0[4] * 0.5 || k[8] != k0[8]) return fail("camera matrix");
    proc.setOutputSize(0, 0);
    proc.getOutputCameraInfo(1024, 1280, 1, "bayer_rggb8", h, w, K, P);
    k = reinterpret_cast<const double*>(K.data);
    if (h != 1024 || w != 1280 || std::memcmp(k, k0, 9 * sizeof(double)) != 0) return fail("camera info without a target");
  }
  if (mode == "host") {
    proc.setOutputSize(4, 4);
    try {
      Mat img = make_u8(8, 8, 1);
      std::string enc = "bayer_rggb8";
      proc.apply(img, enc);
      return fail("frame processed without a device");
    } catch (const std::invalid_argument&) {
      return fail("a target refused by the facade");
    } catch (const std::runtime_error& e) {
      std::printf("expected failure: %s\n", e.what());
    }
    std::printf("resize host OK\n");
    return 0;
  }
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
  tw = std::atoi(argv[4]);
  th = std::atoi(argv[5]);
  Mat bayer = make_u8(h, w, 1);
  unsigned s = 12345u;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      s = s * 1664525u + 1013904223u;  // LCG, reproduced by the Python side of the test
      bayer.data[(size_t)y * bayer.step + x] = (uint8_t)(s >> 24);
    }
  std::ofstream f(argv[6], std::ios::binary);
  std::string enc = "bayer_rggb8";
  Mat native = proc.process(bayer, enc);
  if (enc != "bgr8" || native.rows != h || native.cols != w || native.channels() != 3) return fail("native geometry");
  f.write(reinterpret_cast<const char*>(native.data), (std::streamsize)w * h * 3);
  proc.setOutputSize(tw, th);
  enc = "bayer_rggb8";
  Mat small = proc.process(bayer, enc);
  if (enc != "bgr8" || small.rows != th || small.cols != tw || small.channels() != 3) return fail("resized geometry");
  if (!proc.getProcessedImage().empty()) return fail("processed image under a resize");
  if (proc.getDistDebayeredImage().rows != h || proc.getDistDebayeredImage().cols != w) return fail("debayered tap under a resize");
  f.write(reinterpret_cast<const char*>(small.data), (std::streamsize)tw * th * 3);
  {  // apply re-seats, submit / collect deliver the same bytes
    Mat inplace = bayer.clone();
    std::string e2 = "bayer_rggb8";
    if (!proc.apply(inplace, e2) || e2 != "bgr8" || inplace.rows != th || inplace.cols != tw) return fail("apply re-seat");
    if (std::memcmp(inplace.data, small.data, (size_t)tw * th * 3) != 0) return fail("apply != process");
    std::string e3, e4;
    const uint64_t t1 = proc.submit(bayer, "bayer_rggb8"), t2 = proc.submit(bayer, "bayer_rggb8");
    Mat v = proc.collectView(t1, e3);
    if (e3 != "bgr8" || v.rows != th || v.cols != tw || std::memcmp(v.data, small.data, (size_t)tw * th * 3) != 0) return fail("collectView != process");
    Mat c = proc.collect(t2, e4);
    if (e4 != "bgr8" || std::memcmp(c.data, small.data, (size_t)tw * th * 3) != 0) return fail("collect != process");
  }
  proc.setOutputFormat("rgb8");
  enc = "bayer_rggb8";
  Mat rgb = proc.process(bayer, enc);
  if (enc != "rgb8" || rgb.rows != th || rgb.cols != tw || rgb.channels() != 3) return fail("rgb8 geometry");
  f.write(reinterpret_cast<const char*>(rgb.data), (std::streamsize)tw * th * 3);
  std::printf("resize gpu OK\n");
  return 0;
}
