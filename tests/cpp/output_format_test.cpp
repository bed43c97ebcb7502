// The output stage through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputFormat / getOutputFormat /
// setOutputNormalization, rgb8 and mono8 through the frame calls as CV_8UC3 / CV_8UC1, the planar float formats refused by them.
// Built as C++14 like the reference.
// usage: output_format_test host | output_format_test gpu <width> <height> <out.bin>
//   gpu writes the native, rgb8 and mono8 results of one Bayer frame back to back (w*h*3, w*h*3, w*h bytes)
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
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
  if (proc.getOutputFormat() != "native") return fail("default format");
  proc.setOutputFormat("rgb_chw_bf16");
  if (proc.getOutputFormat() != "rgb_chw_bf16") return fail("format getter");
  try {
    proc.setOutputFormat("rgb_hwc_f32");
    return fail("unknown format accepted");
  } catch (const std::invalid_argument&) {
  }
  if (proc.getOutputFormat() != "rgb_chw_bf16") return fail("format changed by a refused name");
  proc.setOutputNormalization(255.0, {0.485, 0.456, 0.406}, {0.229, 0.224, 0.225});
  try {
    proc.setOutputNormalization(255.0, {0.0, 0.0, 0.0}, {1.0, 0.0, 1.0});
    return fail("std 0 accepted");
  } catch (const std::invalid_argument&) {
  }
  try {
    proc.setOutputNormalization(0.0, {0.0, 0.0, 0.0}, {1.0, 1.0, 1.0});
    return fail("divisor 0 accepted");
  } catch (const std::invalid_argument&) {
  }
  try {
    proc.setOutputNormalization(255.0, {0.0, 0.0}, {1.0, 1.0, 1.0});
    return fail("two means accepted");
  } catch (const std::invalid_argument&) {
  }
  {
    double divisor = 0, mean[3], sd[3];
    if (rip_get_output_normalization(proc.handle(), &divisor, mean, sd) != RIP_OK) return fail("normalisation getter");
    if (divisor != 255.0 || mean[2] != 0.406 || sd[1] != 0.224) return fail("normalisation changed by a refused call");
  }
  // the planar float formats: the frame calls of the facade throw before they reach the library (device or not)
  for (const char* name : {"rgb_chw_f32", "rgb_chw_f16", "rgb_chw_bf16", "bgr_chw_f32", "bgr_chw_f16", "bgr_chw_bf16"}) {
    proc.setOutputFormat(name);
    Mat img = make_u8(8, 8, 1);
    std::string enc = "bayer_rggb8";
    try {
      proc.process(img, enc);
      return fail("float format through process");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("C interface") == std::string::npos) return fail("the message does not point at the C interface");
    }
    try {
      proc.apply(img, enc);
      return fail("float format through apply");
    } catch (const std::invalid_argument&) {
    }
    try {
      proc.submit(img, enc);
      return fail("float format through submit");
    } catch (const std::invalid_argument&) {
    }
  }
  if (mode == "host") {
    proc.setOutputFormat("rgb8");
    try {
      Mat img = make_u8(8, 8, 1);
      std::string enc = "bayer_rggb8";
      proc.apply(img, enc);
      return fail("frame processed without a device");
    } catch (const std::invalid_argument&) {
      return fail("rgb8 refused by the facade");
    } catch (const std::runtime_error& e) {
      std::printf("expected failure: %s\n", e.what());
    }
    std::printf("output format host OK\n");
    return 0;
  }
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
  Mat bayer = make_u8(h, w, 1);
  unsigned s = 12345u;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      s = s * 1664525u + 1013904223u;  // LCG, reproduced by the Python side of the test
      bayer.data[(size_t)y * bayer.step + x] = (uint8_t)(s >> 24);
    }
  std::ofstream f(argv[4], std::ios::binary);
  proc.setOutputFormat("native");
  std::string enc = "bayer_rggb8";
  Mat native = proc.process(bayer, enc);
  if (enc != "bgr8" || native.channels() != 3) return fail("native geometry");
  f.write(reinterpret_cast<const char*>(native.data), (std::streamsize)w * h * 3);
  proc.setOutputFormat("rgb8");
  enc = "bayer_rggb8";
  Mat rgb = proc.process(bayer, enc);
  if (enc != "rgb8" || rgb.rows != h || rgb.cols != w || rgb.channels() != 3) return fail("rgb8 geometry");
  if (!proc.getProcessedImage().empty()) return fail("processed image under a format");
  if (proc.getDistDebayeredImage().rows != h) return fail("debayered tap under a format");
  f.write(reinterpret_cast<const char*>(rgb.data), (std::streamsize)w * h * 3);
  {  // apply re-seats, submit / collect deliver the same bytes
    Mat inplace = bayer.clone();
    std::string e2 = "bayer_rggb8";
    if (!proc.apply(inplace, e2) || e2 != "rgb8" || inplace.channels() != 3) return fail("apply re-seat");
    if (std::memcmp(inplace.data, rgb.data, (size_t)w * h * 3) != 0) return fail("apply != process");
    std::string e3, e4;
    const uint64_t t1 = proc.submit(bayer, "bayer_rggb8"), t2 = proc.submit(bayer, "bayer_rggb8");
    Mat v = proc.collectView(t1, e3);
    if (e3 != "rgb8" || v.channels() != 3 || std::memcmp(v.data, rgb.data, (size_t)w * h * 3) != 0) return fail("collectView != process");
    Mat c = proc.collect(t2, e4);
    if (e4 != "rgb8" || std::memcmp(c.data, rgb.data, (size_t)w * h * 3) != 0) return fail("collect != process");
  }
  proc.setOutputFormat("mono8");
  enc = "bayer_rggb8";
  Mat grey = proc.process(bayer, enc);
  if (enc != "mono8" || grey.rows != h || grey.cols != w || grey.channels() != 1) return fail("mono8 geometry");
  f.write(reinterpret_cast<const char*>(grey.data), (std::streamsize)w * h);
  {
    std::string e5;
    Mat c = proc.collect(proc.submit(bayer, "bayer_rggb8"), e5);
    if (e5 != "mono8" || c.channels() != 1 || std::memcmp(c.data, grey.data, (size_t)w * h) != 0) return fail("mono8 collect != process");
  }
  std::printf("output format gpu OK\n");
  return 0;
}
