// The output format "jpeg" through include/raw_image_pipeline/raw_image_pipeline.hpp: setOutputFormat("jpeg"), setOutputJpeg /
// getOutputJpeg -- defaults, the ranges and their refusal -- and getOutputJpegSizes, which needs a device, without one ("host"); on a
// device ("gpu") the stream of one Bayer frame through process() and the two-call protocol of getOutputJpegSizes on real lengths.
// Built as C++14 like the reference.
// usage: jpeg_test host | jpeg_test gpu <width> <height> <out.bin>
//   gpu writes the native result (w*h*3 bytes), the count of lengths and the first length (uint32 each) and the slot's bytes
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdio>
#include <fstream>
#include <string>

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
  const std::string mode = argc > 1 ? argv[1] : "";
  if (!((mode == "host" && argc == 2) || (mode == "gpu" && argc == 5))) return fail("usage: jpeg_test host | jpeg_test gpu <width> <height> <out.bin>");
  RawImagePipeline proc(false, "", "", "");
  int quality = 0, restart_rows = 0;
  proc.getOutputJpeg(quality, restart_rows);
  if (quality != 90 || restart_rows != 1) return fail("the defaults");
  const int good[4][2] = {{1, 1}, {100, 64}, {50, 2}, {75, 3}};
  for (const auto& g : good) {
    proc.setOutputJpeg(g[0], g[1]);
    proc.getOutputJpeg(quality, restart_rows);
    if (quality != g[0] || restart_rows != g[1]) return fail("the getter does not return what was set");
  }
  const int bad[6][2] = {{0, 1}, {101, 1}, {-5, 1}, {90, 0}, {90, 65}, {90, -1}};
  for (const auto& b : bad) {
    try {
      proc.setOutputJpeg(b[0], b[1]);
      return fail("a value outside the ranges accepted");
    } catch (const std::invalid_argument& e) {
      if (std::string(e.what()).find("output jpeg") == std::string::npos) return fail("the refusal does not name the setting");
    }
  }
  proc.getOutputJpeg(quality, restart_rows);
  if (quality != 75 || restart_rows != 3) return fail("a refused value changed the setting");
  for (const char* fmt : {"jpeg", "native"}) {
    proc.setOutputFormat(fmt);
    if (proc.getOutputFormat() != fmt) return fail("the format getter");
  }
  try {
    proc.setOutputFormat("jpg");
    return fail("an unknown format accepted");
  } catch (const std::invalid_argument& e) {
    if (std::string(e.what()).find("'jpeg'") == std::string::npos) return fail("the format refusal does not list the new name");
  }
  if (mode == "host") {
    try {  // the lengths live on the device
      (void)proc.getOutputJpegSizes();
      return fail("sizes without a device");
    } catch (const std::exception&) {
    }
    std::printf("jpeg host OK\n");
    return 0;
  }
  proc.setFlip(false);
  proc.setWhiteBalance(false);
  proc.setColorCalibration(false);
  proc.setGammaCorrection(true);
  proc.setGammaCorrectionMethod("custom");
  proc.setGammaCorrectionK(0.8);
  proc.setVignettingCorrection(false);
  proc.setColorEnhancer(false);
  proc.setUndistortion(false);
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
  Mat bayer = make_u8(h, w, 1);
  unsigned s = 12345u;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      s = s * 1664525u + 1013904223u;  // LCG: any frame will do, the native result travels with the stream
      bayer.data[(size_t)y * bayer.step + x] = (uint8_t)(s >> 24);
    }
  std::ofstream f(argv[4], std::ios::binary);
  if (!proc.getOutputJpegSizes().empty()) return fail("lengths before the first frame call");
  std::string enc = "bayer_rggb8";
  Mat native = proc.process(bayer, enc);
  if (enc != "bgr8" || native.channels() != 3 || native.rows != h || native.cols != w) return fail("native geometry");
  if (!proc.getOutputJpegSizes().empty()) return fail("lengths after a native frame call");
  for (int y = 0; y < h; y++) f.write(reinterpret_cast<const char*>(native.data + (size_t)y * native.step), (std::streamsize)w * 3);
  proc.setOutputFormat("jpeg");
  proc.setOutputJpeg(85, 2);
  enc = "bayer_rggb8";
  Mat slot = proc.process(bayer, enc);
  if (enc != "jpeg" || slot.rows != 1 || slot.channels() != 1) return fail("the delivered slot's geometry");
  const std::vector<uint32_t> sizes = proc.getOutputJpegSizes();
  if (sizes.size() != 1 || sizes[0] == 0 || sizes[0] > (uint32_t)slot.cols) return fail("the stream length");
  const uint32_t head[2] = {(uint32_t)sizes.size(), sizes[0]};
  f.write(reinterpret_cast<const char*>(head), 8);
  f.write(reinterpret_cast<const char*>(slot.data), (std::streamsize)sizes[0]);
  proc.setOutputFormat("native");
  enc = "bayer_rggb8";
  (void)proc.process(bayer, enc);
  if (!proc.getOutputJpegSizes().empty()) return fail("the lengths of an earlier call outlived a native frame call");
  std::printf("jpeg gpu OK\n");
  return 0;
}
