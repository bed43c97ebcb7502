// The 16-bit range through the C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp): setDebayer16Bit,
// setDebayer16BitRange / getDebayer16BitRange, invalid ranges rejected with std::invalid_argument and nothing changed.
// Without a device (RIP_DEVICE=-1) that is all; with one (RIP_DEVICE >= 0, "frames" as the first argument) a one-channel Mat of
// 16-bit samples goes through apply / process / submit + collect / submitTo and comes back as an ordinary uint8 bgr8 Mat: a
// flat colour at the white level, so every output byte is known without a reference implementation.
#include <raw_image_pipeline/raw_image_pipeline.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using raw_image_pipeline::Mat;
using raw_image_pipeline::RawImagePipeline;

static int fail(const char* what) {
  std::printf("FAIL: %s\n", what);
  return 1;
}

static bool rejected(RawImagePipeline& proc, int black, int white) {
  try {
    proc.setDebayer16BitRange(black, white);
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static bool all_equal(const Mat& m, int rows, int cols, uint8_t b, uint8_t g, uint8_t r) {
  if (m.rows != rows || m.cols != cols || m.channels() != 3) return false;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const uint8_t* px = m.data + (size_t)y * m.step + (size_t)x * 3;
      if (px[0] != b || px[1] != g || px[2] != r) return false;
    }
  return true;
}

int main(int argc, char** argv) {
  RawImagePipeline proc(false, "", "", "");
  if (proc.getDebayer16BitRange() != std::make_pair(0, 0)) return fail("default range");
  proc.setDebayer16Bit(true);
  proc.setDebayer16BitRange(64, 1023);
  if (proc.getDebayer16BitRange() != std::make_pair(64, 1023)) return fail("set range");
  if (!rejected(proc, -1, 100) || !rejected(proc, 0, 65536) || !rejected(proc, 500, 500) || !rejected(proc, 600, 500) || !rejected(proc, 5, 0))
    return fail("invalid range not rejected");
  if (proc.getDebayer16BitRange() != std::make_pair(64, 1023)) return fail("rejected range changed the handle");
  proc.setDebayer16BitRange(0, 0);
  if (proc.getDebayer16BitRange() != std::make_pair(0, 0)) return fail("range off");
  proc.setDebayer16BitRange(64, 1023);

  if (argc > 1 && std::string(argv[1]) == "frames") {
    const int rows = 70, cols = 132;
    proc.setWhiteBalance(false);
    proc.setUndistortion(false);
    proc.setFlip(true);
    proc.setFlipAngle(90);
    proc.setGammaCorrection(false);
    // rggb: R = 1023 (white level -> 255), G = 64 (black level -> 0), B = 544 (255 * 480 / 959 = 127.6 -> 128)
    std::vector<uint16_t> samples((size_t)rows * cols);
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) samples[(size_t)y * cols + x] = (y & 1) ? ((x & 1) ? 544 : 64) : ((x & 1) ? 64 : 1023);
#ifdef RIP_HAVE_OPENCV
    Mat frame(rows, cols, CV_16UC1, samples.data());
#else
    Mat frame(rows, cols, 1, reinterpret_cast<uint8_t*>(samples.data()), (size_t)cols * 2);
#endif
    for (const char* method : {"bilinear", "mht"}) {
      proc.setDebayerMethod(method);
      std::string enc = "bayer_rggb16";
      Mat out = proc.process(frame, enc);
      if (enc != "bgr8" || !all_equal(out, cols, rows, 128, 0, 255)) return fail("process");
      enc = "bayer_rggb16";
      Mat in_place = frame;
      proc.apply(in_place, enc);
      if (enc != "bgr8" || !all_equal(in_place, cols, rows, 128, 0, 255)) return fail("apply");
      const uint64_t t = proc.submit(frame, "bayer_rggb16");
      Mat got = proc.collect(t, enc);
      if (enc != "bgr8" || !all_equal(got, cols, rows, 128, 0, 255)) return fail("submit / collect");
      uint8_t* pinned = static_cast<uint8_t*>(rip_host_alloc((size_t)rows * cols * 3));
      if (!pinned) return fail("rip_host_alloc");
      std::memset(pinned, 7, (size_t)rows * cols * 3);
#ifdef RIP_HAVE_OPENCV
      Mat dst(cols, rows, CV_8UC3, pinned);
#else
      Mat dst(cols, rows, 3, pinned);
#endif
      const uint64_t t2 = proc.submitTo(frame, "bayer_rggb16", dst);
      proc.collectView(t2, enc);
      const bool ok = enc == "bgr8" && all_equal(dst, cols, rows, 128, 0, 255);
      rip_host_free(pinned);
      if (!ok) return fail("submitTo");
    }
    std::printf("raw16 frames OK\n");
  }
  std::printf("raw16 range OK\n");
  return 0;
}
