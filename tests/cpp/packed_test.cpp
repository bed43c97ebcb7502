// Packed 10- / 12-bit Bayer frames through the C++ facade (include/raw_image_pipeline/raw_image_pipeline.hpp): a one-channel
// uint8 Mat of rows x ROW BYTES, setDebayerPackedWidth / getDebayerPackedWidth.  Without a device (RIP_DEVICE=-1) the facade
// state and rip_debug_unpack on the known answers; with one ("frames" as the first argument) a flat colour packed in each of
// the four layouts goes through apply / process / submit + collect / submitTo and comes back as an ordinary uint8 bgr8 Mat
// whose every byte is known without a reference implementation.
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

static bool all_equal(const Mat& m, int rows, int cols, uint8_t b, uint8_t g, uint8_t r) {
  if (m.rows != rows || m.cols != cols || m.channels() != 3) return false;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const uint8_t* px = m.data + (size_t)y * m.step + (size_t)x * 3;
      if (px[0] != b || px[1] != g || px[2] != r) return false;
    }
  return true;
}

// one row of samples -> packed bytes, written from the layouts' definitions
static std::vector<uint8_t> pack_row(const std::vector<uint16_t>& s, const std::string& layout) {
  const int n = (int)s.size(), bits = layout[1] == '0' ? 10 : 12;
  std::vector<uint8_t> out(((size_t)n * bits + 7) / 8, 0);
  if (layout == "10p" || layout == "12p") {
    for (int x = 0; x < n; x++)
      for (int k = 0; k < bits; k++)
        if ((s[x] >> k) & 1) out[(size_t)(x * bits + k) >> 3] |= (uint8_t)(1u << ((x * bits + k) & 7));
  } else if (layout == "10_csi2") {
    for (int x = 0; x < n; x++) {
      out[(size_t)5 * (x >> 2) + (x & 3)] = (uint8_t)(s[x] >> 2);
      out[(size_t)5 * (x >> 2) + 4] |= (uint8_t)((s[x] & 3) << (2 * (x & 3)));
    }
  } else {
    for (int x = 0; x < n; x++) {
      out[(size_t)3 * (x >> 1) + (x & 1)] = (uint8_t)(s[x] >> 4);
      out[(size_t)3 * (x >> 1) + 2] |= (uint8_t)((s[x] & 15) << (4 * (x & 1)));
    }
  }
  return out;
}

static bool known_answer(const char* encoding, std::vector<uint8_t> bytes, std::vector<uint16_t> want) {
  std::vector<uint16_t> got(want.size(), 0xFFFF);
  if (rip_debug_unpack(encoding, bytes.data(), 0, 1, (int)want.size(), got.data()) != RIP_OK) return false;
  return got == want;
}

int main(int argc, char** argv) {
  RawImagePipeline proc(false, "", "", "");
  if (proc.getDebayerPackedWidth() != 0) return fail("default packed width");
  proc.setDebayerPackedWidth(132);
  if (proc.getDebayerPackedWidth() != 132) return fail("set packed width");
  bool threw = false;
  try {
    proc.setDebayerPackedWidth(-4);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw || proc.getDebayerPackedWidth() != 132) return fail("negative packed width");
  proc.setDebayerPackedWidth(0);
  if (!known_answer("bayer_rggb10p", {0xFF, 0x03, 0x50, 0x95, 0xAA}, {0x3FF, 0, 0x155, 0x2AA})) return fail("10p known answer");
  if (!known_answer("bayer_rggb10_csi2", {0xFF, 0x00, 0x55, 0xAA, 0x93}, {0x3FF, 0, 0x155, 0x2AA})) return fail("10_csi2 known answer");
  if (!known_answer("bayer_bggr12p", {0xBC, 0x3A, 0x12}, {0xABC, 0x123})) return fail("12p known answer");
  if (!known_answer("bayer_bggr12_csi2", {0xAB, 0x12, 0x3C}, {0xABC, 0x123})) return fail("12_csi2 known answer");
  uint16_t dummy[4];
  const uint8_t five[5] = {0};
  if (rip_debug_unpack("bayer_rggb8", five, 0, 1, 4, dummy) != RIP_ERR_INVALID_ARGUMENT) return fail("not a packed name");
  if (rip_debug_unpack("bayer_rggb10_csi2", five, 0, 1, 3, dummy) != RIP_ERR_INVALID_ARGUMENT) return fail("csi2 width rule");
  if (rip_debug_unpack("bayer_rggb10p", five, 4, 1, 4, dummy) != RIP_ERR_INVALID_ARGUMENT) return fail("pitch below a row");

  if (argc > 1 && std::string(argv[1]) == "frames") {
    const int rows = 70, cols = 132;
    proc.setWhiteBalance(false);
    proc.setUndistortion(false);
    proc.setFlip(true);
    proc.setFlipAngle(90);
    proc.setGammaCorrection(false);
    for (const char* layout : {"10p", "12p", "10_csi2", "12_csi2"}) {
      const bool ten = layout[1] == '0';
      // rggb, range (64, 1023) / (256, 4095): R at the white level -> 255, G at the black level -> 0,
      // B = 544 (255 * 480 / 959 = 127.6 -> 128) / 2176 (255 * 1920 / 3839 = 127.5 -> 128, half up)
      const uint16_t r = ten ? 1023 : 4095, g = ten ? 64 : 256, b = ten ? 544 : 2176;
      proc.setDebayer16BitRange(ten ? 64 : 256, ten ? 1023 : 4095);
      std::vector<uint16_t> even(cols), odd(cols);
      for (int x = 0; x < cols; x++) {
        even[x] = (x & 1) ? g : r;
        odd[x] = (x & 1) ? b : g;
      }
      const std::vector<uint8_t> pe = pack_row(even, layout), po = pack_row(odd, layout);
      const int rb = (int)pe.size(), pitch = rb + 5;  // padding columns: the width has to be spelled out
      std::vector<uint8_t> tight((size_t)rows * rb), padded((size_t)rows * pitch, 0xA5);
      for (int y = 0; y < rows; y++) {
        std::memcpy(&tight[(size_t)y * rb], (y & 1) ? po.data() : pe.data(), rb);
        std::memcpy(&padded[(size_t)y * pitch], (y & 1) ? po.data() : pe.data(), rb);
      }
#ifdef RIP_HAVE_OPENCV
      Mat frame(rows, rb, CV_8UC1, tight.data());
      Mat wide(rows, pitch, CV_8UC1, padded.data());
#else
      Mat frame(rows, rb, 1, tight.data());
      Mat wide(rows, pitch, 1, padded.data());
#endif
      const std::string name = std::string("bayer_rggb") + layout;
      for (const char* method : {"bilinear", "mht"}) {
        proc.setDebayerMethod(method);
        proc.setDebayerPackedWidth(0);
        std::string enc = name;
        Mat out = proc.process(frame, enc);
        if (enc != "bgr8" || !all_equal(out, cols, rows, 128, 0, 255)) return fail("process");
        enc = name;
        Mat in_place = frame;
        proc.apply(in_place, enc);
        if (enc != "bgr8" || !all_equal(in_place, cols, rows, 128, 0, 255)) return fail("apply");
        proc.setDebayerPackedWidth(cols);
        enc = name;
        out = proc.process(wide, enc);
        if (enc != "bgr8" || !all_equal(out, cols, rows, 128, 0, 255)) return fail("process with a width");
        const uint64_t t = proc.submit(wide, name);
        Mat got = proc.collect(t, enc);
        if (enc != "bgr8" || !all_equal(got, cols, rows, 128, 0, 255)) return fail("submit / collect");
        proc.setDebayerPackedWidth(0);
        uint8_t* pinned = static_cast<uint8_t*>(rip_host_alloc((size_t)rows * cols * 3));
        if (!pinned) return fail("rip_host_alloc");
        std::memset(pinned, 7, (size_t)rows * cols * 3);
#ifdef RIP_HAVE_OPENCV
        Mat dst(cols, rows, CV_8UC3, pinned);
#else
        Mat dst(cols, rows, 3, pinned);
#endif
        const uint64_t t2 = proc.submitTo(frame, name, dst);
        proc.collectView(t2, enc);
        const bool ok = enc == "bgr8" && all_equal(dst, cols, rows, 128, 0, 255);
        rip_host_free(pinned);
        if (!ok) return fail("submitTo");
      }
    }
    std::printf("packed frames OK\n");
  }
  std::printf("packed facade OK\n");
  return 0;
}
