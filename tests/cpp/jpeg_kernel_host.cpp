// The four kernels of csrc/rip_jpeg.hip executed on the host, thread by thread over the launchers' own grids (hip_host_stub), with the
// tables and the header of rip_jpeg.hpp's builders.  Every buffer of a case is a heap block of exactly the bytes the interface asks
// for: the source ends with its last pixel, the scratch is jpeg_coef_bytes / jpeg_interval_bytes, the destination starts `dst_off`
// bytes into a 16-byte aligned allocation and ends 7 bytes behind the last slot, 0xA5 everywhere beforehand.  The sizes and the whole
// destination go to the output file: the test compares them with tests/jpeg_reference.py, sentinels included.  Built with clang++,
// -I hip_host_stub in front of the ROCm headers; with -fsanitize=address,undefined it also proves that no access leaves a buffer
// and that no wide access is misaligned.
// usage: jpeg_kernel_host cases.bin out.bin
//   cases.bin: int32 n, then per case int32 {rows, cols, channels, quality, restart_rows, frames, slot, stride, dst_off, src_pitch}
//   and the source bytes; out.bin: per case uint32 sizes[frames], then dst_off + stride * (frames - 1) + slot + 7 bytes
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_jpeg.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static const int kBt601Full[10] = {3735, 19235, 9798, 16384, -10855, -5529, -2664, -13720, 16384, 0};

struct Case {
  rip::JpegParams p = {};
  rip::JpegTables tables;
  std::vector<uint8_t> header;
  void *src = nullptr, *dst = nullptr, *coef = nullptr, *intervals = nullptr;
  std::vector<uint32_t> sizes;
  size_t dst_bytes = 0;
  ~Case() { free(src), free(dst), free(coef), free(intervals); }
};

static bool make_case(Case& c, const int h[10], FILE* in) {
  const int rows = h[0], cols = h[1], channels = h[2], quality = h[3], restart_rows = h[4], frames = h[5];
  const size_t slot = (size_t)h[6], stride = (size_t)h[7], dst_off = (size_t)h[8], src_pitch = (size_t)h[9];
  const size_t src_bytes = src_pitch * (size_t)rows * (size_t)(frames - 1) + src_pitch * (size_t)(rows - 1) + (size_t)cols * channels;
  c.src = malloc(src_bytes);
  if (!c.src) return false;
  for (int f = 0; f < frames; f++) {  // the file holds whole pitches; the block ends with the last pixel
    std::vector<uint8_t> frame(src_pitch * (size_t)rows);
    if (fread(frame.data(), 1, frame.size(), in) != frame.size()) return false;
    const size_t at = src_pitch * (size_t)rows * (size_t)f;
    memcpy((uint8_t*)c.src + at, frame.data(), src_bytes - at < frame.size() ? src_bytes - at : frame.size());
  }
  c.dst_bytes = dst_off + stride * (size_t)(frames - 1) + slot + 7;
  if (posix_memalign(&c.dst, 16, c.dst_bytes) != 0) return false;
  memset(c.dst, 0xA5, c.dst_bytes);
  if (posix_memalign(&c.coef, 16, rip::jpeg_coef_bytes(rows, cols, channels, frames)) != 0) return false;
  c.intervals = malloc(rip::jpeg_interval_bytes(rows, channels, restart_rows, frames));
  c.sizes.assign((size_t)frames, 0xDEADBEEFu);
  uint8_t q[128];
  rip::jpeg_build_tables(quality, c.tables, q);
  c.header.resize((size_t)rip::jpeg_header_bytes(channels));
  if (rip::jpeg_build_header(rows, cols, channels, restart_rows, q, c.header.data()) != (int)c.header.size()) return false;
  rip::JpegParams& p = c.p;
  p.src = (const uint8_t*)c.src, p.src_step = src_pitch, p.src_frame_stride = src_pitch * (size_t)rows;
  p.dst = (uint8_t*)c.dst + dst_off, p.dst_step = slot, p.dst_frame_stride = stride;
  p.rows = rows, p.cols = cols, p.channels = channels, p.n_frames = frames, p.restart_rows = restart_rows;
  for (int k = 0; k < 3; k++) p.m.y[k] = kBt601Full[k], p.m.cb[k] = kBt601Full[3 + k], p.m.cr[k] = kBt601Full[6 + k];
  p.m.yoff = kBt601Full[9];
  p.tables = &c.tables, p.header = c.header.data();
  p.coef = (int16_t*)c.coef, p.intervals = (uint32_t*)c.intervals, p.sizes = c.sizes.data();
  return true;
}

// what the launch functions must refuse without launching
static int refusals(const rip::JpegParams& good) {
  int bad = 0;
  auto refused = [&](rip::JpegParams q, const char* what) {
    if (rip::launch_jpeg_transform(q, nullptr, nullptr) || rip::launch_jpeg_size(q, nullptr, nullptr) || rip::launch_jpeg_scan(q, nullptr, nullptr) ||
        rip::launch_jpeg_write(q, nullptr, nullptr)) {
      printf("accepted: %s\n", what);
      bad++;
    }
  };
  { auto q = good; q.src = nullptr; refused(q, "a null source"); }
  { auto q = good; q.dst = nullptr; refused(q, "a null destination"); }
  { auto q = good; q.tables = nullptr; refused(q, "no tables"); }
  { auto q = good; q.header = nullptr; refused(q, "no header"); }
  { auto q = good; q.coef = nullptr; refused(q, "no coefficient scratch"); }
  { auto q = good; q.intervals = nullptr; refused(q, "no interval scratch"); }
  { auto q = good; q.sizes = nullptr; refused(q, "no sizes"); }
  { auto q = good; q.channels = 2; refused(q, "two channels"); }
  { auto q = good; q.rows = 0; refused(q, "no row"); }
  { auto q = good; q.cols = 65536; refused(q, "a width beyond 65535"); }
  { auto q = good; q.restart_rows = 0; refused(q, "no restart rows"); }
  { auto q = good; q.restart_rows = 65; refused(q, "65 restart rows"); }
  { auto q = good; q.src_step = (size_t)q.cols * q.channels - 1; refused(q, "a source pitch smaller than a row"); }
  { auto q = good; q.dst_step = (size_t)rip::jpeg_header_bytes(q.channels) + 1; refused(q, "a slot below header + 2"); }
  { auto q = good; q.dst_frame_stride = q.dst_step - 1; refused(q, "a frame stride below the slot"); }
  { auto q = good; q.n_frames = 0; refused(q, "no frame"); }
  { auto q = good; q.coef = (int16_t*)((uint8_t*)q.coef + 2); refused(q, "a misaligned coefficient scratch"); }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: jpeg_kernel_host cases.bin out.bin\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) { printf("cannot open the files\n"); return 2; }
  int n = 0, bad = 0;
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int i = 0; i < n; i++) {
    int h[10];
    if (fread(h, 4, 10, in) != 10) return 2;
    Case c;
    if (!make_case(c, h, in)) { printf("case %d: cannot be set up\n", i); return 2; }
    if (i == 0) bad += refusals(c.p);
    rip::LaunchInfo info[4] = {};
    const bool ok = rip::launch_jpeg_transform(c.p, nullptr, &info[0]) && rip::launch_jpeg_size(c.p, nullptr, &info[1]) &&
                    rip::launch_jpeg_scan(c.p, nullptr, &info[2]) && rip::launch_jpeg_write(c.p, nullptr, &info[3]);
    const unsigned intervals = (unsigned)rip::jpeg_intervals(c.p.rows, c.p.channels, c.p.restart_rows);
    const unsigned want_x[4] = {(unsigned)((rip::jpeg_blocks(c.p.rows, c.p.cols, c.p.channels) + 63) / 64), (intervals + 63) / 64,
                                ((unsigned)c.p.n_frames + 63) / 64, (intervals + 63) / 64 + 1};
    const char* want_name[4] = {c.p.channels == 3 ? "jpeg_transform_kernel<true>" : "jpeg_transform_kernel<false>", "jpeg_size_kernel", "jpeg_scan_kernel",
                                "jpeg_write_kernel"};
    if (!ok) { printf("case %d refused\n", i); bad++; }
    for (int k = 0; ok && k < 4; k++)
      if (strcmp(info[k].kernel, want_name[k]) != 0 || info[k].grid_x != want_x[k] || info[k].grid_y != 1 || info[k].block != 64) {
        printf("case %d: launch record %s %u %u %u\n", i, info[k].kernel, info[k].grid_x, info[k].grid_y, info[k].block);
        bad++;
      }
    fwrite(c.sizes.data(), 4, c.sizes.size(), outf);
    fwrite(c.dst, 1, c.dst_bytes, outf);
  }
  fclose(in);
  fclose(outf);
  printf("jpeg kernels on the host: %d cases, %d bad\n", n, bad);
  return bad ? 1 : 0;
}
