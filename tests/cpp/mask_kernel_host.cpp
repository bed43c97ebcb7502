// rect_mask_kernel<false / true> and mask_threshold_kernel of csrc/rip_mask.hip executed on the host, thread by thread over the
// launcher's own grid (hip_host_stub).  The maps of a case are a heap block of exactly drows x dcols x 8 bytes that starts `map_phase`
// (0 or 8) bytes into a 16-byte aligned allocation; the mask is written into a heap block that ends with the last mask byte and starts
// `dst_off` bytes into a 16-byte aligned allocation, rows `pitch` bytes apart, 0xA5 everywhere beforehand.  The whole block goes to the
// output file: the test compares the rows with the oracle's remap of a white image and everything else with the sentinel.  Built with
// clang++, -I hip_host_stub in front of the ROCm headers; with -fsanitize=address,undefined it also proves that no access leaves a
// buffer and that no wide access is misaligned.
// usage: mask_kernel_host cases.bin out.bin
//   cases.bin: int32 n, then per case int32 {drows, dcols, src_rows, src_cols, binary, pitch, dst_off, map_phase} and drows * dcols * 2 floats
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_mask.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// mask_threshold_kernel on images of every width 1 .. 70 and 1023 .. 1026, 3 rows, pitches of the staging rule (16) and of 4: every
// byte of the dwords that hold a pixel is v == 255 ? 255 : 0 of what was there, every other byte of the pitch is what it was, and the
// block is exactly rows x pitch bytes
static int threshold_cases() {
  int bad = 0;
  std::vector<int> widths;
  for (int w = 1; w <= 70; w++) widths.push_back(w);
  for (int w = 1023; w <= 1026; w++) widths.push_back(w);
  for (int w : widths)
    for (size_t align : {(size_t)16, (size_t)4}) {
      const int rows = 3;
      const size_t step = ((size_t)w + align - 1) & ~(align - 1);
      void* block = nullptr;
      if (posix_memalign(&block, 16, step * rows) != 0) return 1;
      uint8_t* img = (uint8_t*)block;
      std::vector<uint8_t> was(step * rows);
      for (size_t i = 0; i < step * rows; i++) was[i] = img[i] = (uint8_t)((i * 37u + (i >> 3)) % 5 == 0 ? 255 : (i * 131u + 7u) % 256);
      rip::MaskThresholdParams t = {img, step, rows, w};
      rip::LaunchInfo info = {};
      if (!rip::launch_mask_threshold(t, nullptr, &info) || strcmp(info.kernel, "mask_threshold_kernel") != 0) { printf("threshold refused width %d\n", w); bad++; }
      for (size_t i = 0; i < step * rows && !bad; i++) {
        const bool touched = i % step < (((size_t)w + 3) & ~(size_t)3);  // the dwords that hold a pixel; the rest of the pitch stays
        if (img[i] != (touched ? (was[i] == 255 ? 255 : 0) : was[i])) { printf("threshold width %d pitch %zu: byte %zu is %u\n", w, step, i, img[i]); bad++; }
      }
      free(block);
    }
  alignas(16) static uint8_t buf[64];
  if (rip::launch_mask_threshold({buf + 1, 16, 2, 8}, nullptr, nullptr)) { printf("accepted a misaligned image\n"); bad++; }
  if (rip::launch_mask_threshold({buf, 18, 2, 8}, nullptr, nullptr)) { printf("accepted a pitch that is no multiple of 4\n"); bad++; }
  if (rip::launch_mask_threshold({buf, 8, 2, 9}, nullptr, nullptr)) { printf("accepted a pitch smaller than the padded row\n"); bad++; }
  if (rip::launch_mask_threshold({nullptr, 16, 2, 8}, nullptr, nullptr)) { printf("accepted a null image\n"); bad++; }
  return bad;
}

// what launch_rect_mask must refuse without launching
static int refusals() {
  alignas(16) static float maps[64];
  alignas(16) static uint8_t out[64];
  rip::RectMaskParams p = {};
  p.map_xy = maps; p.drows = 2; p.dcols = 4; p.src_rows = 3; p.src_cols = 5; p.dst = out; p.dst_step = 4;
  int bad = 0;
  if (!rip::launch_rect_mask(p, nullptr, nullptr)) { printf("the valid launch was refused\n"); bad++; }
  auto refused = [&](rip::RectMaskParams q, const char* what) {
    if (rip::launch_rect_mask(q, nullptr, nullptr)) { printf("accepted: %s\n", what); bad++; }
  };
  { auto q = p; q.map_xy = nullptr; refused(q, "null maps"); }
  { auto q = p; q.map_xy = maps + 1; refused(q, "maps that are not 8-byte aligned"); }
  { auto q = p; q.dst = nullptr; refused(q, "a null mask"); }
  { auto q = p; q.dst_step = 3; refused(q, "a pitch smaller than a row"); }
  { auto q = p; q.drows = 0; refused(q, "no row"); }
  { auto q = p; q.dcols = 0; refused(q, "no column"); }
  { auto q = p; q.src_rows = 0; refused(q, "an empty source"); }
  { auto q = p; q.src_cols = -1; refused(q, "a negative source"); }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: mask_kernel_host cases.bin out.bin\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) { printf("cannot open the files\n"); return 2; }
  int n = 0, bad = refusals() + threshold_cases();
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int i = 0; i < n; i++) {
    int h[8];
    if (fread(h, 4, 8, in) != 8) return 2;
    const int drows = h[0], dcols = h[1], binary = h[4];
    const size_t pitch = (size_t)h[5], dst_off = (size_t)h[6], map_phase = (size_t)h[7];
    const size_t map_bytes = (size_t)drows * dcols * 8;
    void* mblock = nullptr;  // exactly map_phase + map_bytes bytes: the maps end where the block ends
    if (posix_memalign(&mblock, 16, map_phase + map_bytes) != 0) return 2;
    float* maps = (float*)((uint8_t*)mblock + map_phase);
    if (fread(maps, 1, map_bytes, in) != map_bytes) return 2;
    const size_t total = dst_off + pitch * (size_t)(drows - 1) + (size_t)dcols;  // ends with the last mask byte
    void* dblock = nullptr;
    if (posix_memalign(&dblock, 16, total) != 0) return 2;
    memset(dblock, 0xA5, total);
    rip::RectMaskParams p = {};
    p.map_xy = maps; p.drows = drows; p.dcols = dcols; p.src_rows = h[2]; p.src_cols = h[3];
    p.dst = (uint8_t*)dblock + dst_off; p.dst_step = pitch; p.binary = binary;
    rip::LaunchInfo info = {};
    if (!rip::launch_rect_mask(p, nullptr, &info)) { printf("case %d refused\n", i); bad++; }
    else if (strcmp(info.kernel, binary ? "rect_mask_kernel<true>" : "rect_mask_kernel<false>") != 0 || info.grid_x != (unsigned)((dcols + 1023) / 1024) ||
             info.grid_y != (unsigned)drows || info.block != 256) {
      printf("case %d: launch record %s %u %u %u\n", i, info.kernel, info.grid_x, info.grid_y, info.block);
      bad++;
    }
    fwrite(dblock, 1, total, outf);
    free(mblock);
    free(dblock);
  }
  fclose(in);
  fclose(outf);
  printf("rect mask kernels on the host: %d cases, %d bad\n", n, bad);
  return bad ? 1 : 0;
}
