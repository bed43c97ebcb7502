// The kernels of csrc/rip_area.hip executed on the host, thread by thread over the launcher's own grid (hip_host_stub), into exactly
// sized heap buffers and from exactly sized tables laid out as rip_batch.cpp lays them out.  The cases and their source frames come
// from a file tests/test_resize_area.py writes; every byte of every destination buffer -- delivered pixels, row padding, frame gaps
// -- goes to a second file, which the test compares with tests/area_reference.py.  Built with clang++, -I hip_host_stub in front of
// the ROCm headers; with -fsanitize=address,undefined it also proves that no access leaves a buffer.
// usage: area_kernel_host <cases.bin> <out.bin>
//   cases.bin: int32 count, then per case 9 x int32 (R, C, H, W, channels, frames, dst row padding, dst offset, frame gap) and the
//   frames' R * C * channels tight bytes each.  out.bin: per case the destination buffer, 0xA5 where nothing was written.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_area.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rip_host.hpp"

static int run(FILE* in, FILE* out) {
  int32_t h[9];
  if (fread(h, 4, 9, in) != 9) return 1;
  const int R = h[0], C = h[1], H = h[2], W = h[3], cn = h[4], n = h[5];
  const size_t dst_pad = h[6], dst_off = h[7], gap = h[8];
  const size_t sstep = ((size_t)C * cn + 15) & ~(size_t)15, sframe = sstep * R;
  uint8_t* src = (uint8_t*)aligned_alloc(16, sframe * n);  // exactly the staging image
  memset(src, 0x5A, sframe * n);
  for (int f = 0; f < n; f++)
    for (int y = 0; y < R; y++)
      if (fread(src + f * sframe + y * sstep, 1, (size_t)C * cn, in) != (size_t)C * cn) return 1;
  const size_t dstep = (size_t)W * cn + dst_pad, dframe = dstep * H + gap;
  const size_t total = dst_off + dframe * (n - 1) + dstep * (H - 1) + (size_t)W * cn;  // ends with the last delivered byte
  uint8_t* base = (uint8_t*)aligned_alloc(16, (total + 15) & ~(size_t)15);
  memset(base, 0xA5, total);
  // the tables, each in a heap block of exactly its size
  std::vector<int32_t> xfirst(W), xcount(W), yfirst(H), ycount(H);
  std::vector<float> xw((size_t)C + 2 * W), yw((size_t)R + 2 * H);
  int whole = 0;
  float scale = 0.f;
  rip::build_resize_area_tables(R, C, H, W, xfirst.data(), xcount.data(), xw.data(), yfirst.data(), ycount.data(), yw.data(), &whole, &scale);
  int32_t* xwofs = (int32_t*)malloc((size_t)W * 4);
  int32_t* ywofs = (int32_t*)malloc((size_t)H * 4);
  int32_t nx = 0, ny = 0;
  for (int i = 0; i < W; i++) { xwofs[i] = nx; nx += xcount[i]; }
  for (int i = 0; i < H; i++) { ywofs[i] = ny; ny += ycount[i]; }
  float* xweight = (float*)malloc((size_t)nx * 4);
  float* yweight = (float*)malloc((size_t)ny * 4);
  memcpy(xweight, xw.data(), (size_t)nx * 4);
  memcpy(yweight, yw.data(), (size_t)ny * 4);
  rip::AreaParams p = {};
  p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
  p.dst = base + dst_off; p.dst_step = dstep; p.dst_frame_stride = dframe;
  p.src_rows = R; p.src_cols = C; p.rows = H; p.cols = W; p.channels = cn; p.n_frames = n;
  p.whole = whole; p.scale = scale;
  p.xfirst = xfirst.data(); p.xcount = xcount.data(); p.xwofs = xwofs; p.xweight = xweight;
  p.yfirst = yfirst.data(); p.ycount = ycount.data(); p.ywofs = ywofs; p.yweight = yweight;
  rip::LaunchInfo info = {};
  if (!rip::launch_area_reduce(p, nullptr, &info)) { printf("refused %d x %d -> %d x %d\n", C, R, W, H); return 1; }
  const char* expect = cn == 1 ? (whole ? "area_reduce_kernel<1, true>" : "area_reduce_kernel<1, false>")
                               : (whole ? "area_reduce_kernel<3, true>" : "area_reduce_kernel<3, false>");
  if (strcmp(info.kernel, expect) != 0 || info.grid_x != (unsigned)((W + rip::kAreaTileCols - 1) / rip::kAreaTileCols) ||
      info.grid_y != (unsigned)((H + rip::kAreaTileRows - 1) / rip::kAreaTileRows)) { printf("launch record %s %u %u\n", info.kernel, info.grid_x, info.grid_y); return 1; }
  if (fwrite(base, 1, total, out) != total) return 1;
  free(src); free(base); free(xwofs); free(ywofs); free(xweight); free(yweight);
  return 0;
}

// what the launch function must refuse without launching
static int refusals() {
  static uint32_t buf[64];
  rip::AreaParams p = {};
  p.src = (const uint8_t*)buf; p.src_step = 16; p.src_frame_stride = 64;
  p.dst = (uint8_t*)buf + 128; p.dst_step = 6; p.dst_frame_stride = 12;
  p.src_rows = 4; p.src_cols = 4; p.rows = 2; p.cols = 1; p.channels = 3; p.n_frames = 1; p.whole = 1; p.scale = 0.125f;
  int bad = 0;
  auto refused = [&](rip::AreaParams q, const char* what) {
    gridDim = dim3(0, 0, 0);
    if (rip::launch_area_reduce(q, nullptr, nullptr) || gridDim.x != 0) { printf("accepted: %s\n", what); bad++; }
  };
  if (!rip::launch_area_reduce(p, nullptr, nullptr)) { printf("the valid launch was refused\n"); bad++; }
  { auto q = p; q.cols = 5; refused(q, "an upscale"); }
  { auto q = p; q.rows = 4; q.cols = 4; refused(q, "the identity"); }
  { auto q = p; q.rows = 2; q.cols = 2; refused(q, "the 2 x 2 case"); }
  { auto q = p; q.whole = 0; refused(q, "a whole flag that does not match"); }
  { auto q = p; q.cols = 3; q.whole = 0; refused(q, "missing tables"); }
  { auto q = p; q.channels = 2; refused(q, "two channels"); }
  { auto q = p; q.src_step = 15; refused(q, "an unaligned source pitch"); }
  { auto q = p; q.src = (const uint8_t*)buf + 1; refused(q, "an unaligned source"); }
  { auto q = p; q.src_step = 8; refused(q, "a source pitch smaller than a row"); }
  { auto q = p; q.dst_step = 2; refused(q, "a destination pitch smaller than a row"); }
  { auto q = p; q.src_rows = 16385; refused(q, "a side above 16384"); }
  { auto q = p; q.src_rows = 514; q.src_frame_stride = 16 * 514; refused(q, "a factor above 256"); }
  { auto q = p; q.n_frames = 0; refused(q, "no frame"); }
  { auto q = p; q.dst = nullptr; refused(q, "a null destination"); }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t count = 0;
  if (fread(&count, 4, 1, in) != 1) return 2;
  int bad = refusals();
  for (int i = 0; i < count; i++)
    if (run(in, out)) { printf("case %d failed\n", i); bad++; break; }
  fclose(out);
  printf("area kernel on the host: %d cases, %d bad\n", count, bad);
  return bad ? 1 : 0;
}
