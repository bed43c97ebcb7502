// The kernels of csrc/rip_aa.hip executed on the host (hip_host_stub_lds): launch_aa checks and records the launch, then every
// workgroup of the recorded grid gets a heap block of exactly the launch's LDS size and runs aa_phase1 for its 256 threads, then
// aa_phase2 -- the kernel's two phases around its barrier.  Frames sit in an exactly sized staging image, tables in heap blocks of
// exactly their sizes, destinations in exactly sized buffers filled with a sentinel.  The cases come from a file
// tests/test_resize_aa.py writes; every byte of every destination buffer goes to a second file, which the test compares with
// tests/aa_reference.py.  Built with clang++; with -fsanitize=address,undefined it also proves that no access leaves a buffer.
// usage: aa_kernel_host <cases.bin> <out.bin>
//   cases.bin: int32 count, then per case 15 x int32 (filter 2 | 3, R, C of F, window x, y, w, h, H, W of F', channels, frames, dst
//   row padding, dst offset, frame gap, tile height to force or 0 for the host's choice) and the frames' R * C * channels tight
//   bytes each.  out.bin: per case the destination buffer, 0xA5 where nothing was written.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
host_stub::Launch host_stub::last_launch;
void* host_stub::block_lds;
#include "rip_aa.hip"
#include <cstdio>
#include <cstring>
#include <vector>
#include "rip_host.hpp"

template <int CH, bool WIN>
static void run_blocks(const rip::AaParams& p, const rip::FitWindow& w) {
  const host_stub::Launch l = host_stub::last_launch;
  gridDim = l.grid;
  blockDim = l.block;
  for (unsigned z = 0; z < l.grid.z; z++)
    for (unsigned y = 0; y < l.grid.y; y++)
      for (unsigned x = 0; x < l.grid.x; x++) {
        blockIdx = dim3(x, y, z);
        uint8_t* lds = (uint8_t*)malloc(l.shmem);
        memset(lds, 0xEE, l.shmem);
        host_stub::block_lds = lds;
        for (unsigned t = 0; t < l.block.x; t++) {
          threadIdx = dim3(t, 0, 0);
          rip::aa_phase1<CH, WIN>(p, w, lds);
        }
        for (unsigned t = 0; t < l.block.x; t++) {
          threadIdx = dim3(t, 0, 0);
          rip::aa_phase2<CH, WIN>(p, w, lds);
        }
        host_stub::block_lds = nullptr;
        free(lds);
      }
}

template <typename T>
static T* exact_copy(const T* from, size_t n) {
  T* q = (T*)malloc(n ? n * sizeof(T) : 1);
  memcpy(q, from, n * sizeof(T));
  return q;
}

static int run(FILE* in, FILE* out) {
  int32_t h[15];
  if (fread(h, 4, 15, in) != 15) return 1;
  const int filter = h[0], R = h[1], C = h[2], wx = h[3], wy = h[4], ww = h[5], wh = h[6], H = h[7], W = h[8], cn = h[9], n = h[10];
  const size_t dst_pad = h[11], dst_off = h[12], gap = h[13];
  const int force_th = h[14];
  const size_t sstep = ((size_t)C * cn + 15) & ~(size_t)15, sframe = sstep * R;
  uint8_t* src = (uint8_t*)aligned_alloc(16, sframe * n);  // exactly the staging image
  memset(src, 0x5A, sframe * n);
  for (int f = 0; f < n; f++)
    for (int y = 0; y < R; y++)
      if (fread(src + f * sframe + y * sstep, 1, (size_t)C * cn, in) != (size_t)C * cn) return 1;
  const size_t dstep = (size_t)W * cn + dst_pad, dframe = dstep * H + gap;
  const size_t total = dst_off + dframe * (n - 1) + dstep * (H - 1) + (size_t)W * cn;  // ends with the last delivered byte
  uint8_t* base = (uint8_t*)malloc(total);
  memset(base, 0xA5, total);
  // the tables of the window's size, each in a heap block of exactly its size
  std::vector<int32_t> xf(W), xc(W), xo(W), yf(H), yc(H), yo(H);
  std::vector<int16_t> xw(rip::resize_aa_weight_capacity(filter, ww, W)), yw(rip::resize_aa_weight_capacity(filter, wh, H));
  int xprec = 0, yprec = 0, th[2], lr[2];
  rip::build_resize_aa_tables(filter, wh, ww, H, W, xf.data(), xc.data(), xo.data(), xw.data(), &xprec, yf.data(), yc.data(), yo.data(), yw.data(), &yprec, th, lr);
  rip::AaParams p = {};
  p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
  p.dst = base + dst_off; p.dst_step = dstep; p.dst_frame_stride = dframe;
  p.src_rows = wh; p.src_cols = ww; p.rows = H; p.cols = W; p.channels = cn; p.n_frames = n;
  p.tile_rows = force_th ? force_th : th[cn == 3];
  p.lds_rows = force_th ? rip::aa_lds_rows(wh, H, yf.data(), yc.data(), force_th) : lr[cn == 3];
  p.xprec = xprec; p.yprec = yprec;
  p.xfirst = exact_copy(xf.data(), W); p.xcount = exact_copy(xc.data(), W); p.xwofs = exact_copy(xo.data(), W);
  p.yfirst = exact_copy(yf.data(), H); p.ycount = exact_copy(yc.data(), H); p.ywofs = exact_copy(yo.data(), H);
  p.xweight = exact_copy(xw.data(), (size_t)xo[W - 1] + xc[W - 1]);
  p.yweight = exact_copy(yw.data(), (size_t)yo[H - 1] + yc[H - 1]);
  const rip::FitWindow w = {wx, wy, C, R};
  const bool win = wx != 0 || wy != 0 || ww != C || wh != R;
  rip::LaunchInfo info = {};
  host_stub::last_launch.count = 0;
  if (!rip::launch_aa(p, w, nullptr, &info) || host_stub::last_launch.count != 1) { printf("refused %d x %d -> %d x %d\n", ww, wh, W, H); return 1; }
  char expect[64];
  snprintf(expect, sizeof(expect), "aa_kernel<%d, %s>", cn, win ? "true" : "false");
  const host_stub::Launch& l = host_stub::last_launch;
  if (strcmp(info.kernel, expect) != 0 || l.grid.x != (unsigned)((W + 63) / 64) || l.grid.y != (unsigned)((H + p.tile_rows - 1) / p.tile_rows) ||
      l.grid.z != (unsigned)n || l.block.x != 256 || l.shmem != (size_t)p.lds_rows * 64 * cn || l.shmem > 65536 || info.grid_x != l.grid.x || info.grid_y != l.grid.y) {
    printf("launch record %s %u %u %u lds %zu\n", info.kernel, l.grid.x, l.grid.y, l.grid.z, l.shmem);
    return 1;
  }
  if (cn == 1) win ? run_blocks<1, true>(p, w) : run_blocks<1, false>(p, w);
  else win ? run_blocks<3, true>(p, w) : run_blocks<3, false>(p, w);
  if (fwrite(base, 1, total, out) != total) return 1;
  for (const void* q : {(const void*)p.xfirst, (const void*)p.xcount, (const void*)p.xwofs, (const void*)p.yfirst, (const void*)p.ycount, (const void*)p.ywofs,
                        (const void*)p.xweight, (const void*)p.yweight, (const void*)src, (const void*)base})
    free(const_cast<void*>(q));
  return 0;
}

// what the launch function must refuse without launching
static int refusals() {
  static uint32_t buf[4096];
  static int32_t tab[64];
  static int16_t wts[64];
  rip::AaParams p = {};
  p.src = (const uint8_t*)buf; p.src_step = 16; p.src_frame_stride = 64;
  p.dst = (uint8_t*)buf + 8192; p.dst_step = 6; p.dst_frame_stride = 12;
  p.src_rows = 4; p.src_cols = 4; p.rows = 2; p.cols = 2; p.channels = 3; p.n_frames = 1;
  p.tile_rows = 8; p.lds_rows = 4; p.xprec = 14; p.yprec = 14;
  p.xfirst = p.xcount = p.xwofs = p.yfirst = p.ycount = p.ywofs = tab;
  p.xweight = p.yweight = wts;
  const rip::FitWindow whole = {0, 0, 4, 4};
  int bad = 0;
  auto refused = [&](rip::AaParams q, rip::FitWindow w, const char* what) {
    host_stub::last_launch.count = 0;
    if (rip::launch_aa(q, w, nullptr, nullptr) || host_stub::last_launch.count != 0) { printf("accepted: %s\n", what); bad++; }
  };
  host_stub::last_launch.count = 0;
  if (!rip::launch_aa(p, whole, nullptr, nullptr) || host_stub::last_launch.count != 1) { printf("the valid launch was refused\n"); bad++; }
  { auto q = p; q.rows = 4; q.cols = 4; refused(q, whole, "the identity"); }
  { auto q = p; q.src_rows = 130; q.src_frame_stride = 16 * 130; rip::FitWindow w = {0, 0, 4, 130}; refused(q, w, "a factor above 64"); }
  { auto q = p; q.tile_rows = 3; refused(q, whole, "a tile height of 3"); }
  { auto q = p; q.tile_rows = 16; refused(q, whole, "a tile height of 16"); }
  { auto q = p; q.lds_rows = 0; refused(q, whole, "no LDS row"); }
  { auto q = p; q.lds_rows = 342; refused(q, whole, "more LDS than 64 KiB"); }
  { auto q = p; q.xprec = 23; refused(q, whole, "a precision above 22"); }
  { auto q = p; q.yweight = nullptr; refused(q, whole, "a missing table"); }
  { auto q = p; q.xfirst = (const int32_t*)((const uint8_t*)tab + 2); refused(q, whole, "a misaligned table"); }
  { auto q = p; q.channels = 2; refused(q, whole, "two channels"); }
  { auto q = p; q.src_step = 15; refused(q, whole, "an unaligned source pitch"); }
  { auto q = p; q.src = (const uint8_t*)buf + 1; refused(q, whole, "an unaligned source"); }
  { auto q = p; q.src_step = 8; refused(q, whole, "a source pitch smaller than a row"); }
  { auto q = p; q.dst_step = 5; refused(q, whole, "a destination pitch smaller than a row"); }
  { auto q = p; q.src_rows = 16385; refused(q, whole, "a side above 16384"); }
  { auto q = p; q.n_frames = 0; refused(q, whole, "no frame"); }
  { auto q = p; q.dst = nullptr; refused(q, whole, "a null destination"); }
  { rip::FitWindow w = {1, 0, 4, 4}; refused(p, w, "a window that leaves F on the right"); }
  { rip::FitWindow w = {0, 1, 4, 4}; refused(p, w, "a window that leaves F at the bottom"); }
  { rip::FitWindow w = {-1, 0, 8, 8}; refused(p, w, "a negative origin"); }
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
  printf("aa kernel on the host: %d cases, %d bad\n", count, bad);
  return bad ? 1 : 0;
}
