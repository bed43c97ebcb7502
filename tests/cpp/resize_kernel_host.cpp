// The kernels of csrc/rip_resize.hip executed on the host, thread by thread over the launcher's own grid (hip_host_stub), into
// exactly sized heap buffers and from exactly sized tables: every byte of the destination buffer -- delivered pixels, row padding,
// frame gaps -- is compared with oracle/rip_oracle.c ripo_resize_linear_8u.  Built with clang++ (the vector types of the kernel),
// -I hip_host_stub in front of the ROCm headers; with -fsanitize=address,undefined it also proves that no access leaves a buffer.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_resize.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "rip_host.hpp"
extern "C" void ripo_resize_linear_8u(const uint8_t* src, int rows, int cols, int cn, uint8_t* dst, int drows, int dcols);

static std::mt19937 rng(7);
static long cases = 0;
static int run(int R, int C, int H, int W, int cn, int n, size_t dst_pad, size_t dst_off, size_t gap) {
  const size_t sstep = ((size_t)C * cn + 15) & ~(size_t)15, sframe = sstep * R;
  uint8_t* src = (uint8_t*)aligned_alloc(16, sframe * n);   // exactly the staging image
  for (size_t i = 0; i < sframe * n; i++) src[i] = (uint8_t)rng();
  const size_t dstep = (size_t)W * cn + dst_pad, dframe = dstep * H + gap;
  const size_t total = dst_off + dframe * (n - 1) + dstep * (H - 1) + (size_t)W * cn;  // ends with the last delivered byte
  uint8_t* base = (uint8_t*)aligned_alloc(16, (total + 15) & ~(size_t)15);
  uint8_t* dst = base + dst_off;
  std::vector<uint8_t> guard(base, base + total);
  memset(base, 0xA5, total);
  const size_t wp = rip::resize_table_cols(W);
  int32_t* xofs = (int32_t*)aligned_alloc(16, wp * 4);
  int16_t* alpha = (int16_t*)aligned_alloc(16, wp * 4);
  memset(xofs, 0, wp * 4); memset(alpha, 0, wp * 4);
  int32_t* yofs = (int32_t*)malloc((size_t)H * 8);
  int16_t* beta = (int16_t*)malloc((size_t)H * 4);
  int area = 0;
  rip::build_resize_tables(R, C, H, W, xofs, alpha, yofs, beta, &area);
  rip::ResizeParams p = {};
  p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
  p.dst = dst; p.dst_step = dstep; p.dst_frame_stride = dframe;
  p.src_rows = R; p.src_cols = C; p.rows = H; p.cols = W; p.channels = cn; p.n_frames = n; p.area2 = area;
  p.xofs = xofs; p.alpha = alpha; p.yofs = yofs; p.beta = beta;
  rip::LaunchInfo info;
  if (!rip::launch_resize(p, nullptr, &info)) { printf("refused %d %d %d %d\n", R, C, H, W); return 1; }
  // expectation: every byte of the buffer
  std::vector<uint8_t> want(total, 0xA5), tight((size_t)R * C * cn), out((size_t)H * W * cn);
  for (int f = 0; f < n; f++) {
    for (int y = 0; y < R; y++) memcpy(&tight[(size_t)y * C * cn], src + f * sframe + y * sstep, (size_t)C * cn);
    ripo_resize_linear_8u(tight.data(), R, C, cn, out.data(), H, W);
    for (int y = 0; y < H; y++) memcpy(&want[dst_off + f * dframe + y * dstep], &out[(size_t)y * W * cn], (size_t)W * cn);
  }
  int bad = memcmp(want.data(), base, total) != 0;
  if (bad) printf("MISMATCH %dx%dx%d -> %dx%d n=%d pad=%zu off=%zu gap=%zu kernel %s\n", C, R, cn, W, H, n, dst_pad, dst_off, gap, info.kernel);
  free(src); free(base); free(xofs); free(alpha); free(yofs); free(beta);
  cases++;
  return bad;
}

int main() {
  int bad = 0;
  const int widths[] = {1, 3, 4, 5, 7, 8, 1021, 1024, 1025, 1027};
  for (int cn : {1, 3})
    for (int w : widths) {
      const int sw = std::max(3, (w * 17 + 5) / 10);
      for (size_t pad : {(size_t)0, (size_t)1, (size_t)16})
        for (size_t off : {(size_t)0, (size_t)1}) {
          bad += run(9, sw, 5, w, cn, 2, pad, off, off ? 5 : 0);
          bad += run(10, 2 * w, 5, w, cn, 2, pad, off, off ? 5 : 0);   // the 2 x 2 mean
          bad += run(5, std::max(1, w * 6 / 10), 9, w, cn, 2, pad, off, 0);  // upscale
        }
    }
  for (int cn : {1, 3}) {
    bad += run(5, 611, 9, 1027, cn, 3, 0, 0, 0);
    bad += run(23, 1747, 1, 1027, cn, 3, 0, 0, 0);
    bad += run(2 * 5, 2048, 5, 1024, cn, 3, 0, 0, 0);
    bad += run(10, 2050, 5, 1025, cn, 3, 0, 0, 0);
    bad += run(9, 2050, 5, 1025, cn, 3, 0, 0, 0);
    bad += run(1, 1, 3, 5, cn, 1, 0, 0, 0);
    bad += run(3, 16384, 2, 3, cn, 1, 0, 0, 0);
    bad += run(2, 3, 2, 16384, cn, 1, 0, 0, 0);
  }
  std::uniform_int_distribution<int> side(1, 70), fr(1, 5), pd(0, 17), of(0, 3);
  for (int i = 0; i < 3000; i++) {
    int R = side(rng), C = side(rng), H = side(rng), W = side(rng);
    if (i % 7 == 0) { R = 2 * H; C = 2 * W; }
    if (i % 11 == 0) C = 2 * W;
    bad += run(R, C, H, W, (i & 1) ? 3 : 1, fr(rng), (size_t)pd(rng), (size_t)of(rng), (size_t)pd(rng));
  }
  printf("resize kernel on the host: %ld cases, %d bad\n", cases, bad);
  return bad ? 1 : 0;
}
