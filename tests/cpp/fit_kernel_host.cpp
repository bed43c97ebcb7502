// The kernels of csrc/rip_fit.hip executed on the host, thread by thread over the launcher's own grid (hip_host_stub): a window of an
// exactly sized staging image F is resized into a rectangle of an exactly sized destination, and the pad kernel fills the rest.
// Tables are those of the window's size, in heap blocks of exactly their size, laid out as rip_batch.cpp lays them out.  The cases
// and their frames come from a file tests/test_fit.py writes; every byte of every destination buffer -- picture, bands, row padding,
// frame gaps -- goes to a second file, which the test compares with tests/fit_reference.py.  Built with clang++, -I hip_host_stub in
// front of the ROCm headers; with -fsanitize=address,undefined it also proves that no access leaves a buffer.
// usage: fit_kernel_host <cases.bin> <out.bin>
//   cases.bin: int32 count, then per case 21 x int32 (R, C, channels, frames, window x, y, w, h, picture w, h, area, delivered W, H,
//   picture left, top, dst row padding, dst offset, frame gap, pad bytes 0 .. 2) and the frames' R * C * channels tight bytes each.
//   out.bin: per case the destination buffer, 0xA5 where nothing was written.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_fit.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rip_host.hpp"

static int run(FILE* in, FILE* out) {
  int32_t h[21];
  if (fread(h, 4, 21, in) != 21) return 1;
  const int R = h[0], C = h[1], cn = h[2], n = h[3], xs = h[4], ys = h[5], ws = h[6], hs = h[7], Wi = h[8], Hi = h[9], area = h[10];
  const int W = h[11], H = h[12], left = h[13], top = h[14];
  const size_t dst_pad = h[15], dst_off = h[16], gap = h[17];
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
  uint8_t* pic = base + dst_off + (size_t)top * dstep + (size_t)left * cn;
  const rip::FitWindow win = {xs, ys, C, R};
  rip::LaunchInfo info = {};
  const bool same = ws == Wi && hs == Hi, mean2 = ws == 2 * Wi && hs == 2 * Hi;
  char expect[64];
  if (area && !same && !mean2) {
    std::vector<int32_t> xfirst(Wi), xcount(Wi), yfirst(Hi), ycount(Hi);
    std::vector<float> xw((size_t)ws + 2 * Wi), yw((size_t)hs + 2 * Hi);
    int whole = 0;
    float scale = 0.f;
    rip::build_resize_area_tables(hs, ws, Hi, Wi, xfirst.data(), xcount.data(), xw.data(), yfirst.data(), ycount.data(), yw.data(), &whole, &scale);
    int32_t* xwofs = (int32_t*)malloc((size_t)Wi * 4);
    int32_t* ywofs = (int32_t*)malloc((size_t)Hi * 4);
    int32_t nx = 0, ny = 0;
    for (int i = 0; i < Wi; i++) { xwofs[i] = nx; nx += xcount[i]; }
    for (int i = 0; i < Hi; i++) { ywofs[i] = ny; ny += ycount[i]; }
    float* xweight = (float*)malloc((size_t)nx * 4);
    float* yweight = (float*)malloc((size_t)ny * 4);
    memcpy(xweight, xw.data(), (size_t)nx * 4);
    memcpy(yweight, yw.data(), (size_t)ny * 4);
    rip::AreaParams p = {};
    p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
    p.dst = pic; p.dst_step = dstep; p.dst_frame_stride = dframe;
    p.src_rows = hs; p.src_cols = ws; p.rows = Hi; p.cols = Wi; p.channels = cn; p.n_frames = n;
    p.whole = whole; p.scale = scale;
    p.xfirst = xfirst.data(); p.xcount = xcount.data(); p.xwofs = xwofs; p.xweight = xweight;
    p.yfirst = yfirst.data(); p.ycount = ycount.data(); p.ywofs = ywofs; p.yweight = yweight;
    if (!rip::launch_fit_area(p, win, nullptr, &info)) { printf("area refused\n"); return 1; }
    snprintf(expect, sizeof expect, "fit_area_kernel<%d, %s>", cn, whole ? "true" : "false");
    free(xwofs); free(ywofs); free(xweight); free(yweight);
  } else {
    const size_t wp = rip::resize_table_cols(Wi);
    int32_t* xofs = (int32_t*)aligned_alloc(16, wp * 4);
    int16_t* alpha = (int16_t*)aligned_alloc(16, wp * 4);
    int32_t* yofs = (int32_t*)malloc((size_t)Hi * 8);
    int16_t* beta = (int16_t*)malloc((size_t)Hi * 4);
    memset(xofs, 0, wp * 4);
    memset(alpha, 0, wp * 4);
    int area2 = 0;
    rip::build_resize_tables(hs, ws, Hi, Wi, xofs, alpha, yofs, beta, &area2);
    rip::ResizeParams p = {};
    p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
    p.dst = pic; p.dst_step = dstep; p.dst_frame_stride = dframe;
    p.src_rows = hs; p.src_cols = ws; p.rows = Hi; p.cols = Wi; p.channels = cn; p.n_frames = n;
    p.area2 = area2;
    if (!area2) { p.xofs = xofs; p.alpha = alpha; p.yofs = yofs; p.beta = beta; }  // the mean reads no table
    if (!rip::launch_fit_resize(p, win, nullptr, &info)) { printf("resize refused\n"); return 1; }
    snprintf(expect, sizeof expect, area2 ? "fit_mean2_kernel<%d>" : "fit_linear_kernel<%d>", cn);
    free(xofs); free(alpha); free(yofs); free(beta);
  }
  if (strcmp(info.kernel, expect) != 0) { printf("launch record %s, expected %s\n", info.kernel, expect); return 1; }
  rip::FitPadParams f = {};
  f.dst = base + dst_off; f.dst_step = dstep; f.dst_frame_stride = dframe;
  f.rows = H; f.cols = W; f.pic_x = left; f.pic_y = top; f.pic_w = Wi; f.pic_h = Hi; f.channels = cn; f.n_frames = n;
  for (int i = 0; i < 3; i++) f.color[i] = (uint8_t)h[18 + i];
  gridDim = dim3(0, 0, 0);
  const bool padded = rip::launch_fit_pad(f, nullptr, &info);
  if (padded != (Wi != W || Hi != H) || (!padded && gridDim.x != 0)) { printf("pad launched: %d\n", (int)padded); return 1; }
  if (fwrite(base, 1, total, out) != total) return 1;
  free(src); free(base);
  return 0;
}

// what the launch functions must refuse without launching
static int refusals() {
  static uint32_t buf[256];
  static int32_t tab[64] __attribute__((aligned(16)));
  rip::ResizeParams p = {};
  p.src = (const uint8_t*)buf; p.src_step = 16; p.src_frame_stride = 64;
  p.dst = (uint8_t*)buf + 512; p.dst_step = 6; p.dst_frame_stride = 12;
  p.src_rows = 3; p.src_cols = 3; p.rows = 2; p.cols = 2; p.channels = 3; p.n_frames = 1;
  p.xofs = tab; p.alpha = (const int16_t*)(tab + 4); p.yofs = tab + 8; p.beta = (const int16_t*)(tab + 12);
  const rip::FitWindow w = {1, 1, 4, 4};
  int bad = 0;
  auto refused = [&](rip::ResizeParams q, rip::FitWindow v, const char* what) {
    gridDim = dim3(0, 0, 0);
    if (rip::launch_fit_resize(q, v, nullptr, nullptr) || gridDim.x != 0) { printf("accepted: %s\n", what); bad++; }
  };
  if (!rip::launch_fit_resize(p, w, nullptr, nullptr)) { printf("the valid launch was refused\n"); bad++; }
  { auto v = w; v.x = 2; refused(p, v, "a window beyond the last column"); }
  { auto v = w; v.y = 2; refused(p, v, "a window beyond the last row"); }
  { auto v = w; v.x = -1; refused(p, v, "a negative origin"); }
  { auto v = w; v.frame_cols = 6; refused(p, v, "a source pitch smaller than a row of F"); }
  { auto v = w; v.frame_rows = 5; refused(p, v, "a frame stride smaller than F"); }
  { auto q = p; q.area2 = 1; refused(q, w, "a mean flag that does not match"); }
  { auto q = p; q.xofs = nullptr; refused(q, w, "a missing table"); }
  { auto q = p; q.channels = 2; refused(q, w, "two channels"); }
  { auto q = p; q.src = (const uint8_t*)buf + 1; refused(q, w, "an unaligned source"); }
  { auto q = p; q.dst_step = 5; refused(q, w, "a destination pitch smaller than a row"); }
  { auto q = p; q.n_frames = 0; refused(q, w, "no frame"); }
  rip::FitPadParams f = {};
  f.dst = (uint8_t*)buf; f.dst_step = 12; f.dst_frame_stride = 48; f.rows = 4; f.cols = 4; f.pic_x = 1; f.pic_y = 0; f.pic_w = 2; f.pic_h = 4;
  f.channels = 3; f.n_frames = 1;
  auto pad_refused = [&](rip::FitPadParams q, const char* what) {
    gridDim = dim3(0, 0, 0);
    if (rip::launch_fit_pad(q, nullptr, nullptr) || gridDim.x != 0) { printf("accepted: %s\n", what); bad++; }
  };
  if (!rip::launch_fit_pad(f, nullptr, nullptr)) { printf("the valid pad launch was refused\n"); bad++; }
  { auto q = f; q.pic_x = 0; q.pic_w = 4; pad_refused(q, "a picture that leaves no band"); }
  { auto q = f; q.pic_x = 3; pad_refused(q, "a picture beyond the last column"); }
  { auto q = f; q.pic_h = 5; pad_refused(q, "a picture beyond the last row"); }
  { auto q = f; q.dst_step = 11; pad_refused(q, "a destination pitch smaller than a row"); }
  { auto q = f; q.channels = 4; pad_refused(q, "four channels"); }
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
  printf("fit kernels on the host: %d cases, %d bad\n", count, bad);
  return bad ? 1 : 0;
}
