// yuv420_kernel<true / false> of csrc/rip_yuv.hip executed on the host, thread by thread over the launcher's own grid (hip_host_stub).
// The source of a case is a heap block of exactly src_pitch x (rows - 1) bytes plus the last row's dwords; the destination is a heap
// block of `total` bytes that ends with the last byte the layout holds and starts `dst_off` bytes into a 16-byte aligned allocation,
// 0xA5 everywhere beforehand.  The whole block goes to the output file: the test compares it with tests/yuv_reference.py laid out at
// the same pitch, sentinels included.  Built with clang++, -I hip_host_stub in front of the ROCm headers; with
// -fsanitize=address,undefined it also proves that no access leaves a buffer and that no wide access is misaligned.
// usage: yuv_kernel_host cases.bin out.bin
//   cases.bin: int32 n, then per case int32 {rows, cols, semi_planar, src_pitch, dst_pitch, dst_off, total, frames}, int32[10] the
//   matrix (y, cb, cr weights of B G R, yoff) and the source bytes
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_yuv.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>

// what launch_yuv420 must refuse without launching
static int refusals() {
  alignas(16) static uint8_t src[256];
  alignas(16) static uint8_t out[256];
  rip::Yuv420Params p = {};
  p.src = src; p.src_step = 12; p.src_frame_stride = 24; p.dst = out; p.dst_step = 4; p.dst_frame_stride = 12;
  p.rows = 2; p.cols = 4; p.n_frames = 1; p.semi_planar = 1;
  int bad = 0;
  if (!rip::launch_yuv420(p, nullptr, nullptr)) { printf("the valid launch was refused\n"); bad++; }
  auto refused = [&](rip::Yuv420Params q, const char* what) {
    if (rip::launch_yuv420(q, nullptr, nullptr)) { printf("accepted: %s\n", what); bad++; }
  };
  { auto q = p; q.src = nullptr; refused(q, "a null source"); }
  { auto q = p; q.dst = nullptr; refused(q, "a null destination"); }
  { auto q = p; q.src = src + 2; refused(q, "a source that is not 4-byte aligned"); }
  { auto q = p; q.src_step = 14; refused(q, "a source pitch that is no multiple of 4"); }
  { auto q = p; q.src_step = 8; refused(q, "a source pitch smaller than a row"); }
  { auto q = p; q.rows = 3; refused(q, "an odd height"); }
  { auto q = p; q.cols = 3; refused(q, "an odd width"); }
  { auto q = p; q.rows = 0; refused(q, "no row"); }
  { auto q = p; q.dst_step = 3; refused(q, "a destination pitch smaller than a row"); }
  { auto q = p; q.semi_planar = 0; q.dst_step = 5; refused(q, "an odd pitch under i420"); }
  { auto q = p; q.n_frames = 0; refused(q, "no frame"); }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: yuv_kernel_host cases.bin out.bin\n"); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* outf = fopen(argv[2], "wb");
  if (!in || !outf) { printf("cannot open the files\n"); return 2; }
  int n = 0, bad = refusals();
  if (fread(&n, 4, 1, in) != 1) return 2;
  for (int i = 0; i < n; i++) {
    int h[8], m[10];
    if (fread(h, 4, 8, in) != 8 || fread(m, 4, 10, in) != 10) return 2;
    const int rows = h[0], cols = h[1], semi = h[2], frames = h[7];
    const size_t src_pitch = (size_t)h[3], dst_pitch = (size_t)h[4], dst_off = (size_t)h[5], total = (size_t)h[6];
    const size_t src_frame = src_pitch * (size_t)rows;
    const size_t src_bytes = src_frame * (size_t)(frames - 1) + src_pitch * (size_t)(rows - 1) + (((size_t)cols * 3 + 3) & ~(size_t)3);
    void* sblock = nullptr;  // exactly the bytes the rule makes readable: the source ends where the block ends
    if (posix_memalign(&sblock, 16, src_bytes) != 0) return 2;
    if (fread(sblock, 1, src_bytes, in) != src_bytes) return 2;
    void* dblock = nullptr;
    if (posix_memalign(&dblock, 16, dst_off + total) != 0) return 2;
    memset(dblock, 0xA5, dst_off + total);
    rip::Yuv420Params p = {};
    p.src = (const uint8_t*)sblock; p.src_step = src_pitch; p.src_frame_stride = src_frame;
    p.dst = (uint8_t*)dblock + dst_off; p.dst_step = dst_pitch; p.dst_frame_stride = dst_pitch * (size_t)(rows / 2 * 3) + 5;  // an odd gap between frames
    p.rows = rows; p.cols = cols; p.n_frames = frames; p.semi_planar = semi;
    for (int k = 0; k < 3; k++) p.m.y[k] = m[k], p.m.cb[k] = m[3 + k], p.m.cr[k] = m[6 + k];
    p.m.yoff = m[9];
    rip::LaunchInfo info = {};
    const unsigned groups = (unsigned)((rows / 2 + rip::kYuvPairsPerBlock - 1) / rip::kYuvPairsPerBlock);
    if (!rip::launch_yuv420(p, nullptr, &info)) { printf("case %d refused\n", i); bad++; }
    else if (strcmp(info.kernel, semi ? "yuv420_kernel<true>" : "yuv420_kernel<false>") != 0 ||
             info.grid_x != (unsigned)((cols + rip::kYuvPxPerBlockX - 1) / rip::kYuvPxPerBlockX) || info.grid_y != groups || info.block != 256) {
      printf("case %d: launch record %s %u %u %u\n", i, info.kernel, info.grid_x, info.grid_y, info.block);
      bad++;
    }
    fwrite(dblock, 1, dst_off + total, outf);
    free(sblock);
    free(dblock);
  }
  fclose(in);
  fclose(outf);
  printf("yuv420 kernels on the host: %d cases, %d bad\n", n, bad);
  return bad ? 1 : 0;
}
