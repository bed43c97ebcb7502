// The kernels of csrc/rip_clahe.hip executed on the host (hip_host_stub_lds): the launch functions check and record the launches,
// then every workgroup of a recorded grid gets a heap block of exactly the launch's LDS size and runs the kernel's phases, each for
// all 256 threads before the next -- which is what the barriers between them mean.  Frames sit in an exactly sized staging image
// (out of place) or in the destination itself (in place), the tables in a heap block of exactly their size, destinations in exactly
// sized buffers filled with a sentinel.  The cases come from a file tests/test_clahe.py writes; every byte of every destination
// buffer and of every table block goes to a second file, which the test compares with tests/clahe_reference.py.  Built with clang++;
// with -fsanitize=address,undefined it also proves that no access leaves a buffer and no wide access is misaligned.
// usage: clahe_kernel_host <cases.bin> <out.bin>
//   cases.bin: int32 count, then per case 9 x int32 (H, W of the picture, tiles_x, tiles_y, frames, in place 0 | 1, dst row padding,
//   dst offset, frame gap), the clip limit as a float64, and the frames' H * W tight bytes each.
//   out.bin: per case the destination buffer, 0xA5 where nothing was written, then the frames' tables.
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
host_stub::Launch host_stub::last_launch;
void* host_stub::block_lds;
// the stub has no atomic add; the threads of a workgroup run one after another here
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) {
  const uint32_t old = *p;
  *p = old + v;
  return old;
}
#include "rip_clahe.hip"
#include <cstdio>
#include <cstring>

template <typename Body>
static void for_each_block(const char* name, size_t lds_bytes, Body body) {
  const host_stub::Launch l = host_stub::last_launch;
  if (l.shmem != lds_bytes || l.block.x != 256) { printf("%s: launch with %zu bytes of LDS, %u lanes\n", name, l.shmem, l.block.x); exit(1); }
  gridDim = l.grid;
  blockDim = l.block;
  for (unsigned z = 0; z < l.grid.z; z++)
    for (unsigned y = 0; y < l.grid.y; y++)
      for (unsigned x = 0; x < l.grid.x; x++) {
        blockIdx = dim3(x, y, z);
        uint8_t* lds = (uint8_t*)aligned_alloc(16, l.shmem);
        memset(lds, 0xEE, l.shmem);
        host_stub::block_lds = lds;
        body(lds);
        host_stub::block_lds = nullptr;
        free(lds);
      }
}

template <typename Phase>
static void all_threads(Phase phase) {
  for (unsigned t = 0; t < 256; t++) {
    threadIdx = dim3(t, 0, 0);
    phase();
  }
}

static int run(FILE* in, FILE* out) {
  int32_t h[9];
  double clip = 0;
  if (fread(h, 4, 9, in) != 9 || fread(&clip, 8, 1, in) != 1) return 1;
  const int H = h[0], W = h[1], tx = h[2], ty = h[3], n = h[4], in_place = h[5];
  const size_t dst_pad = h[6], dst_off = h[7], gap = h[8];
  const size_t dstep = (size_t)W + dst_pad, dframe = dstep * H + gap;
  const size_t total = dst_off + dframe * (n - 1) + dstep * (H - 1) + (size_t)W;  // ends with the last delivered byte
  uint8_t* base = (uint8_t*)malloc(total);
  memset(base, 0xA5, total);
  const size_t sstep = ((size_t)W + 15) & ~(size_t)15, sframe = sstep * H;
  uint8_t* staged = in_place ? nullptr : (uint8_t*)aligned_alloc(16, sframe * n);  // exactly the staging image
  if (staged) memset(staged, 0x5A, sframe * n);
  for (int f = 0; f < n; f++)
    for (int y = 0; y < H; y++) {
      uint8_t* row = in_place ? base + dst_off + f * dframe + y * dstep : staged + f * sframe + y * sstep;
      if (fread(row, 1, (size_t)W, in) != (size_t)W) return 1;
    }
  const size_t lut_bytes = rip::clahe_lut_bytes(tx, ty, n);
  uint8_t* lut = (uint8_t*)malloc(lut_bytes);
  memset(lut, 0xC3, lut_bytes);
  rip::ClaheParams p = {};
  p.src = in_place ? base + dst_off : staged;
  p.src_step = in_place ? dstep : sstep;
  p.src_frame_stride = in_place ? dframe : sframe;
  p.dst = base + dst_off; p.dst_step = dstep; p.dst_frame_stride = dframe;
  p.lut = lut;
  p.rows = H; p.cols = W; p.n_frames = n;
  rip::clahe_constants(H, W, tx, ty, clip, p);
  rip::LaunchInfo info = {};
  host_stub::last_launch.count = 0;
  if (!rip::launch_clahe_lut(p, nullptr, &info) || host_stub::last_launch.count != 1) { printf("the table launch was refused\n"); return 1; }
  const host_stub::Launch& l = host_stub::last_launch;
  if (strcmp(info.kernel, "clahe_lut_kernel") != 0 || l.grid.x != (unsigned)tx || l.grid.y != (unsigned)ty || l.grid.z != (unsigned)n || info.grid_x != l.grid.x || info.grid_y != l.grid.y) {
    printf("launch record %s %u %u %u\n", info.kernel, l.grid.x, l.grid.y, l.grid.z);
    return 1;
  }
  for_each_block("clahe_lut_kernel", 4096, [&](uint8_t* lds) {
    uint32_t* hist = (uint32_t*)lds;
    all_threads([&] { rip::clahe_lut_zero(p, hist); });
    all_threads([&] { rip::clahe_lut_count(p, hist); });
    all_threads([&] { rip::clahe_lut_clip(p, hist); });
    all_threads([&] { rip::clahe_lut_spread(p, hist); });
    all_threads([&] { rip::clahe_lut_store(p, hist); });
  });
  host_stub::last_launch.count = 0;
  if (!rip::launch_clahe_apply(p, nullptr, &info) || host_stub::last_launch.count != 1) { printf("the blend launch was refused\n"); return 1; }
  const int strip_rows = rip::clahe_strip_rows(p);
  if (strcmp(info.kernel, "clahe_apply_kernel") != 0 || l.grid.x != 1 || l.grid.y != (unsigned)((ty + 1) * (p.th / strip_rows + 1)) || l.grid.z != (unsigned)n || l.grid.y > 65535 || l.shmem > 8192) {
    printf("launch record %s %u %u %u\n", info.kernel, l.grid.x, l.grid.y, l.grid.z);
    return 1;
  }
  for_each_block("clahe_apply_kernel", (size_t)2 * tx * 256, [&](uint8_t* lds) {
    all_threads([&] { rip::clahe_apply_stage(p, strip_rows, lds); });
    all_threads([&] { rip::clahe_apply_blend(p, strip_rows, lds); });
  });
  if (fwrite(base, 1, total, out) != total || fwrite(lut, 1, lut_bytes, out) != lut_bytes) return 1;
  free(base);
  free(staged);
  free(lut);
  return 0;
}

// what the launch functions must refuse without launching
static int refusals() {
  static uint32_t buf[1024], tables[4 * 64];
  rip::ClaheParams p = {};
  p.src = (const uint8_t*)buf; p.src_step = 16; p.src_frame_stride = 128;
  p.dst = (uint8_t*)buf + 2048; p.dst_step = 9; p.dst_frame_stride = 72;
  p.lut = (uint8_t*)tables;
  p.rows = 8; p.cols = 9; p.n_frames = 1;
  rip::clahe_constants(8, 9, 2, 2, 3.0, p);
  int bad = 0;
  auto refused = [&](rip::ClaheParams q, const char* what) {
    host_stub::last_launch.count = 0;
    if (rip::launch_clahe_lut(q, nullptr, nullptr) || rip::launch_clahe_apply(q, nullptr, nullptr) || host_stub::last_launch.count != 0) { printf("accepted: %s\n", what); bad++; }
  };
  host_stub::last_launch.count = 0;
  if (!rip::launch_clahe_lut(p, nullptr, nullptr) || !rip::launch_clahe_apply(p, nullptr, nullptr) || host_stub::last_launch.count != 2) { printf("the valid launches were refused\n"); bad++; }
  { auto q = p; q.src = nullptr; refused(q, "a null source"); }
  { auto q = p; q.dst = nullptr; refused(q, "a null destination"); }
  { auto q = p; q.lut = nullptr; refused(q, "no table block"); }
  { auto q = p; q.lut = (uint8_t*)tables + 2; refused(q, "a misaligned table block"); }
  { auto q = p; q.tiles_x = 0; refused(q, "no tile"); }
  { auto q = p; q.tiles_y = 17; refused(q, "17 tiles"); }
  { auto q = p; q.tiles_x = 5; refused(q, "a tile of fewer than two columns"); }
  { auto q = p; q.rows = 3; refused(q, "a tile of fewer than two rows"); }
  { auto q = p; q.tw = 4; refused(q, "a tile width that is not the picture's"); }
  { auto q = p; q.th = 4; refused(q, "a tile height that is not the picture's"); }
  { auto q = p; q.scale = 1.0f; refused(q, "a scale that is not the tile's"); }
  { auto q = p; q.inv_tw = 0.5f; refused(q, "a reciprocal that is not the tile's"); }
  { auto q = p; q.clip = -1; refused(q, "a negative clip"); }
  { auto q = p; q.clip = 26; refused(q, "a clip above the tile's area"); }
  { auto q = p; q.src_step = 8; refused(q, "a source pitch smaller than a row"); }
  { auto q = p; q.dst_step = 8; refused(q, "a destination pitch smaller than a row"); }
  { auto q = p; q.n_frames = 0; refused(q, "no frame"); }
  { auto q = p; q.n_frames = 65536; refused(q, "65536 frames"); }
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
  printf("clahe kernels on the host: %d cases, %d bad\n", count, bad);
  return bad ? 1 : 0;
}
