// head_copy_kernel of csrc/rip_heads.hip executed on the host, thread by thread over the launcher's own grid (hip_host_stub).  The
// staging image is a heap block of exactly rows x pitch x frames bytes, the pitch being the row rounded up to 16 and no byte more; the
// destination is a heap block that ends with the last delivered byte and starts `offset` bytes into a 16-byte aligned allocation.
// Row lengths 1 .. 70 and 4095 .. 4098 bytes (the workgroup edge), destination offsets 0 .. 17, pitches tight, + 1 and the next
// multiple of 16, 1 and 3 frames.  Every byte of every destination is compared: the rows with the source, everything else with the
// sentinel.  Built with clang++, -I hip_host_stub in front of the ROCm headers; with -fsanitize=address,undefined it also proves
// that no access leaves a buffer and that no wide access is misaligned.
// usage: heads_kernel_host
#include <hip/hip_runtime.h>
dim3 blockIdx, threadIdx, gridDim, blockDim;
#include "rip_heads.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int run(size_t row_bytes, int rows, int n, size_t offset, int pitch_kind) {
  const size_t sstep = (row_bytes + 15) & ~(size_t)15, sframe = sstep * rows;
  uint8_t* src = (uint8_t*)aligned_alloc(16, sframe * n);  // exactly the staging image
  for (size_t i = 0; i < sframe * n; i++) src[i] = (uint8_t)(i * 131u + (i >> 8) * 7u + 1u);
  const size_t dstep = pitch_kind == 0 ? row_bytes : pitch_kind == 1 ? row_bytes + 1 : ((row_bytes + 15) & ~(size_t)15) + 16;
  const size_t gap = pitch_kind == 1 ? 5 : 0, dframe = dstep * rows + gap;
  const size_t total = offset + dframe * (n - 1) + dstep * (rows - 1) + row_bytes;  // ends with the last delivered byte
  void* block = nullptr;  // exactly `total` bytes from a 16-byte aligned address: `offset` is the phase of the first row
  if (posix_memalign(&block, 16, total) != 0) return 1;
  uint8_t* base = (uint8_t*)block;
  memset(base, 0xA5, total);
  rip::HeadCopyParams p = {};
  p.src = src; p.src_step = sstep; p.src_frame_stride = sframe;
  p.dst = base + offset; p.dst_step = dstep; p.dst_frame_stride = dframe;
  p.rows = rows; p.n_frames = n; p.row_bytes = row_bytes;
  rip::LaunchInfo info = {};
  if (!rip::launch_head_copy(p, nullptr, &info)) { printf("refused %zu x %d\n", row_bytes, rows); return 1; }
  if (strcmp(info.kernel, "head_copy_kernel") != 0 || info.grid_x != (unsigned)((row_bytes + 4095) / 4096) || info.grid_y != (unsigned)rows || info.block != 256) {
    printf("launch record %s %u %u %u\n", info.kernel, info.grid_x, info.grid_y, info.block);
    return 1;
  }
  int bad = 0;
  for (size_t i = 0; i < total && !bad; i++) {
    uint8_t want = 0xA5;
    if (i >= offset) {
      const size_t f = (i - offset) / dframe, in_frame = (i - offset) % dframe, y = in_frame / dstep, x = in_frame % dstep;
      if (f < (size_t)n && y < (size_t)rows && x < row_bytes) want = src[f * sframe + y * sstep + x];
    }
    if (base[i] != want) { printf("row bytes %zu rows %d frames %d offset %zu pitch %zu: byte %zu is %u, expected %u\n", row_bytes, rows, n, offset, dstep, i, base[i], want); bad = 1; }
  }
  free(src);
  free(base);
  return bad;
}

// what the launch function must refuse without launching
static int refusals() {
  alignas(16) static uint8_t buf[4096];
  rip::HeadCopyParams p = {};
  p.src = buf; p.src_step = 32; p.src_frame_stride = 64;
  p.dst = buf + 2048; p.dst_step = 20; p.dst_frame_stride = 40;
  p.rows = 2; p.n_frames = 2; p.row_bytes = 20;
  int bad = 0;
  if (!rip::launch_head_copy(p, nullptr, nullptr)) { printf("the valid launch was refused\n"); bad++; }
  auto refused = [&](rip::HeadCopyParams q, const char* what) {
    if (rip::launch_head_copy(q, nullptr, nullptr)) { printf("accepted: %s\n", what); bad++; }
  };
  { auto q = p; q.src = buf + 4; refused(q, "a source that is not 16-byte aligned"); }
  { auto q = p; q.src_step = 24; refused(q, "a source pitch that is no multiple of 16"); }
  { auto q = p; q.src_step = 16; q.src_frame_stride = 32; refused(q, "a source pitch smaller than the padded row"); }
  { auto q = p; q.src_frame_stride = 72; refused(q, "a source frame stride that is no multiple of 16"); }
  { auto q = p; q.src_frame_stride = 48; refused(q, "a source frame stride smaller than a frame"); }
  { auto q = p; q.dst_step = 19; refused(q, "a destination pitch smaller than a row"); }
  { auto q = p; q.dst_frame_stride = 39; refused(q, "a destination frame stride smaller than a frame"); }
  { auto q = p; q.rows = 0; refused(q, "no row"); }
  { auto q = p; q.row_bytes = 0; refused(q, "an empty row"); }
  { auto q = p; q.n_frames = 0; refused(q, "no frame"); }
  { auto q = p; q.n_frames = 65536; refused(q, "more frames than the grid takes"); }
  { auto q = p; q.dst = nullptr; refused(q, "a null destination"); }
  { auto q = p; q.src = nullptr; refused(q, "a null source"); }
  return bad;
}

int main() {
  int bad = refusals(), cases = 0;
  for (int n : {1, 3})
    for (int pitch_kind = 0; pitch_kind < 3; pitch_kind++)
      for (size_t offset = 0; offset < 18; offset++) {
        for (size_t row_bytes = 1; row_bytes <= 70; row_bytes++, cases++) bad += run(row_bytes, 3, n, offset, pitch_kind);
        for (size_t row_bytes = 4095; row_bytes <= 4098; row_bytes++, cases++) bad += run(row_bytes, 2, n, offset, pitch_kind);
      }
  printf("head copy kernel on the host: %d cases, %d bad\n", cases, bad);
  return bad ? 1 : 0;
}
