// A stand-in for <hip/hip_runtime.h> for kernels with dynamic shared memory and one barrier between two phases
// (tests/cpp/aa_kernel_host.cpp).  A launch is recorded, not run: the harness then walks the recorded grid itself and, per workgroup,
// runs the first phase for every thread, then the second -- which is what the barrier between them means.  The workgroup's
// __shared__ storage is a heap block of exactly the launch's size (host_stub::block_lds), allocated per workgroup by the harness, so
// that a sanitizer sees every access that leaves it.  Calling a kernel's own entry point is a mistake: __syncthreads() aborts.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
extern dim3 blockIdx, threadIdx, gridDim, blockDim;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
typedef struct ihipStream_t* hipStream_t;
using std::max;
using std::min;

namespace host_stub {
struct Launch {
  dim3 grid, block;
  size_t shmem;
  int count;  // launches recorded since the harness cleared it
};
extern Launch last_launch;
extern void* block_lds;  // the running workgroup's shared memory: exactly last_launch.shmem bytes
inline void record(dim3 grid, dim3 block, size_t shmem) {
  last_launch.grid = grid;
  last_launch.block = block;
  last_launch.shmem = shmem;
  last_launch.count++;
}
}  // namespace host_stub

#define HIP_DYNAMIC_SHARED(type, var) type* var = static_cast<type*>(host_stub::block_lds);
inline void __syncthreads() { abort(); }
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) host_stub::record(grid, block, shmem)
