// A stand-in for <hip/hip_runtime.h> that runs a HIP kernel on the host, one thread after another over the launcher's own grid
// (tests/cpp/resize_kernel_host.cpp).  Enough for kernels without __syncthreads, shared memory or cross-lane operations.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
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

template <typename F>
void host_launch(dim3 grid, dim3 block, F&& f) {
  gridDim = grid;
  blockDim = block;
  for (unsigned z = 0; z < grid.z; z++)
    for (unsigned y = 0; y < grid.y; y++)
      for (unsigned x = 0; x < grid.x; x++)
        for (unsigned t = 0; t < block.x; t++) {
          blockIdx = dim3(x, y, z);
          threadIdx = dim3(t, 0, 0);
          f();
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) host_launch(grid, block, [&] { kernel(__VA_ARGS__); })
