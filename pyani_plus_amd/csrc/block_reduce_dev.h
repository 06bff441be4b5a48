// block_reduce_dev.h -- the reduction of one value per lane over a workgroup by halving in LDS: a fixed tree, so a sum
// of doubles has the same bits run to run (pa_moments_f64 and pa_kde_gauss_f64 promise that).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pa_dev {

// op over the THREADS (a power of two) values `x` of the workgroup, to every lane.  Steps THREADS / 2, ..., 1; in each,
// lane t < step does s[t] = op(s[t], s[t + step]).  `s` holds THREADS elements and is free again on return.
template <int THREADS, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T x, T *s, Op op) {
  static_assert(THREADS > 0 && (THREADS & (THREADS - 1)) == 0, "the tree halves");
  s[threadIdx.x] = x;
  __syncthreads();
  for (uint32_t step = THREADS / 2; step > 0; step >>= 1) {
    if (threadIdx.x < step) {
      const T other = s[threadIdx.x + step];
      s[threadIdx.x] = op(s[threadIdx.x], other);
    }
    __syncthreads();
  }
  const T total = s[0];
  __syncthreads();
  return total;
}

}  // namespace pa_dev
