// pair_tile_dev.h -- the 64 x 64 tile of a run's pairs as classify.hip and derep.hip walk it (gfx950, wave64): one
// workgroup per tile, a wave per row of the tile, a lane per column.
//
// M[a,b] is read from global memory as it lies (a row of the tile is 512 contiguous bytes).  M[b,a] lies in the mirrored
// tile, whose rows are read the same coalesced way into LDS and read back transposed.  The tile is held as [64][65]
// doubles: the transposed read has a lane stride of 65 doubles = 130 words, so the 32 lanes of a ds_read_b64 group touch
// the 64 banks once each (bank = 2 * lane and 2 * lane + 1, mod 64); with a stride of 64 doubles all of them would meet
// on two banks.  Several matrices go through the same 33 KB buffer one after the other.
#pragma once

#include "pair_rule.h"

namespace pair_tile {

constexpr int kTile = 64;
constexpr int kThreads = 256;
constexpr int kRows = kTile / (kThreads / 64);  // rows of the tile per wave
constexpr int kPad = kTile + 1;

// out[k] = the aggregate of the pair (a, b), a = a0 + wave * kRows + k, b = b0 + lane; NaN outside the matrix.  On the
// diagonal tile a >= b happens: with kBothTriangles the two cells change places there (pair_value).  With false, out[k]
// is the pair's value for a < b and undefined for a >= b: for a caller that keeps the pairs a < b alone (classify.hip).
// `tile` is the caller's __shared__ double[kTile][kPad].
template <bool kBothTriangles>
__device__ __forceinline__ void tile_values(const double *__restrict__ m, uint32_t n, uint32_t a0, uint32_t b0, int how, double (*tile)[kPad],
                                            double out[kRows]) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const double nan = __builtin_nan("");
  __syncthreads();  // the previous matrix has been read
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint32_t r = wave * kRows + k;
    const uint32_t bb = b0 + r, aa = a0 + lane;
    tile[r][lane] = (bb < n && aa < n) ? m[(uint64_t)bb * n + aa] : nan;  // M[b0 + r, a0 + lane]
  }
  __syncthreads();
  const uint32_t b = b0 + lane;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint32_t r = wave * kRows + k;
    const uint32_t a = a0 + r;
    const double m_ba = tile[lane][r];
    const double m_ab = (a < n && b < n) ? m[(uint64_t)a * n + b] : nan;
    out[k] = kBothTriangles ? pair_rule::pair_value(how, a, b, m_ab, m_ba) : pair_rule::agg2(how, m_ba, m_ab);
  }
}

}  // namespace pair_tile
