// pairs_f64_tile.h -- the tile skeleton of the all-pairs f64 row kernels (gfx950, wave64), stated once: every pair of a
// 64 x 64 tile of row pairs gets acc = Term::add(acc, a[c], b[c]) over the columns c in ascending order.
// rowdist.hip (the squared difference, a run-time column count) and tetra.hip's correlation kernel (the product, 256
// columns) are its two users; each keeps its own bit contract, its own early return and its own epilogue.
//
// The functions below are inlined into the including kernel, and a Term's rounded product must not fuse with its
// addition into a v_fma_f64 (strict_fp.h).
//
// Layout: one 256-thread workgroup per tile.  Lane (ty, tx) = (tid / 16, tid % 16) holds the 4 x 4 pairs of rows
// i0 + 4 ty .. + 3 with rows j0 + 4 tx .. + 3: 16 accumulators, one per pair, so the order of a pair's additions is the
// column order whatever the tiling.  The two 64-row panels go through LDS kStage = 16 columns at a time.  Global reads run
// along the rows (a wave reads 4 rows x 128 contiguous bytes).  In LDS a panel is held transposed, [column][row] with a
// row stride of 66 doubles, so that a lane's four row values at one column are 32 contiguous, 16-byte-aligned bytes (two
// ds_read_b128 per panel): the 16 tx of a wave read 512 contiguous bytes, every bank once per ds_read_b128, and its 4 ty
// read four addresses that are broadcast.  The transposing ds_write_b64 of the staging step is 4-way conflicted whatever
// the stride (64 lanes x 2 words on 32 banks), which is its minimum; it is 1/16 of the LDS traffic.  The stage is
// double-buffered: the global loads of stage k + 1 are issued before the arithmetic of stage k and written to the other
// buffer after it, one barrier per stage.  The two buffers are 33 KB (33 792 bytes); with 114 VGPRs four workgroups fit a
// CU (__launch_bounds__(256, 4) on the kernels: four waves per SIMD).
// The column loop of a stage is unrolled by 4, not by kStage: fully unrolled, the compiler hoists all 64 ds_read_b128 of a
// stage above the arithmetic, takes 338 VGPRs for it and leaves one wave per SIMD; unrolled by 4 it is 114 VGPRs and four.
// A 32 x 32 tile for small n (at n = 1000 there are 136 tiles for 256 CUs) was not built: at that size the whole call
// takes tens of microseconds.
#ifndef PA_PAIRS_F64_TILE_H
#define PA_PAIRS_F64_TILE_H
#include <cstdint>

#include "strict_fp.h"

namespace pairs_f64 {

constexpr int kTile = 64;
constexpr int kThreads = 256;
constexpr int kStage = 16;                         // columns per stage
constexpr int kStride = kTile + 2;                 // doubles per LDS column: 16-byte aligned rows of four, see above
constexpr int kLoads = kTile * kStage / kThreads;  // doubles per lane, panel and stage

struct Staged {
  double a[kLoads], b[kLoads];
};

// the lane's share of columns [c0, c0 + kStage) of the two panels: element f = tid + 256 e is (row f / 16, column f % 16).
// Rows past the ends, and with kFixedCols == 0 columns past m, are staged as 0.0
template <int kFixedCols>
__device__ __forceinline__ void load_stage(const double *__restrict__ x, uint32_t m, uint32_t i0, uint32_t i_end, uint32_t j0, uint32_t j_end,
                                           uint32_t c0, Staged &st) {
  const uint32_t cols = kFixedCols > 0 ? (uint32_t)kFixedCols : m;
#pragma unroll
  for (int e = 0; e < kLoads; ++e) {
    const uint32_t f = threadIdx.x + kThreads * e;
    const uint32_t r = f / kStage, c = c0 + f % kStage;
    const uint32_t ia = i0 + r, jb = j0 + r;
    const bool in_cols = kFixedCols > 0 || c < cols;
    st.a[e] = (ia < i_end && in_cols) ? x[(uint64_t)ia * cols + c] : 0.0;
    st.b[e] = (jb < j_end && in_cols) ? x[(uint64_t)jb * cols + c] : 0.0;
  }
}

__device__ __forceinline__ void store_stage(double (*pa)[kStride], double (*pb)[kStride], const Staged &st) {
#pragma unroll
  for (int e = 0; e < kLoads; ++e) {
    const uint32_t f = threadIdx.x + kThreads * e;
    pa[f % kStage][f / kStage] = st.a[e];
    pb[f % kStage][f / kStage] = st.b[e];
  }
}

// acc[a][b] = 0.0, then acc[a][b] = Term::add(acc[a][b], x[i0 + 4 ty + a][c], x[j0 + 4 tx + b][c]) for every column c in
// ascending order.  The rows of x are m doubles apart; kFixedCols > 0 is that count at compile time (a multiple of kStage,
// no column guard, m is not read), kFixedCols == 0 takes it from m.  Every lane of the workgroup calls this, once per
// kernel: it owns the LDS panels and the barriers.  (ty, tx) is the lane's place in the tile, (tid / 16, tid % 16); the
// kernel's epilogue needs it too and hands it in -- worked out a second time here, the compiler keeps both copies live
// (116 VGPRs in place of 114 in rowdist.hip).
template <int kFixedCols, class Term>
__device__ __forceinline__ void pair_tile_accumulate(const double *__restrict__ x, uint32_t m, uint32_t i0, uint32_t i_end, uint32_t j0,
                                                     uint32_t j_end, uint32_t ty, uint32_t tx, double (&acc)[4][4]) {
  static_assert(kFixedCols >= 0 && kFixedCols % kStage == 0, "a compile-time column count is whole stages");
  __shared__ __attribute__((aligned(16))) double pa[2][kStage][kStride];
  __shared__ __attribute__((aligned(16))) double pb[2][kStage][kStride];
  const uint32_t n_stages = kFixedCols > 0 ? (uint32_t)(kFixedCols / kStage) : (m + kStage - 1) / kStage;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  Staged st;
  if (n_stages) {
    load_stage<kFixedCols>(x, m, i0, i_end, j0, j_end, 0, st);
    store_stage(pa[0], pb[0], st);
  }
  __syncthreads();
  for (uint32_t k = 0; k < n_stages; ++k) {
    const int cur = (int)(k & 1u);
    const bool more = k + 1 < n_stages;  // uniform in the workgroup
    if (more) load_stage<kFixedCols>(x, m, i0, i_end, j0, j_end, (k + 1) * kStage, st);
#pragma unroll 4
    for (int c = 0; c < kStage; ++c) {
      const double2 a01 = *reinterpret_cast<const double2 *>(&pa[cur][c][4 * ty]);
      const double2 a23 = *reinterpret_cast<const double2 *>(&pa[cur][c][4 * ty + 2]);
      const double2 b01 = *reinterpret_cast<const double2 *>(&pb[cur][c][4 * tx]);
      const double2 b23 = *reinterpret_cast<const double2 *>(&pb[cur][c][4 * tx + 2]);
      const double av[4] = {a01.x, a01.y, a23.x, a23.y};
      const double bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = Term::add(acc[a][b], av[a], bv[b]);
    }
    // the other buffer was last read in iteration k - 1, which every lane has left (the barrier below)
    if (more) store_stage(pa[cur ^ 1], pb[cur ^ 1], st);
    __syncthreads();
  }
}

}  // namespace pairs_f64

#endif  // PA_PAIRS_F64_TILE_H
