// rowdist.hip -- the Euclidean distances between the rows of an f64 matrix, all pairs, on the device (gfx950, wave64).
//
// plot-run orders a heatmap by a hierarchical clustering of the matrix rows.  The reference's stack does that with
// scipy's pdist(rows, "euclidean") on one host thread: n (n - 1) / 2 pairs of m-long rows, n^2 m / 2 subtract-multiply-add
// steps.  This kernel writes the same condensed vector, d[idx(i, j)] for i < j with idx = n i - i (i + 1) / 2 + (j - i - 1),
// with the same bits.  DESIGN.md section 7c has the contract, the layout and the measurements.
//
// Bit contract (what makes the result equal to pdist's, and to pa_rowdist_euclid_host's, bit for bit):
//   * one accumulator per pair, the columns added in ascending order: s = s + (a - b) * (a - b).  No split over the
//     columns, no atomics: either would change the order of the additions;
//   * the square is rounded before it is added.  hipcc's default is -ffp-contract=fast, which would turn s + d * d into one
//     v_fma_f64 with an unrounded product: the pragma below switches contraction off for this whole file (the Makefile
//     passes -ffp-contract=off for it as well), and the loop below compiles to v_add_f64, v_mul_f64, v_add_f64;
//   * the square root is the correctly rounded one: __dsqrt_rn, which the compiler expands into v_rsq_f64 plus a
//     Newton-Raphson refinement with v_fma_f64 and a scaling of very small and very large arguments.  The bare v_sqrt_f64
//     is an approximation and is not used;
//   * the inputs are finite (plot_run fills NaN cells before it clusters).  Columns past m are staged as 0.0 in both
//     panels: they add (0 - 0)^2 = +0.0 to a sum that is never -0.0, which leaves every bit of it.
//
// Layout: one 256-thread workgroup per 64 x 64 tile of pairs on or above the diagonal (grid nt x nt, the tiles below
// return at once, as in classify.hip).  Lane (ty, tx) = (tid / 16, tid % 16) holds the 4 x 4 pairs of rows
// i0 + 4 ty .. + 3 with rows j0 + 4 tx .. + 3: 16 accumulators.  The two 64-row panels go through LDS kChunk = 16 columns at
// a time.  Global reads run along the rows (a wave reads 4 rows x 128 contiguous bytes).  In LDS a panel is held
// transposed, [column][row] with a row stride of 66 doubles, so that a lane's four row values at one column are 32
// contiguous, 16-byte-aligned bytes (two ds_read_b128 per panel): the 16 tx of a wave read 512 contiguous bytes, every
// bank once per ds_read_b128, and its 4 ty read four addresses that are broadcast.  The transposing
// ds_write_b64 of the staging step is 4-way conflicted whatever the stride (64 lanes x 2 words on 32 banks), which is its
// minimum; it is 1/16 of the LDS traffic.  The stage is double-buffered: the global loads of chunk k + 1 are issued
// before the arithmetic of chunk k and written to the other buffer after it, one barrier per chunk.  The two buffers are
// 33 KB; with 114 VGPRs four workgroups fit a CU (__launch_bounds__(256, 4): four waves per SIMD).
// A 32 x 32 tile for small n (at n = 1000 there are 136 tiles for 256 CUs) was not built: at that size the whole call
// takes tens of microseconds.
#include "pa_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 64;
constexpr int kThreads = 256;
constexpr int kChunk = 16;             // columns per stage
constexpr int kStride = kTile + 2;     // doubles per LDS column: 16-byte aligned rows of four, see above
constexpr int kLoads = kTile * kChunk / kThreads;  // doubles per lane, panel and stage

struct Staged {
  double a[kLoads], b[kLoads];
};

// the lane's share of columns [c0, c0 + kChunk) of the two panels: element f = tid + 256 e is (row f / 16, column f % 16)
__device__ __forceinline__ void load_stage(const double *__restrict__ x, uint32_t n, uint32_t m, uint32_t i0, uint32_t j0, uint32_t c0,
                                           Staged &st) {
#pragma unroll
  for (int e = 0; e < kLoads; ++e) {
    const uint32_t f = threadIdx.x + kThreads * e;
    const uint32_t r = f / kChunk, c = c0 + f % kChunk;
    const uint32_t ia = i0 + r, jb = j0 + r;
    st.a[e] = (ia < n && c < m) ? x[(uint64_t)ia * m + c] : 0.0;
    st.b[e] = (jb < n && c < m) ? x[(uint64_t)jb * m + c] : 0.0;
  }
}

__device__ __forceinline__ void store_stage(double (*pa)[kStride], double (*pb)[kStride], const Staged &st) {
#pragma unroll
  for (int e = 0; e < kLoads; ++e) {
    const uint32_t f = threadIdx.x + kThreads * e;
    pa[f % kChunk][f / kChunk] = st.a[e];
    pb[f % kChunk][f / kChunk] = st.b[e];
  }
}

__global__ __launch_bounds__(kThreads, 4) void rowdist_euclid_kernel(const double *__restrict__ x, uint32_t n, uint32_t m,
                                                                  double *__restrict__ out) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  __shared__ __attribute__((aligned(16))) double pa[2][kChunk][kStride];
  __shared__ __attribute__((aligned(16))) double pb[2][kChunk][kStride];
  const uint32_t i0 = ti * kTile, j0 = tj * kTile;
  const uint32_t ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;

  const uint32_t n_chunks = (m + kChunk - 1) / kChunk;
  Staged st;
  if (n_chunks) {
    load_stage(x, n, m, i0, j0, 0, st);
    store_stage(pa[0], pb[0], st);
  }
  __syncthreads();
  for (uint32_t k = 0; k < n_chunks; ++k) {
    const int cur = (int)(k & 1u);
    const bool more = k + 1 < n_chunks;  // uniform in the workgroup
    if (more) load_stage(x, n, m, i0, j0, (k + 1) * kChunk, st);
    // unrolled by 4, not by kChunk: fully unrolled, the compiler hoists all 64 ds_read_b128 of a chunk above the
    // arithmetic, takes 338 VGPRs for it and leaves one wave per SIMD; this way it is 114 VGPRs and four
#pragma unroll 4
    for (int c = 0; c < kChunk; ++c) {
      const double2 a01 = *reinterpret_cast<const double2 *>(&pa[cur][c][4 * ty]);
      const double2 a23 = *reinterpret_cast<const double2 *>(&pa[cur][c][4 * ty + 2]);
      const double2 b01 = *reinterpret_cast<const double2 *>(&pb[cur][c][4 * tx]);
      const double2 b23 = *reinterpret_cast<const double2 *>(&pb[cur][c][4 * tx + 2]);
      const double av[4] = {a01.x, a01.y, a23.x, a23.y};
      const double bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double d = av[a] - bv[b];
          const double sq = d * d;  // rounded here: contraction is off for this file
          acc[a][b] = acc[a][b] + sq;
        }
    }
    // the other buffer was last read in iteration k - 1, which every lane has left (the barrier below)
    if (more) store_stage(pa[cur ^ 1], pb[cur ^ 1], st);
    __syncthreads();
  }

#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t i = i0 + 4 * ty + a;
    if (i >= n) continue;
    const uint64_t row_base = (uint64_t)n * i - (uint64_t)i * (i + 1) / 2;  // idx(i, j) = row_base + (j - i - 1)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = j0 + 4 * tx + b;
      if (j < n && j > i) out[row_base + (j - i - 1)] = __dsqrt_rn(acc[a][b]);
    }
  }
}

}  // namespace

extern "C" int pa_rowdist_euclid(pa_ctx *c, const double *d_x, uint32_t n, uint32_t m, double *d_out) {
  PA_REQUIRE(c != nullptr, "pa_rowdist_euclid: null context");
  PA_REQUIRE(n <= (1u << 16), "pa_rowdist_euclid: %u rows; at most 65536", n);
  if (n < 2) return PA_OK;  // no pair
  PA_REQUIRE(d_out != nullptr && (m == 0 || d_x != nullptr), "pa_rowdist_euclid: null argument");
  PA_HIP(hipSetDevice(c->device));
  ProfScope prof(c, PA_PROF_ROWDIST);
  const uint32_t nt = (n + kTile - 1) / kTile;
  return PA_LAUNCH(c, rowdist_euclid_kernel, LaunchDim(nt, nt), kThreads, 0, d_x, n, m, d_out);
}
