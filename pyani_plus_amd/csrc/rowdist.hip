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
//     v_fma_f64 with an unrounded product: strict_fp.h below switches contraction off for this whole file (the Makefile
//     passes -ffp-contract=off for it as well), and the loop below compiles to v_add_f64, v_mul_f64, v_add_f64;
//   * the square root is the correctly rounded one: __dsqrt_rn, which the compiler expands into v_rsq_f64 plus a
//     Newton-Raphson refinement with v_fma_f64 and a scaling of very small and very large arguments.  The bare v_sqrt_f64
//     is an approximation and is not used;
//   * the inputs are finite (plot_run fills NaN cells before it clusters).  Columns past m are staged as 0.0 in both
//     panels: they add (0 - 0)^2 = +0.0 to a sum that is never -0.0, which leaves every bit of it.
//
// Layout: pairs_f64_tile.h (the 64 x 64 tile of pairs per 256-thread workgroup, the two panels staged through LDS, the
// bank argument, the double buffer, the register count), here with the run-time column count m and its column guard;
// grid nt x nt, the tiles below the diagonal return at once, as in classify.hip.
#include "pa_internal.h"

#include "pairs_f64_tile.h"

namespace {

using namespace pairs_f64;

struct EuclidTerm {
  static __device__ __forceinline__ double add(double acc, double a, double b) {
    const double d = a - b;
    const double sq = d * d;  // rounded here: contraction is off for this file
    return acc + sq;
  }
};

__global__ __launch_bounds__(kThreads, 4) void rowdist_euclid_kernel(const double *__restrict__ x, uint32_t n, uint32_t m,
                                                                  double *__restrict__ out) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  const uint32_t i0 = ti * kTile, j0 = tj * kTile;
  const uint32_t ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  double acc[4][4];
  pair_tile_accumulate<0, EuclidTerm>(x, m, i0, n, j0, n, ty, tx, acc);

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
