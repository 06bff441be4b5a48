// mantel.hip -- mantel-run-comp on the device (gfx950, wave64): the cross sums of two distance matrices under many
// permutations of the genomes of one of them, and the moments that turn them into Mantel's r.
//
// The definitions are this project's own: include/pyani_hip.h and DESIGN.md section 7j have the contract,
// tests/mantel_cases.py restates it independently, mantel_host.cpp has the twin with the same bits and the checks of the
// arguments, mantel_rule.h the constants and formulas of both.  A row's terms go to 64 accumulators by j % 64 and the
// accumulators are added as a tree: here an accumulator is a lane of a wave, and a wave walks a row of X in blocks of 64
// aligned columns, so that lane l meets exactly the columns j with j % 64 == l, in ascending order.
//
// The cross kernel.  cross(pi) pairs row i of X with row pi[i] of Y read at the columns pi[j]: a gather.  A workgroup
// owns one row r of Y: it loads the row once, coalesced and already centred, into dynamic LDS (8 n bytes, up to 128 KB).
// Its waves share out the permutations of the batch; for a permutation the wave looks up i = pi^-1[r] (the inverses are
// made on the host beside the check that keeps every pi[j] inside the row), streams X[i, j] and pi[j] for j > i
// coalesced, kUnroll blocks in flight, gathers y from LDS at pi[j], and each lane adds its products in order.  The tree
// over the lanes gives the row's sum, which goes to rows[i][permutation]; a second kernel adds a permutation's rows in
// ascending i, one lane per permutation, reading coalesced across the permutations.  No floating-point atomics.
//
// A call works through the identity and the permutations PA_MANTEL_BATCH at a time, so that the workspace is bounded:
// the batch's permutations and inverses (u32) and its row sums (f64), n each.  The cross sums collect on the device and
// come back once.
#include "pa_internal.h"

#include "mantel_rule.h"

namespace {

using mantel::kLanes;
using mantel::kSumStart;

constexpr int kThreads = 256;       // lanes per workgroup of the cell-wise and row kernels, and of the cross kernel for short rows
constexpr int kThreadsLong = 1024;  // ... for rows past kShortRow: a workgroup holds 32 KB of LDS and more, so few fit a CU
constexpr uint32_t kShortRow = 4096;
constexpr int kUnroll = 4;          // blocks of 64 columns a wave has in flight
constexpr int kChainLoads = 8;      // loads of a lane in flight before the first is added (the chains)
constexpr uint32_t kBatch = PA_MANTEL_BATCH;
constexpr uint32_t kCrossWaves = 16384;  // waves the cross kernel's grid aims at: rows times slices of the batch
static_assert((uint64_t)PA_MANTEL_MAX_N * 8 <= 160u * 1024, "a row of Y fits the LDS of a CU");

// the tree over the accumulators: lane 0 ends with the row's sum
__device__ __forceinline__ double lanes_tree(double a, uint32_t lane) {
#pragma unroll
  for (uint32_t w = kLanes / 2; w >= 1; w /= 2) {
    const double other = __shfl_down(a, w, kLanes);
    if (lane < w) a = a + other;
  }
  return a;
}

// out[i] = the sum of row i's terms, j > i: M[i, j] itself (mean == nullptr) or the square of M[i, j] - *mean.
// One wave per row.
__global__ __launch_bounds__(kThreads) void mantel_rows_kernel(const double *__restrict__ M, uint32_t n, const double *__restrict__ mean,
                                                             double *__restrict__ out) {
  const uint32_t lane = threadIdx.x % kLanes, i = blockIdx.x * (kThreads / kLanes) + threadIdx.x / kLanes;
  if (i >= n) return;  // a whole wave
  const double *row = M + (uint64_t)i * n;
  const double mu = mean ? *mean : 0.0;
  double a = kSumStart;
  for (uint32_t j = ((i + 1) & ~(kLanes - 1)) + lane; j < n; j += kLanes) {
    if (j <= i) continue;
    a = mean ? mantel::add_square(a, mantel::centred(row[j], mu)) : a + row[j];
  }
  a = lanes_tree(a, lane);
  if (lane == 0) out[i] = a;
}

// out[q] = (((-0.0 + rows[0][q]) + rows[1][q]) + ...) + rows[n - 1][q], divided by `divisor` where that is not 0:
// one lane per q, because the order is the contract's; rows[i][q] is at i * stride + q
__global__ __launch_bounds__(kLanes) void mantel_chain_kernel(const double *__restrict__ rows, uint32_t n, uint32_t stride, uint32_t count,
                                                             double divisor, double *__restrict__ out) {
  const uint32_t q = blockIdx.x * kLanes + threadIdx.x;
  if (q >= count) return;
  double s = kSumStart;
  for (uint32_t i0 = 0; i0 < n; i0 += kChainLoads) {
    double v[kChainLoads];
#pragma unroll
    for (int t = 0; t < kChainLoads; ++t) v[t] = i0 + t < n ? rows[(uint64_t)(i0 + t) * stride + q] : 0.0;
#pragma unroll
    for (int t = 0; t < kChainLoads; ++t)
      if (i0 + t < n) s = s + v[t];
  }
  out[q] = divisor != 0.0 ? s / divisor : s;
}

// Workgroup blockIdx.x owns row r of Y; slice blockIdx.y of the batch's permutations goes to its waves.
// rows[i * stride + q] = the sum of (X[i, j] - mean_x) * (Y[pi_q[i], pi_q[j]] - mean_y) over j > i, for i = pi_q^-1[r].
// Every perms[] value is below n (mantel::check_arguments), so every LDS index is inside the row.
__global__ __launch_bounds__(kThreadsLong) void mantel_cross_kernel(const double *__restrict__ X, const double *__restrict__ Y, uint32_t n,
                                                                  const double *__restrict__ stats, const uint32_t *__restrict__ perms,
                                                                  const uint32_t *__restrict__ inverse, uint32_t count, uint32_t stride,
                                                                  double *__restrict__ rows) {
  extern __shared__ double s_y[];
  const uint32_t r = blockIdx.x;
  const double mean_x = stats[0], mean_y = stats[1];
  const double *y_row = Y + (uint64_t)r * n;
  for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) s_y[j] = mantel::centred(y_row[j], mean_y);  // s_y[r] is never gathered
  __syncthreads();
  const uint32_t lane = threadIdx.x % kLanes, waves = blockDim.x / kLanes;
  for (uint32_t q = blockIdx.y * waves + threadIdx.x / kLanes; q < count; q += gridDim.y * waves) {
    const uint32_t *pi = perms + (uint64_t)q * n;
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)inverse[(uint64_t)q * n + r]);
    const double *x_row = X + (uint64_t)i * n;
    double a = kSumStart;
    for (uint32_t j0 = ((i + 1) & ~(kLanes - 1)) + lane; j0 < n + lane; j0 += kUnroll * kLanes) {
      double x[kUnroll];
      uint32_t p[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t j = j0 + u * kLanes;
        const bool live = j > i && j < n;
        x[u] = live ? x_row[j] : 0.0;
        p[u] = live ? pi[j] : 0u;
      }
      double y[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) y[u] = s_y[p[u]];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t j = j0 + u * kLanes;
        if (j > i && j < n) a = mantel::add_product(a, mantel::centred(x[u], mean_x), y[u]);
      }
    }
    a = lanes_tree(a, lane);
    if (lane == 0) rows[(uint64_t)i * stride + q] = a;
  }
}

// the workspace of a call over `total` cross sums (the identity's and the permutations')
struct Work {
  double *stats;            // mean_x, mean_y, ss_x, ss_y
  double *cross;            // `total` sums
  double *rows;             // n x kBatch row sums; the moments use its first n
  uint32_t *perms, *inverse;  // kBatch x n each
  void layout(Carve &k, uint32_t n, uint64_t total) {
    stats = k.take<double>(4);
    // stats is given 64 bytes for its 32: 32 bytes earlier, every 256-byte wave read of pi in the cross kernel at N = 10 000,
    // 1 000 sums (rows of 40 000 bytes) spans three 128-byte lines where every other permutation's spans two: 0.7 % of the call
    k.slack(64 - 4 * sizeof(double));
    cross = k.take<double>(total);
    rows = k.take<double>((uint64_t)n * kBatch);
    perms = k.take<uint32_t>((uint64_t)n * kBatch);
    inverse = k.take<uint32_t>((uint64_t)n * kBatch);
  }
};

// pa_mantel behind the checks of its arguments; the host arrays it copies from outlive the stream's work (the caller waits)
int mantel_device(pa_ctx *c, const double *d_X, const double *d_Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms,
                  const std::vector<uint32_t> &h_inverse, double *h_stats, double *h_cross) {
  const uint64_t total = n_perms + 1;
  Work w;
  PA_TRY(pa_carve(c->mantel_work, "mantel_work", [&](Carve &k) { w.layout(k, n, total); }));
  const double *matrices[2] = {d_X, d_Y};
  const char *const names[2] = {"X", "Y"};
  PA_TRY(pa_check_distance_matrices(c, "pa_mantel", names, matrices, 2, n));  // one read-back for both
  // the moments: stats[m] = tri(M) / pairs, stats[2 + m] = tri of the centred squares
  const uint32_t row_blocks = (n + kThreads / kLanes - 1) / (kThreads / kLanes);
  const double pairs = (double)((uint64_t)n * (n - 1) / 2);
  for (int m = 0; m < 2; ++m) {
    PA_TRY(PA_LAUNCH(c, mantel_rows_kernel, row_blocks, kThreads, 0, matrices[m], n, (const double *)nullptr, w.rows));
    PA_TRY(PA_LAUNCH(c, mantel_chain_kernel, 1, kLanes, 0, (const double *)w.rows, n, 1u, 1u, pairs, w.stats + m));
    PA_TRY(PA_LAUNCH(c, mantel_rows_kernel, row_blocks, kThreads, 0, matrices[m], n, (const double *)(w.stats + m), w.rows));
    PA_TRY(PA_LAUNCH(c, mantel_chain_kernel, 1, kLanes, 0, (const double *)w.rows, n, 1u, 1u, 0.0, w.stats + 2 + m));
  }
  // the cross sums, a batch at a time: sum g is the identity's for g = 0 and row g - 1's otherwise
  const uint32_t threads = n <= kShortRow ? kThreads : kThreadsLong, waves = threads / kLanes;
  for (uint64_t g0 = 0; g0 < total; g0 += kBatch) {
    const uint32_t count = (uint32_t)std::min<uint64_t>(kBatch, total - g0);
    const uint32_t own = g0 == 0 ? 1 : 0;  // the identity's row: the first of h_inverse is one
    if (own) PA_HIP(hipMemcpyAsync(w.perms, h_inverse.data(), (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (count > own)
      PA_HIP(hipMemcpyAsync(w.perms + (uint64_t)own * n, h_perms + (g0 + own - 1) * n, (uint64_t)(count - own) * n * 4, hipMemcpyHostToDevice, c->stream));
    PA_HIP(hipMemcpyAsync(w.inverse, h_inverse.data() + g0 * n, (uint64_t)count * n * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t slices = std::min<uint32_t>((count + waves - 1) / waves, std::max<uint32_t>(1, kCrossWaves / waves / n));
    PA_TRY(PA_LAUNCH_RAISE_LDS(c, mantel_cross_kernel, LaunchDim(n, slices), threads, (size_t)n * 8, d_X, d_Y, n, (const double *)w.stats,
                               (const uint32_t *)w.perms, (const uint32_t *)w.inverse, count, kBatch, w.rows));
    PA_TRY(PA_LAUNCH(c, mantel_chain_kernel, (count + kLanes - 1) / kLanes, kLanes, 0, (const double *)w.rows, n, kBatch, count, 0.0, w.cross + g0));
  }
  PA_HIP(hipMemcpyAsync(h_stats, w.stats, 32, hipMemcpyDeviceToHost, c->stream));
  return pa_copy_to_host(c, h_cross, w.cross, total * 8);
}

}  // namespace

extern "C" int pa_mantel(pa_ctx *c, const double *d_X, const double *d_Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, double *h_stats,
                         double *h_cross) {
  PA_REQUIRE(c != nullptr, "pa_mantel: null context");
  std::vector<uint32_t> h_inverse;
  PA_TRY(mantel::check_arguments(d_X, d_Y, n, h_perms, n_perms, h_stats, h_cross, &h_inverse));  // does not throw
  PA_HIP(hipSetDevice(c->device));
  const int status = mantel_device(c, d_X, d_Y, n, h_perms, n_perms, h_inverse, h_stats, h_cross);
  if (status != PA_OK) (void)hipStreamSynchronize(c->stream);  // copies from h_inverse may still be queued
  return status;
}
