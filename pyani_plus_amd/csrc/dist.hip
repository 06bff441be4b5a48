// dist.hip -- plot-run's score distributions on the device (gfx950, wave64): the order statistics the automatic bin
// rule needs, the moments behind Scott's bandwidth and the Gaussian kernel density on a grid.  The histogram itself is
// hist.hip's.  DESIGN.md section 7e has the definitions and the error bound.
//
// pa_select_f64: an MSB radix select.  A double becomes a u64 key whose unsigned order is the order of the values (the
// sign bit flipped for positive values, all bits for negative ones; -0.0 sorts directly below 0.0, which is the same
// value).  Eight passes, one per byte from the top: a pass counts, for every live prefix (the bytes chosen so far for
// one requested rank; ranks that still agree share one), the next byte of the keys that begin with that prefix, in
// 256 u32 counters per prefix in LDS, added once per workgroup to u64 counters in global memory.  The host reads the
// at most 8 x 256 counters, walks each rank down its histogram and extends its prefix.  After the eighth pass the
// prefix is the key.  Integer counters only, no sort, no copy of the data; eight host synchronisations.
//
// pa_moments_f64: two grid-stride passes with the same shape: a lane adds its elements in index order, a workgroup
// reduces its 256 lanes by halving in LDS, a one-workgroup kernel reduces the workgroups' partials the same way.  The
// first pass gives the count and the sum, the one-workgroup kernel leaves mean = sum / count on the device, the second
// pass sums (x - mean)^2.  The grid depends on n alone, so two runs add in the same order.  No atomics.
//
// pa_kde_gauss_f64: sum_i exp(-0.5 ((g_j - v_i) / bw)^2) for up to 1024 grid points g_j.  A workgroup has 1024
// accumulators (256 lanes x 4 registers), each with its grid point in a register: accumulator a serves grid point
// a % n_grid and data slice a / n_grid of S slices, S the largest power of two with S n_grid <= 1024.  A workgroup
// takes kKdeChain * S consecutive data, staged 1024 at a time in LDS (each datum is read from global memory once per
// workgroup); slice s takes the staged elements s, s + S, ..., so an accumulator adds exactly kKdeChain terms one
// after the other.  NaN and the positions past n are staged as +inf, whose term is exp(-inf) = 0: adding it changes
// nothing.  The S slices of a grid point are added by halving in LDS, the workgroups' sums by halving in global memory
// (one small launch per level): a fixed tree, no atomics, the same bits run to run.  The division and the exponent
// are the definition's: (g - v) / bw correctly rounded, its square, times -0.5 (contraction is off for this file).
#include <cmath>
#include <cstring>

#include "block_reduce_dev.h"
#include "pa_internal.h"
#include "strict_fp.h"

namespace {

constexpr int kThreads = kStrideThreads;
constexpr uint32_t kMaxRanks = PA_SELECT_MAX_RANKS;
constexpr uint32_t kKdeChain = PA_KDE_CHAIN;  // c: the longest run of sequential additions of the density sum
constexpr uint32_t kKdeAcc = 4;               // accumulators (grid point, slice) per lane
constexpr uint32_t kKdeSlots = kThreads * kKdeAcc;  // 1024: accumulators per workgroup, and data staged at a time
static_assert(kKdeSlots == 1024 && kKdeChain % kKdeSlots == 0, "a slice of every S <= 1024 takes whole staged blocks");

// ---- select -------------------------------------------------------------------
__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
inline double key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

struct SelectPrefixes {
  uint64_t prefix[kMaxRanks];  // the bytes above `shift + 8` of the keys a group counts
  uint32_t n;
};

// counts[256 g + d] += the non-NaN elements whose key begins with prefix g and has byte d at `shift`
__global__ __launch_bounds__(kThreads) void dist_select_kernel(const double *__restrict__ v, uint64_t n, SelectPrefixes live, uint32_t shift,
                                                               unsigned long long *__restrict__ counts) {
  __shared__ uint32_t s_counts[kMaxRanks * 256];
  for (uint32_t b = threadIdx.x; b < live.n * 256; b += kThreads) s_counts[b] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
    const double x = v[i];
    if (x == x) {
      const uint64_t key = order_key(x);
      const uint64_t head = shift == 56 ? 0ULL : key >> (shift + 8);
      const uint32_t digit = (uint32_t)(key >> shift) & 255u;
      for (uint32_t g = 0; g < live.n; ++g)
        if (head == live.prefix[g]) atomicAdd(&s_counts[g * 256 + digit], 1u);  // the prefixes differ: at most one g
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < live.n * 256; b += kThreads)
    if (s_counts[b]) atomicAdd(&counts[b], (unsigned long long)s_counts[b]);
}

// ---- moments ------------------------------------------------------------------
// the sum of the workgroup's `x`, by halving: a fixed tree
template <typename T>
__device__ __forceinline__ T block_sum(T x, T *s_x) {
  return pa_dev::block_reduce<kThreads>(x, s_x, [](T a, T b) { return a + b; });
}

// SQUARES false: partial[2 b] = the sum of workgroup b's non-NaN elements, partial[2 b + 1] = the bits of their number.
// SQUARES true: partial[2 b] = the sum of (x - *mean)^2 over them.
template <bool SQUARES>
__global__ __launch_bounds__(kThreads) void dist_moments_kernel(const double *__restrict__ v, uint64_t n, const double *__restrict__ mean,
                                                                double *__restrict__ partial) {
  __shared__ double s_sum[kThreads];
  __shared__ unsigned long long s_cnt[kThreads];
  const double m = SQUARES ? *mean : 0.0;
  double sum = 0.0;
  unsigned long long cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
    const double x = v[i];
    if (x == x) {
      const double d = x - m;
      sum += SQUARES ? d * d : x;
      ++cnt;
    }
  }
  sum = block_sum(sum, s_sum);
  if (!SQUARES) cnt = block_sum(cnt, s_cnt);
  if (threadIdx.x == 0) {
    partial[2 * (uint64_t)blockIdx.x] = sum;
    if (!SQUARES) partial[2 * (uint64_t)blockIdx.x + 1] = __longlong_as_double((long long)cnt);
  }
}

// one workgroup.  SQUARES false: result[0] = sum / count (the mean), result[2] = the count's bits.  true: result[1] = sum.
template <bool SQUARES>
__global__ __launch_bounds__(kThreads) void dist_moments_final_kernel(const double *__restrict__ partial, uint32_t n_partial,
                                                                      double *__restrict__ result) {
  __shared__ double s_sum[kThreads];
  __shared__ unsigned long long s_cnt[kThreads];
  double sum = 0.0;
  unsigned long long cnt = 0;
  for (uint32_t b = threadIdx.x; b < n_partial; b += kThreads) {
    sum += partial[2 * (uint64_t)b];
    if (!SQUARES) cnt += (unsigned long long)__double_as_longlong(partial[2 * (uint64_t)b + 1]);
  }
  sum = block_sum(sum, s_sum);
  if (!SQUARES) cnt = block_sum(cnt, s_cnt);
  if (threadIdx.x == 0) {
    if (SQUARES) {
      result[1] = sum;
    } else {
      result[0] = cnt ? sum / (double)cnt : 0.0;
      result[2] = __longlong_as_double((long long)cnt);
    }
  }
}

// ---- kernel density -------------------------------------------------------------
// partial[blockIdx.x * n_grid + j] = the sum over the workgroup's data of exp(-0.5 ((grid[j] - v) / bw)^2)
__global__ __launch_bounds__(kThreads) void dist_kde_kernel(const double *__restrict__ v, uint64_t n, const double *__restrict__ grid,
                                                            uint32_t n_grid, uint32_t slices /*S*/, double bw, double *__restrict__ partial) {
  __shared__ double s_x[kKdeSlots];  // the staged data, then the accumulators
  const uint32_t used = slices * n_grid;  // <= kKdeSlots
  double g[kKdeAcc], acc[kKdeAcc];
  uint32_t slice[kKdeAcc];
#pragma unroll
  for (uint32_t r = 0; r < kKdeAcc; ++r) {
    const uint32_t a = threadIdx.x + r * kThreads;
    const bool on = a < used;
    g[r] = on ? grid[a % n_grid] : 0.0;
    slice[r] = on ? a / n_grid : 0u;
    acc[r] = 0.0;
  }
  const uint64_t base = (uint64_t)blockIdx.x * kKdeChain * slices;
  const uint32_t n_stage = kKdeChain * slices / kKdeSlots;  // staged blocks of the workgroup
  const uint32_t per_stage = kKdeSlots / slices;            // terms an accumulator adds per staged block
  for (uint32_t st = 0; st < n_stage; ++st) {
    const uint64_t at = base + (uint64_t)st * kKdeSlots;
    if (at >= n) break;  // uniform: the later blocks lie further on
#pragma unroll
    for (uint32_t r = 0; r < kKdeAcc; ++r) {
      const uint64_t i = at + threadIdx.x + r * kThreads;
      const double x = i < n ? v[i] : __builtin_inf();
      s_x[threadIdx.x + r * kThreads] = x == x ? x : __builtin_inf();
    }
    __syncthreads();
    for (uint32_t k = 0; k < per_stage; ++k) {
#pragma unroll
      for (uint32_t r = 0; r < kKdeAcc; ++r) {
        const double z = (g[r] - s_x[k * slices + slice[r]]) / bw;
        acc[r] += exp(-0.5 * (z * z));
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (uint32_t r = 0; r < kKdeAcc; ++r) s_x[threadIdx.x + r * kThreads] = acc[r];  // accumulator a = slice * n_grid + point
  __syncthreads();
  for (uint32_t step = slices / 2; step > 0; step >>= 1) {
    for (uint32_t a = threadIdx.x; a < step * n_grid; a += kThreads) s_x[a] += s_x[a + step * n_grid];
    __syncthreads();
  }
  for (uint32_t j = threadIdx.x; j < n_grid; j += kThreads) partial[(uint64_t)blockIdx.x * n_grid + j] = s_x[j];
}

// one level of the tree over the workgroups' sums: row w += row w + step for w < step, w + step < rows
__global__ __launch_bounds__(kThreads) void dist_kde_fold_kernel(double *__restrict__ partial, uint32_t rows, uint32_t step, uint32_t n_grid) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t w = i / n_grid;
  if (w < step && w + step < rows) partial[i] += partial[i + (uint64_t)step * n_grid];
}

}  // namespace

extern "C" int pa_select_f64(pa_ctx *c, const double *d_v, uint64_t n, const uint64_t *h_ranks, uint32_t n_ranks, double *h_out) {
  PA_REQUIRE(c != nullptr, "pa_select_f64: null argument");
  PA_REQUIRE(n_ranks <= kMaxRanks, "pa_select_f64: %u ranks; at most %u", n_ranks, kMaxRanks);
  if (n_ranks == 0) return PA_OK;
  PA_REQUIRE(h_ranks != nullptr && h_out != nullptr, "pa_select_f64: null argument");
  PA_REQUIRE(n == 0 || d_v != nullptr, "pa_select_f64: null array");
  PA_REQUIRE(n < (1ULL << 40), "pa_select_f64: %llu values; a workgroup's counters are 32-bit", (unsigned long long)n);
  uint64_t prefix[kMaxRanks] = {0}, rank[kMaxRanks];  // per requested rank: the bytes chosen so far, the rank within them
  for (uint32_t r = 0; r < n_ranks; ++r) rank[r] = h_ranks[r];
  if (n == 0) {
    pa_set_error("pa_select_f64: rank %llu of 0 values", (unsigned long long)rank[0]);
    return PA_E_INVALID;
  }
  PA_HIP(hipSetDevice(c->device));
  PA_TRY(c->hist.reserve((uint64_t)kMaxRanks * 256 * 8));
  unsigned long long *d_counts = c->hist.as<unsigned long long>();
  std::vector<uint64_t> counts((size_t)kMaxRanks * 256);
  for (uint32_t pass = 0; pass < 8; ++pass) {
    const uint32_t shift = 56 - 8 * pass;
    SelectPrefixes live;
    live.n = 0;
    uint32_t group[kMaxRanks];
    for (uint32_t r = 0; r < n_ranks; ++r) {
      uint32_t g = 0;
      while (g < live.n && live.prefix[g] != prefix[r]) ++g;
      if (g == live.n) live.prefix[live.n++] = prefix[r];
      group[r] = g;
    }
    for (uint32_t g = live.n; g < kMaxRanks; ++g) live.prefix[g] = 0;
    PA_HIP(hipMemsetAsync(d_counts, 0, (uint64_t)live.n * 256 * 8, c->stream));
    PA_TRY(PA_LAUNCH(c, dist_select_kernel, stride_blocks(n), kThreads, 0, d_v, n, live, shift, d_counts));
    PA_TRY(pa_copy_to_host(c, counts.data(), d_counts, (uint64_t)live.n * 256 * 8));
    for (uint32_t r = 0; r < n_ranks; ++r) {
      const uint64_t *h = counts.data() + (size_t)group[r] * 256;
      uint32_t d = 0;
      uint64_t below = 0;
      while (d < 256 && below + h[d] <= rank[r]) below += h[d++];
      if (d == 256) {  // only in the first pass: `below` is the number of non-NaN values
        pa_set_error("pa_select_f64: rank %llu of %llu values that are not NaN", (unsigned long long)h_ranks[r], (unsigned long long)below);
        return PA_E_INVALID;
      }
      rank[r] -= below;
      prefix[r] = (prefix[r] << 8) | d;
    }
  }
  for (uint32_t r = 0; r < n_ranks; ++r) h_out[r] = key_value(prefix[r]);
  return PA_OK;
}

extern "C" int pa_moments_f64(pa_ctx *c, const double *d_v, uint64_t n, double *out) {
  PA_REQUIRE(c != nullptr && out != nullptr, "pa_moments_f64: null argument");
  if (n == 0) return PA_OK;
  PA_REQUIRE(d_v != nullptr, "pa_moments_f64: null array");
  PA_HIP(hipSetDevice(c->device));
  const uint32_t blocks = stride_blocks(n);
  double *d_partial, *d_result;  // d_result: mean, sum of squared deviations, the count's bits
  PA_TRY(pa_carve(c->hist, "hist", [&](Carve &k) { d_partial = k.take<double>(2 * (uint64_t)blocks); d_result = k.take<double>(3); }));
  PA_TRY(PA_LAUNCH(c, dist_moments_kernel<false>, blocks, kThreads, 0, d_v, n, (const double *)nullptr, d_partial));
  PA_TRY(PA_LAUNCH(c, dist_moments_final_kernel<false>, 1, kThreads, 0, (const double *)d_partial, blocks, d_result));
  PA_TRY(PA_LAUNCH(c, dist_moments_kernel<true>, blocks, kThreads, 0, d_v, n, (const double *)d_result, d_partial));
  PA_TRY(PA_LAUNCH(c, dist_moments_final_kernel<true>, 1, kThreads, 0, (const double *)d_partial, blocks, d_result));
  double result[3];
  PA_TRY(pa_read_back(c, d_result, result, 3));
  uint64_t valid;
  memcpy(&valid, &result[2], sizeof valid);
  if (valid) {  // without a value that is not NaN, out is left as it is
    out[0] = result[0];
    out[1] = result[1];
  }
  return PA_OK;
}

extern "C" int pa_kde_gauss_f64(pa_ctx *c, const double *d_v, uint64_t n, const double *h_grid, uint32_t n_grid, double bw, double *h_density) {
  PA_REQUIRE(c != nullptr && h_grid != nullptr && h_density != nullptr, "pa_kde_gauss_f64: null argument");
  PA_REQUIRE(n_grid >= 1 && n_grid <= kKdeSlots, "pa_kde_gauss_f64: %u grid points; 1 to 1024", n_grid);
  PA_REQUIRE(bw > 0.0 && bw - bw == 0.0, "pa_kde_gauss_f64: the bandwidth %g must be positive and finite", bw);
  for (uint32_t j = 0; j < n_grid; ++j) PA_REQUIRE(h_grid[j] - h_grid[j] == 0.0, "pa_kde_gauss_f64: grid point %u is not finite", j);
  double range[2] = {0.0, 0.0};
  uint64_t valid = 0;
  PA_TRY(pa_minmax_f64(c, d_v, n, range, &valid));
  PA_REQUIRE(valid > 0, "pa_kde_gauss_f64: no value that is not NaN");
  PA_REQUIRE(range[0] - range[0] == 0.0 && range[1] - range[1] == 0.0, "pa_kde_gauss_f64: an infinite value among the data");
  uint32_t slices = 1;
  while (2 * slices * n_grid <= kKdeSlots) slices *= 2;
  const uint64_t per_wg = (uint64_t)kKdeChain * slices;
  const uint64_t rows64 = (n + per_wg - 1) / per_wg;
  PA_REQUIRE(rows64 < (1ULL << 31), "pa_kde_gauss_f64: %llu values", (unsigned long long)n);
  const uint32_t rows = (uint32_t)rows64;
  double *d_grid, *d_partial;
  PA_TRY(pa_carve(c->hist, "hist", [&](Carve &k) { d_grid = k.take<double>(n_grid); d_partial = k.take<double>((uint64_t)rows * n_grid); }));
  PA_HIP(hipMemcpyAsync(d_grid, h_grid, (uint64_t)n_grid * 8, hipMemcpyHostToDevice, c->stream));
  PA_TRY(PA_LAUNCH(c, dist_kde_kernel, rows, kThreads, 0, d_v, n, (const double *)d_grid, n_grid, slices, bw, d_partial));
  uint32_t top = 1;
  while (top < rows) top *= 2;
  for (uint32_t step = top / 2; step > 0; step /= 2)
    PA_TRY(PA_LAUNCH(c, dist_kde_fold_kernel, ceil_div((uint64_t)step * n_grid, (uint64_t)kThreads), kThreads, 0, d_partial, rows, step, n_grid));
  PA_TRY(pa_copy_to_host(c, h_density, d_partial, (uint64_t)n_grid * 8));
  const double norm = 1.0 / ((double)valid * bw * sqrt(2.0 * M_PI));
  for (uint32_t j = 0; j < n_grid; ++j) h_density[j] *= norm;
  return PA_OK;
}
