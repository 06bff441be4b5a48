// runcomp.hip -- plot-run-comp on the device (gfx950, wave64): two runs joined pair by pair and the minimum and maximum
// of a vector.  The histograms of the joined values are hist.hip's.
//
// The reference keeps one Python dictionary per run, keyed by (query_hash, subject_hash) tuples, looks every pair of
// the other run up in the reference run's dictionary and hands the joined lists to Axes.hist
// (pyani_plus/plot_run.py:404-575).  Here the reference run R is its n_ref x n_ref identity matrix (NaN: no value) and
// the other run O is three arrays in database order: the row and the column of each of its comparisons in R's matrix,
// and its own identity.  The join is then a gather and a stream compaction, and the histograms are reductions.
// DESIGN.md section 7d has the definition and the measurements.  Contraction is off for this file, by strict_fp.h below
// and by the Makefile, as it is for the host twin.
//
// pa_runcomp_join, the shape of classify.hip:
//   1. rc_join_kernel<false>: a lane per row.  A row survives iff q < n_ref, s < n_ref, y is not NaN and ref[q, s] is
//      not NaN; the indices are checked before the cell is read, and the cell index q * n_ref + s is 64-bit.  Each
//      wave counts the survivors of its 64 consecutive rows with one ballot and writes the count of that group.
//   2. pa_exclusive_scan_u32 over the group counts, which lie in row order: the offset of a group is the number of
//      survivors before it.  The total is read back by the same call, pa_scan_total_u32: the call's only host
//      synchronisation.
//   3. rc_join_kernel<true>: the same evaluation again; a surviving lane writes x = ref[q, s], y and d = y - x at
//      offset + popcount(ballot below the lane).  The output is therefore dense and in input order, and no atomic
//      decides a position.
//
// Rows per workgroup: T = 1024 (256 threads, four 64-row groups per wave).  In iteration k the workgroup takes the 256
// consecutive rows base + 256 k ..., so q, s and y are read coalesced, and the four iterations are unrolled with the
// loads first: a lane has four independent gathers in flight, which is what there is to hide the latency of a cell
// that misses the caches.  More rows per workgroup would only add registers; at 10^8 rows T = 1024 is 97 657
// workgroups, far more than the 256 CUs hold at once, so the tail is short.
//
// The ref gather is the random-access part, and what it costs depends on O's order.  O's rows usually come in the
// order a run was written, over the same sorted genomes as R: row by row (q fixed over n consecutive rows, s
// ascending) the 64 lanes of a wave read 512 contiguous bytes, the same as a stream; column by column (s fixed, q
// ascending) every lane reads its own cache line, n_ref * 8 bytes from its neighbour's, and that line is used again
// only n rows later by the next column, so the reuse needs n_ref lines to stay cached between two columns (1.3 MB of
// 128-byte lines at n_ref = 10^4).  A run over other genomes or in another order is a random gather from an
// 8 n_ref^2 byte table: 8 MB at n_ref = 1000, 800 MB (beyond every cache) at n_ref = 10^4.  Nothing about the cache
// behaviour of any of these has been measured; tools/runcomp_bench.py times whole calls only.
//
// pa_minmax_f64: a grid-stride pass, at most 1024 workgroups, each reduces its share through LDS to one (min, max,
// count) triple; a one-workgroup second pass reduces the triples.  No atomics; values are compared as values.
#include <cstring>

#include "block_reduce_dev.h"
#include "pa_internal.h"
#include "strict_fp.h"

namespace {

constexpr int kThreads = kStrideThreads;
constexpr int kGroups = 4;                                      // 64-row groups per wave
constexpr uint32_t kRowsPerWg = (uint32_t)kThreads * kGroups;  // T
constexpr uint32_t kNone = 0xFFFFFFFFu;

template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void rc_join_kernel(const double *__restrict__ ref, uint32_t n_ref, const uint32_t *__restrict__ q,
                                                           const uint32_t *__restrict__ s, const double *__restrict__ y, uint64_t n_rows,
                                                           uint32_t *__restrict__ counts /*per 64 rows: counts out, or offsets in*/,
                                                           uint64_t n_common, double *__restrict__ o_x, double *__restrict__ o_y,
                                                           double *__restrict__ o_d) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kRowsPerWg;
  const double nan = __builtin_nan("");
  uint32_t qi[kGroups], si[kGroups];
  double yv[kGroups], xv[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const uint64_t r = base + (uint64_t)k * kThreads + threadIdx.x;
    const bool in = r < n_rows;
    qi[k] = in ? q[r] : kNone;
    si[k] = in ? s[r] : kNone;
    yv[k] = in ? y[r] : nan;
  }
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const bool ok = qi[k] < n_ref && si[k] < n_ref && yv[k] == yv[k];
    xv[k] = ok ? ref[(uint64_t)qi[k] * n_ref + si[k]] : nan;
  }
  const uint64_t below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const uint64_t g = (uint64_t)blockIdx.x * (kRowsPerWg / 64) + (uint64_t)k * (kThreads / 64) + wave;  // rows 64 g .. 64 g + 63
    if (g * 64 >= n_rows) break;  // uniform in the wave; the groups of later k lie further on
    const bool keep = xv[k] == xv[k];  // NaN also where an index or y ruled the row out
    const uint64_t mask = __ballot(keep);
    if (!SCATTER) {
      if (lane == 0) counts[g] = (uint32_t)__popcll(mask);
    } else if (keep) {
      const uint64_t at = (uint64_t)counts[g] + __popcll(mask & below);
      if (at < n_common) {  // always: the offsets are the scan of the counts of the same evaluation
        o_x[at] = xv[k];
        o_y[at] = yv[k];
        o_d[at] = yv[k] - xv[k];
      }
    }
  }
}

// (min, max, count) of the non-NaN values seen so far; the identities compare correctly with every value
struct MinMax {
  double lo, hi;
  unsigned long long cnt;
};
__device__ __forceinline__ MinMax block_minmax(MinMax mine, MinMax *s) {
  return pa_dev::block_reduce<kThreads>(mine, s, [](MinMax a, MinMax b) {
    return MinMax{b.lo < a.lo ? b.lo : a.lo, b.hi > a.hi ? b.hi : a.hi, a.cnt + b.cnt};
  });
}

// partial[3 b .. 3 b + 2] = min, max and (as its bits) the count of the non-NaN values of workgroup b's share
__global__ __launch_bounds__(kThreads) void rc_minmax_kernel(const double *__restrict__ v, uint64_t n, double *__restrict__ partial) {
  __shared__ MinMax s_mm[kThreads];
  double lo = __builtin_inf(), hi = -__builtin_inf();
  unsigned long long cnt = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
    const double x = v[i];
    if (x == x) {
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
      ++cnt;
    }
  }
  const MinMax all = block_minmax(MinMax{lo, hi, cnt}, s_mm);
  if (threadIdx.x == 0) {
    partial[3 * (uint64_t)blockIdx.x] = all.lo;
    partial[3 * (uint64_t)blockIdx.x + 1] = all.hi;
    partial[3 * (uint64_t)blockIdx.x + 2] = __longlong_as_double((long long)all.cnt);
  }
}

// one workgroup: the n_partial triples -> result[0 .. 2] (min, max, the count's bits)
__global__ __launch_bounds__(kThreads) void rc_minmax_final_kernel(const double *__restrict__ partial, uint32_t n_partial,
                                                                  double *__restrict__ result) {
  __shared__ MinMax s_mm[kThreads];
  double lo = __builtin_inf(), hi = -__builtin_inf();
  unsigned long long cnt = 0;
  for (uint32_t b = threadIdx.x; b < n_partial; b += kThreads) {
    const unsigned long long c = (unsigned long long)__double_as_longlong(partial[3 * (uint64_t)b + 2]);
    if (c) {  // an empty share holds the identities, which compare correctly, but skip them all the same
      const double a = partial[3 * (uint64_t)b], z = partial[3 * (uint64_t)b + 1];
      lo = a < lo ? a : lo;
      hi = z > hi ? z : hi;
      cnt += c;
    }
  }
  const MinMax all = block_minmax(MinMax{lo, hi, cnt}, s_mm);
  if (threadIdx.x == 0) {
    result[0] = all.lo;
    result[1] = all.hi;
    result[2] = __longlong_as_double((long long)all.cnt);
  }
}

}  // namespace

extern "C" int pa_runcomp_join(pa_ctx *c, const double *d_ref, uint32_t n_ref, const uint32_t *d_q, const uint32_t *d_s, const double *d_y,
                               uint64_t n_rows, double *d_x, double *d_y_out, double *d_diff, uint64_t *n_common) {
  PA_REQUIRE(c != nullptr && n_common != nullptr, "pa_runcomp_join: null argument");
  PA_REQUIRE(n_ref <= (1u << 16), "pa_runcomp_join: %u genomes in the reference run; at most 65536", n_ref);
  // the offsets of the compaction are 32-bit
  PA_REQUIRE(n_rows < (1ULL << 32), "pa_runcomp_join: %llu rows; at most 2^32 - 1", (unsigned long long)n_rows);
  *n_common = 0;
  if (n_rows == 0) return PA_OK;
  PA_REQUIRE(d_q && d_s && d_y && d_x && d_y_out && d_diff && (n_ref == 0 || d_ref), "pa_runcomp_join: null array");
  PA_HIP(hipSetDevice(c->device));
  const uint64_t n_groups = (n_rows + 63) / 64;
  PA_TRY(c->flags.reserve(n_groups * sizeof(uint32_t)));
  uint32_t *d_counts = c->flags.as<uint32_t>();
  const uint64_t grid = ceil_div(n_rows, kRowsPerWg);
  PA_TRY(PA_LAUNCH(c, rc_join_kernel<false>, grid, kThreads, 0, d_ref, n_ref, d_q, d_s, d_y, n_rows, d_counts, 0ULL, nullptr, nullptr, nullptr));
  uint64_t total = 0;
  PA_TRY(pa_scan_total_u32(c, d_counts, d_counts, n_groups, c->slot<uint64_t>(kCompactTotal), &total));
  *n_common = total;
  if (total == 0) return PA_OK;
  return PA_LAUNCH(c, rc_join_kernel<true>, grid, kThreads, 0, d_ref, n_ref, d_q, d_s, d_y, n_rows, d_counts, total, d_x, d_y_out, d_diff);
}

extern "C" int pa_minmax_f64(pa_ctx *c, const double *d_v, uint64_t n, double *out, uint64_t *n_valid) {
  PA_REQUIRE(c != nullptr && out != nullptr && n_valid != nullptr, "pa_minmax_f64: null argument");
  *n_valid = 0;
  if (n == 0) return PA_OK;
  PA_REQUIRE(d_v != nullptr, "pa_minmax_f64: null array");
  PA_HIP(hipSetDevice(c->device));
  const uint32_t blocks = stride_blocks(n);
  double *d_partial, *d_result;
  PA_TRY(pa_carve(c->hist, "hist", [&](Carve &k) { d_partial = k.take<double>(3 * (uint64_t)blocks); d_result = k.take<double>(3); }));
  PA_TRY(PA_LAUNCH(c, rc_minmax_kernel, blocks, kThreads, 0, d_v, n, d_partial));
  PA_TRY(PA_LAUNCH(c, rc_minmax_final_kernel, 1, kThreads, 0, d_partial, blocks, d_result));
  double result[3];  // min, max, the count's bits
  PA_TRY(pa_read_back(c, d_result, result, 3));
  uint64_t valid;
  memcpy(&valid, &result[2], sizeof valid);
  *n_valid = valid;
  if (valid) {
    out[0] = result[0];
    out[1] = result[1];
  }
  return PA_OK;
}
