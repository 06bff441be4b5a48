// scatter.hip -- plot-run's scatter figures on the device (gfx950, wave64): a 2-D binning of N^2 points (x, y) into up
// to 1024 x 1024 cells that keeps, per cell, the number of points and the index of the last one.  DESIGN.md section
// 7f has the definition and the measurements.
//
// pa_bin2d_f64: point t counts iff x[t] and y[t] lie within their edges (NaN does not); its bin on each axis is
// pa_hist_uniform_f64's (uniform_bins.h; contraction is off for this file, by the pragma there and by the Makefile);
// its cell is ix * bins_y + iy.  A cell holds two u32 words in two arrays, `count` and `last + 1` (0: no point), and
// not one packed u64: the count is a sum and the index a maximum, which one 64-bit atomic cannot do together, and the
// 32-bit LDS atomics are the native ones.  n < 2^32 - 1, so both fit; the host widens them to u64.
//
// One grid-stride pass, at most kStrideMaxBlocks workgroups of 256 lanes, 8-byte loads (the callers pass slices of tensors),
// both edge arrays staged in LDS.  ANI points are as contended as points get -- the self comparisons all sit on
// (1, 1), a species cluster fills a handful of cells -- so three things keep a point off the global atomics:
//   1. the wave peels its leading cell: the lanes whose cell is that of the wave's first valid lane are counted with
//      one ballot, and the highest of them (which holds the largest t: t ascends with the lane) carries their number.
//      A wave whose points share a cell issues one update, not 64 to one address.
//   2. small grids (cells <= PA_BIN2D_LDS_CELLS): the workgroup keeps both words of every cell in LDS (atomicAdd,
//      atomicMax) and adds the non-empty ones to global memory once, at its end.
//   3. larger grids: a direct-mapped cache of PA_BIN2D_SLOTS slots in LDS, each {cell + 1, count, last + 1}.  The slot
//      of a cell is cell % PA_BIN2D_SLOTS.  A lane claims an empty slot with a compare-and-swap on the key; it
//      accumulates there if the slot is, or thereby becomes, its cell's, and goes to the global atomics if another cell
//      owns the slot.  A slot never changes owner; the workgroup flushes the owned slots at its end.
// Which lane wins a slot changes where a point is added up, never what: sums and maxima of integers are order-free, so
// the result has the same bits run to run and is the host twin's.  No floating-point atomics; one host synchronisation.
#include <vector>

#include "pa_internal.h"
#include "uniform_bins.h"

namespace {

constexpr int kThreads = kStrideThreads;
constexpr uint32_t kLdsCells = PA_BIN2D_LDS_CELLS;
constexpr uint32_t kSlots = PA_BIN2D_SLOTS;
static_assert((kSlots & (kSlots - 1)) == 0, "the slot of a cell is taken with a mask");
// dynamic LDS: the edges (at most 2 x 1025 doubles) and the larger of the two regimes' words, inside the 64 KB a launch
// gets without asking
static_assert(2 * (PA_BIN2D_MAX_BINS + 1) * 8 + 3 * kSlots * 4 <= 65536 && 2 * (PA_BIN2D_MAX_BINS + 1) * 8 + 2 * kLdsCells * 4 <= 65536,
              "the workgroup's LDS");

inline size_t lds_bytes(uint32_t bins_x, uint32_t bins_y, bool full) {
  return ((size_t)bins_x + bins_y + 2) * 8 + (full ? 2 * (size_t)bins_x * bins_y : 3 * (size_t)kSlots) * 4;
}

// FULL: every cell in LDS.  Otherwise the direct-mapped cache.
template <bool FULL>
__global__ __launch_bounds__(kThreads) void bin2d_kernel(const double *__restrict__ x, const double *__restrict__ y, uint32_t n,
                                                         const double *__restrict__ edges /*[bins_x + 1] then [bins_y + 1]*/, uint32_t bins_x,
                                                         uint32_t bins_y, uint32_t *__restrict__ g_count /*[cells]*/,
                                                         uint32_t *__restrict__ g_last /*[cells]: last + 1*/) {
  extern __shared__ double s_mem[];
  double *s_xe = s_mem, *s_ye = s_mem + bins_x + 1;
  uint32_t *s_words = reinterpret_cast<uint32_t *>(s_ye + bins_y + 1);
  const uint32_t cells = bins_x * bins_y;
  const uint32_t held = FULL ? cells : kSlots;  // cells or slots in LDS
  uint32_t *s_count = s_words, *s_last = s_words + held, *s_key = s_words + 2 * held;  // s_key: the cache alone
  for (uint32_t b = threadIdx.x; b < bins_x + bins_y + 2; b += kThreads) s_mem[b] = edges[b];
  for (uint32_t b = threadIdx.x; b < (FULL ? 2u : 3u) * held; b += kThreads) s_words[b] = 0;
  __syncthreads();
  const double x0 = s_xe[0], x1 = s_xe[bins_x], y0 = s_ye[0], y1 = s_ye[bins_y];
  const double xspan = x1 - x0, yspan = y1 - y0, xnb = (double)bins_x, ynb = (double)bins_y;
  const uint32_t lane = threadIdx.x & 63u;
  // the bound is the workgroup's: every lane of a wave takes part in the ballots of every round
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n; base += (uint64_t)gridDim.x * kThreads) {
    const uint64_t t = base + threadIdx.x;
    bool in = false;
    uint32_t cell = 0;
    if (t < n) {
      const double px = x[t], py = y[t];
      if (px >= x0 && px <= x1 && py >= y0 && py <= y1) {  // false for NaN
        in = true;
        cell = pa_uniform_bin(px, x0, xspan, xnb, bins_x, s_xe) * bins_y + pa_uniform_bin(py, y0, yspan, ynb, bins_y, s_ye);
      }
    }
    const uint64_t live = __ballot(in);
    if (live == 0) continue;  // uniform in the wave
    uint32_t add = 1;
    const uint32_t lead = (uint32_t)__shfl((int)cell, __ffsll((unsigned long long)live) - 1);
    const uint64_t same = __ballot(in && cell == lead);
    if (in && cell == lead) {
      if (lane == 63u - (uint32_t)__clzll((long long)same))
        add = (uint32_t)__popcll(same);
      else
        in = false;  // counted by the highest lane of its cell, whose t is larger
    }
    if (!in) continue;
    const uint32_t t1 = (uint32_t)t + 1u;  // n < 2^32 - 1
    if (FULL) {
      atomicAdd(&s_count[cell], add);
      atomicMax(&s_last[cell], t1);
    } else {
      const uint32_t slot = cell & (kSlots - 1), key = cell + 1u;
      uint32_t owner = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (owner == 0) {
        owner = atomicCAS(&s_key[slot], 0u, key);
        if (owner == 0) owner = key;
      }
      if (owner == key) {
        atomicAdd(&s_count[slot], add);
        atomicMax(&s_last[slot], t1);
      } else {
        atomicAdd(&g_count[cell], add);
        atomicMax(&g_last[cell], t1);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < held; b += kThreads) {
    const uint32_t have = s_count[b];
    if (have) {
      const uint32_t cell = FULL ? b : s_key[b] - 1u;  // a slot with a count has an owner
      atomicAdd(&g_count[cell], have);
      atomicMax(&g_last[cell], s_last[b]);
    }
  }
}

}  // namespace

extern "C" int pa_bin2d_f64(pa_ctx *c, const double *d_x, const double *d_y, uint64_t n, const double *h_xedges, uint32_t bins_x,
                            const double *h_yedges, uint32_t bins_y, uint64_t *h_counts, uint64_t *h_last) {
  PA_REQUIRE(c != nullptr, "pa_bin2d_f64: null argument");
  PA_TRY(pa_bin2d_validate("pa_bin2d_f64", d_x, d_y, n, h_xedges, bins_x, h_yedges, bins_y, h_counts, h_last));
  const uint32_t cells = bins_x * bins_y;  // <= 2^20
  for (uint32_t k = 0; k < cells; ++k) {
    h_counts[k] = 0;
    h_last[k] = PA_BIN2D_NONE;
  }
  if (n == 0) return PA_OK;
  PA_HIP(hipSetDevice(c->device));
  const uint32_t n_edges = bins_x + bins_y + 2;
  double *d_edges;
  uint32_t *d_count, *d_last;  // one memset and one copy span both
  PA_TRY(pa_carve(c->bin2d, "bin2d", [&](Carve &k) { d_edges = k.take<double>(n_edges); d_count = k.take<uint32_t>(cells); d_last = k.take<uint32_t>(cells); }));
  PA_HIP(hipMemsetAsync(d_count, 0, 2 * (uint64_t)cells * 4, c->stream));
  PA_HIP(hipMemcpyAsync(d_edges, h_xedges, ((uint64_t)bins_x + 1) * 8, hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipMemcpyAsync(d_edges + bins_x + 1, h_yedges, ((uint64_t)bins_y + 1) * 8, hipMemcpyHostToDevice, c->stream));
  const bool full = cells <= kLdsCells;
  if (full)
    PA_TRY(PA_LAUNCH(c, bin2d_kernel<true>, stride_blocks(n), kThreads, lds_bytes(bins_x, bins_y, true), d_x, d_y, (uint32_t)n,
                     (const double *)d_edges, bins_x, bins_y, d_count, d_last));
  else
    PA_TRY(PA_LAUNCH(c, bin2d_kernel<false>, stride_blocks(n), kThreads, lds_bytes(bins_x, bins_y, false), d_x, d_y, (uint32_t)n,
                     (const double *)d_edges, bins_x, bins_y, d_count, d_last));
  std::vector<uint32_t> words(2 * (size_t)cells);
  PA_TRY(pa_copy_to_host(c, words.data(), d_count, 2 * (uint64_t)cells * 4));  // the call's one wait; the caller's edges are not read after it
  for (uint32_t k = 0; k < cells; ++k) {
    h_counts[k] = words[k];
    if (words[cells + k]) h_last[k] = (uint64_t)words[cells + k] - 1;
  }
  return PA_OK;
}
