// hist.hip -- numpy's uniform-bin histogram of a vector on the device (gfx950, wave64), behind pa_hist_uniform_f64
// (plot-run-comp, the rug; up to 1024 bins) and pa_hist_uniform_f64_wide (plot-run's distributions; up to 2^20).
// DESIGN.md sections 7d and 7e have the definition and the measurements.
//
// The rule is numpy.histogram's (numpy/lib/_histograms_impl.py), stated in uniform_bins.h: the bin of v is
// ((v - first) / (last - first)) * bins truncated, with the three corrections against the edges.  The division is the
// IEEE one (v_div_scale / v_div_fmas / v_div_fixup, correctly rounded) and the product is rounded on its own:
// contraction is off for this file, by the pragma there and by the Makefile.  The edges are the caller's (numpy's
// linspace in the drivers).
//
// One kernel, a grid-stride pass of at most kStrideMaxBlocks workgroups, in three instantiations chosen by the number
// of bins:
//   up to 1024 bins: the edges staged in LDS, the counters of a workgroup u32 in LDS (a workgroup sees at most
//     n / 1024 + 256 values, and n < 2^40), added once to the u64 counters in global memory, which decides no position;
//   up to PA_HIST_WIDE_LDS_BINS bins: the same counters, the edges read from global memory;
//   above that: every value is one u64 integer atomic on the global counters.
// Counts are integers, so the three give the same bits, and so does the host twin (hist_host.cpp).  All loads are
// 8 bytes per lane: the callers pass slices of tensors, which promise no wider alignment.
#include "pa_internal.h"
#include "uniform_bins.h"

namespace {

constexpr int kThreads = kStrideThreads;
constexpr uint32_t kNarrowBins = 1024, kWideLdsBins = PA_HIST_WIDE_LDS_BINS, kWideMaxBins = 1u << 20;

// EDGE_BINS: the bins whose bins + 1 edges the workgroup stages in LDS; 0: the edges are read from global memory.
// COUNT_BINS: the bins a workgroup counts in u32 LDS counters; 0: u64 atomics on the global counters.
// bins <= EDGE_BINS and bins <= COUNT_BINS where they are not 0.
template <uint32_t EDGE_BINS, uint32_t COUNT_BINS>
__global__ __launch_bounds__(kThreads) void hist_uniform_kernel(const double *__restrict__ v, uint64_t n, const double *__restrict__ g_edges /*[bins + 1]*/,
                                                                uint32_t bins, unsigned long long *__restrict__ counts /*[bins]*/) {
  __shared__ double s_edges[EDGE_BINS ? EDGE_BINS + 1 : 1];
  __shared__ uint32_t s_counts[COUNT_BINS ? COUNT_BINS : 1];
  if (EDGE_BINS)
    for (uint32_t b = threadIdx.x; b <= bins; b += kThreads) s_edges[b] = g_edges[b];
  if (COUNT_BINS)
    for (uint32_t b = threadIdx.x; b < bins; b += kThreads) s_counts[b] = 0;
  if (EDGE_BINS || COUNT_BINS) __syncthreads();
  const double *edges = EDGE_BINS ? s_edges : g_edges;
  const double first = edges[0], last = edges[bins];
  const double span = last - first, nb = (double)bins;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
    const double x = v[i];
    if (x >= first && x <= last) {  // false for NaN
      const uint32_t b = pa_uniform_bin(x, first, span, nb, bins, edges);
      if (COUNT_BINS)
        atomicAdd(&s_counts[b], 1u);
      else
        atomicAdd(&counts[b], 1ULL);
    }
  }
  if (COUNT_BINS) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += kThreads)
      if (s_counts[b]) atomicAdd(&counts[b], (unsigned long long)s_counts[b]);
  }
}

// Both entry points: the checks (`who` begins their messages), the workspace in c->hist (the u64 counters, then the
// edges), the launch and the copy back.
int hist_uniform(pa_ctx *c, const char *who, uint32_t max_bins, const double *d_v, uint64_t n, const double *h_edges, uint32_t bins,
                 uint64_t *h_counts) {
  PA_REQUIRE(c != nullptr && h_edges != nullptr && h_counts != nullptr, "%s: null argument", who);
  PA_REQUIRE(bins >= 1 && bins <= max_bins, "%s: %u bins; 1 to %u", who, bins, max_bins);
  PA_REQUIRE(n < (1ULL << 40), "%s: %llu values; a workgroup's counters are 32-bit", who, (unsigned long long)n);
  PA_TRY(pa_check_uniform_edges(who, "", h_edges, bins));
  for (uint32_t b = 0; b < bins; ++b) h_counts[b] = 0;
  if (n == 0) return PA_OK;
  PA_REQUIRE(d_v != nullptr, "%s: null array", who);
  PA_HIP(hipSetDevice(c->device));
  unsigned long long *d_counts;
  double *d_edges;
  PA_TRY(pa_carve(c->hist, "hist", [&](Carve &k) { d_counts = k.take<unsigned long long>(bins); d_edges = k.take<double>((uint64_t)bins + 1); }));
  PA_HIP(hipMemsetAsync(d_counts, 0, (uint64_t)bins * 8, c->stream));
  PA_HIP(hipMemcpyAsync(d_edges, h_edges, ((uint64_t)bins + 1) * 8, hipMemcpyHostToDevice, c->stream));
  const uint32_t blocks = stride_blocks(n);
  if (bins <= kNarrowBins)
    PA_TRY(PA_LAUNCH(c, (hist_uniform_kernel<kNarrowBins, kNarrowBins>), blocks, kThreads, 0, d_v, n, (const double *)d_edges, bins, d_counts));
  else if (bins <= kWideLdsBins)
    PA_TRY(PA_LAUNCH(c, (hist_uniform_kernel<0, kWideLdsBins>), blocks, kThreads, 0, d_v, n, (const double *)d_edges, bins, d_counts));
  else
    PA_TRY(PA_LAUNCH(c, (hist_uniform_kernel<0, 0>), blocks, kThreads, 0, d_v, n, (const double *)d_edges, bins, d_counts));
  return pa_copy_to_host(c, h_counts, d_counts, (uint64_t)bins * 8);  // the caller's edges and counts are not touched after the return
}

}  // namespace

extern "C" int pa_hist_uniform_f64(pa_ctx *c, const double *d_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts) {
  return hist_uniform(c, "pa_hist_uniform_f64", kNarrowBins, d_v, n, h_edges, bins, h_counts);
}

extern "C" int pa_hist_uniform_f64_wide(pa_ctx *c, const double *d_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts) {
  return hist_uniform(c, "pa_hist_uniform_f64_wide", kWideMaxBins, d_v, n, h_edges, bins, h_counts);
}
