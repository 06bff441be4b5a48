// hist_host.cpp -- host twin of hist.hip: numpy's uniform-bin histogram as one plain loop over pa_uniform_bin
// (uniform_bins.h), exported under the names of its two device entry points, and the check of an edge array that every
// entry point with edges shares.  It is what plot-run-comp and plot-run's distributions use without a GPU and what the
// device kernel is compared with: counts of integers, so the two give the same bits.
// Built with -ffp-contract=off: the bin index is a rounded division followed by a rounded multiplication.
#include <cmath>
#include <cstdint>

#include "pa_host.h"
#include "uniform_bins.h"

int pa_check_uniform_edges(const char *who, const char *axis, const double *e, uint32_t bins) {
  for (uint32_t b = 0; b <= bins; ++b) {
    if (!std::isfinite(e[b])) { pa_set_error("%s: %sedge %u is not finite", who, axis, b); return PA_E_INVALID; }
    if (b && e[b - 1] > e[b]) { pa_set_error("%s: %sedge %u is below edge %u", who, axis, b, b - 1); return PA_E_INVALID; }
  }
  const double span = e[bins] - e[0];
  if (!(span > 0.0) || !std::isfinite(span)) {
    pa_set_error("%s: the last %sedge must be above the first and their difference finite", who, axis);
    return PA_E_INVALID;
  }
  return PA_OK;
}

namespace {

int hist_uniform_host(const char *who, uint32_t max_bins, const double *h_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts) {
  if (!h_edges || !h_counts || (n && !h_v)) { pa_set_error("%s: null argument", who); return PA_E_INVALID; }
  if (bins < 1 || bins > max_bins) { pa_set_error("%s: %u bins; 1 to %u", who, bins, max_bins); return PA_E_INVALID; }
  if (int s = pa_check_uniform_edges(who, "", h_edges, bins)) return s;
  const double first = h_edges[0], last = h_edges[bins];
  const double span = last - first, nb = (double)bins;
  for (uint32_t b = 0; b < bins; ++b) h_counts[b] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const double x = h_v[i];
    if (!(x >= first && x <= last)) continue;  // NaN too
    ++h_counts[pa_uniform_bin(x, first, span, nb, bins, h_edges)];
  }
  return PA_OK;
}

}  // namespace

extern "C" int pa_hist_uniform_f64_host(const double *h_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts) {
  return hist_uniform_host("pa_hist_uniform_f64_host", 1024, h_v, n, h_edges, bins, h_counts);
}

extern "C" int pa_hist_uniform_f64_wide_host(const double *h_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts) {
  return hist_uniform_host("pa_hist_uniform_f64_wide_host", 1u << 28, h_v, n, h_edges, bins, h_counts);
}
