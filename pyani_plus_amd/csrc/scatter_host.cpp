// scatter_host.cpp -- host twin of scatter.hip: the 2-D binning behind plot-run's scatter figures as one plain loop,
// and the argument check the two entry points share.  It is what plot-run --scatter uses without a GPU and what the
// device kernel is compared with: counts and maxima of integers, so the two give the same bits.
// Built with -ffp-contract=off: the bin index is a rounded division followed by a rounded multiplication.
#include <cmath>
#include <cstdint>

#include "pa_host.h"
#include "uniform_bins.h"

int pa_bin2d_validate(const char *who, const void *x, const void *y, uint64_t n, const double *h_xedges, uint32_t bins_x,
                      const double *h_yedges, uint32_t bins_y, const uint64_t *h_counts, const uint64_t *h_last) {
  if (!h_xedges || !h_yedges || !h_counts || !h_last || (n && (!x || !y))) { pa_set_error("%s: null argument", who); return PA_E_INVALID; }
  if (bins_x < 1 || bins_x > PA_BIN2D_MAX_BINS) { pa_set_error("%s: %u x bins; 1 to %u", who, bins_x, PA_BIN2D_MAX_BINS); return PA_E_INVALID; }
  if (bins_y < 1 || bins_y > PA_BIN2D_MAX_BINS) { pa_set_error("%s: %u y bins; 1 to %u", who, bins_y, PA_BIN2D_MAX_BINS); return PA_E_INVALID; }
  if (n >= 0xFFFFFFFFULL) { pa_set_error("%s: %llu points; at most 2^32 - 2 (a cell holds the index of its last point in 32 bits)", who, (unsigned long long)n); return PA_E_INVALID; }
  if (int s = pa_check_uniform_edges(who, "x ", h_xedges, bins_x)) return s;
  return pa_check_uniform_edges(who, "y ", h_yedges, bins_y);
}

extern "C" int pa_bin2d_f64_host(const double *h_x, const double *h_y, uint64_t n, const double *h_xedges, uint32_t bins_x, const double *h_yedges,
                                 uint32_t bins_y, uint64_t *h_counts, uint64_t *h_last) {
  if (int s = pa_bin2d_validate("pa_bin2d_f64_host", h_x, h_y, n, h_xedges, bins_x, h_yedges, bins_y, h_counts, h_last)) return s;
  const uint64_t cells = (uint64_t)bins_x * bins_y;
  for (uint64_t c = 0; c < cells; ++c) {
    h_counts[c] = 0;
    h_last[c] = PA_BIN2D_NONE;
  }
  const double x0 = h_xedges[0], x1 = h_xedges[bins_x], y0 = h_yedges[0], y1 = h_yedges[bins_y];
  const double xspan = x1 - x0, yspan = y1 - y0, xnb = (double)bins_x, ynb = (double)bins_y;
  for (uint64_t t = 0; t < n; ++t) {
    const double x = h_x[t], y = h_y[t];
    if (!(x >= x0 && x <= x1 && y >= y0 && y <= y1)) continue;  // NaN too
    const uint64_t cell = (uint64_t)pa_uniform_bin(x, x0, xspan, xnb, bins_x, h_xedges) * bins_y + pa_uniform_bin(y, y0, yspan, ynb, bins_y, h_yedges);
    ++h_counts[cell];
    h_last[cell] = t;  // t ascends: the last one written is the largest
  }
  return PA_OK;
}
