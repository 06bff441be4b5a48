// uniform_bins.h -- numpy's uniform-bin rule, stated once for every histogram of the library: the bin of a value among
// uniform edges (device and host: hist.hip, scatter.hip, hist_host.cpp, scatter_host.cpp), the check of an edge array
// that the 1-D and the 2-D entry points share, and the argument check of pa_bin2d_f64 and pa_bin2d_f64_host.
// The bin index is a rounded division, then a rounded multiplication, and must not become a fused one (strict_fp.h).
#ifndef PA_UNIFORM_BINS_H
#define PA_UNIFORM_BINS_H
#include <cstdint>

#include "pa_hd.h"
#include "strict_fp.h"

// The bin of x among `bins` uniform bins with these bins + 1 edges; the caller has checked first <= x <= last, where
// first = edges[0], last = edges[bins], span = last - first and nb = (double)bins.  numpy/lib/_histograms_impl.py, the
// uniform-bins branch.
PA_HD uint32_t pa_uniform_bin(double x, double first, double span, double nb, uint32_t bins, const double *edges) {
  const double t = (x - first) / span;  // in [0, 1]: both differences are rounded the same way
  uint32_t b = (uint32_t)(t * nb);      // in [0, bins]
  if (b >= bins) b = bins - 1;          // the last edge belongs to the last bin
  if (x < edges[b]) --b;                // never at b = 0: x >= first
  if (x >= edges[b + 1] && b != bins - 1) ++b;
  return b;
}

// PA_OK, or PA_E_INVALID with the message set: one of the bins + 1 edges is infinite or NaN or lies below the one
// before it, or the last edge is not above the first by a finite difference.  `who` names the entry point and `axis` is
// "", "x " or "y ".  hist_host.cpp
int pa_check_uniform_edges(const char *who, const char *axis, const double *edges, uint32_t bins);

// PA_OK, or PA_E_INVALID with the message set (`who` names the entry point): a null argument, bins outside
// 1 .. PA_BIN2D_MAX_BINS on either axis, n >= 2^32 - 1, and the edge errors above with the axis named.
// Reads the edges and nothing else.  scatter_host.cpp
int pa_bin2d_validate(const char *who, const void *x, const void *y, uint64_t n, const double *h_xedges, uint32_t bins_x,
                      const double *h_yedges, uint32_t bins_y, const uint64_t *h_counts, const uint64_t *h_last);

#endif  // PA_UNIFORM_BINS_H
