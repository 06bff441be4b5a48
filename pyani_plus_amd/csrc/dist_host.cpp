// dist_host.cpp -- host twins of dist.hip: the order statistics, the moments and the Gaussian kernel density on a grid,
// as plain loops.  They are what plot-run's distributions use without a GPU and what the device kernels are compared
// with; the histogram's twin is hist_host.cpp.  The select gives the same values as the device; the moments and the
// density add in another order and agree within the bound of DESIGN.md section 7e.
// Built with -ffp-contract=off: the density's exponent is a rounded division, a rounded square and a halving.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "pa_host.h"
#include "strict_fp.h"

extern "C" {

int pa_select_f64_host(const double *h_v, uint64_t n, const uint64_t *h_ranks, uint32_t n_ranks, double *h_out) {
  if (n_ranks > PA_SELECT_MAX_RANKS) { pa_set_error("pa_select_f64_host: %u ranks; at most %u", n_ranks, PA_SELECT_MAX_RANKS); return PA_E_INVALID; }
  if (n_ranks == 0) return PA_OK;
  if (!h_ranks || !h_out || (n && !h_v)) { pa_set_error("pa_select_f64_host: null argument"); return PA_E_INVALID; }
  std::vector<double> valid;
  try {
    valid.reserve(n);
  } catch (const std::bad_alloc &) {
    pa_set_error("pa_select_f64_host: no memory for a copy of %llu values", (unsigned long long)n);
    return PA_E_NOMEM;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (h_v[i] == h_v[i]) valid.push_back(h_v[i]);
  for (uint32_t r = 0; r < n_ranks; ++r)
    if (h_ranks[r] >= valid.size()) {
      pa_set_error("pa_select_f64_host: rank %llu of %llu values that are not NaN", (unsigned long long)h_ranks[r], (unsigned long long)valid.size());
      return PA_E_INVALID;
    }
  for (uint32_t r = 0; r < n_ranks; ++r) {
    std::nth_element(valid.begin(), valid.begin() + (ptrdiff_t)h_ranks[r], valid.end());
    h_out[r] = valid[h_ranks[r]];
  }
  return PA_OK;
}

int pa_moments_f64_host(const double *h_v, uint64_t n, double *out) {
  if (!out || (n && !h_v)) { pa_set_error("pa_moments_f64_host: null argument"); return PA_E_INVALID; }
  double sum = 0.0;
  uint64_t valid = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (h_v[i] == h_v[i]) {
      sum += h_v[i];
      ++valid;
    }
  if (!valid) return PA_OK;
  const double mean = sum / (double)valid;
  double squares = 0.0;
  for (uint64_t i = 0; i < n; ++i)
    if (h_v[i] == h_v[i]) {
      const double d = h_v[i] - mean;
      squares += d * d;
    }
  out[0] = mean;
  out[1] = squares;
  return PA_OK;
}

int pa_kde_gauss_f64_host(const double *h_v, uint64_t n, const double *h_grid, uint32_t n_grid, double bw, double *h_density) {
  if (!h_grid || !h_density || (n && !h_v)) { pa_set_error("pa_kde_gauss_f64_host: null argument"); return PA_E_INVALID; }
  if (n_grid < 1 || n_grid > 1024) { pa_set_error("pa_kde_gauss_f64_host: %u grid points; 1 to 1024", n_grid); return PA_E_INVALID; }
  if (!(bw > 0.0) || !std::isfinite(bw)) { pa_set_error("pa_kde_gauss_f64_host: the bandwidth %g must be positive and finite", bw); return PA_E_INVALID; }
  for (uint32_t j = 0; j < n_grid; ++j)
    if (!std::isfinite(h_grid[j])) { pa_set_error("pa_kde_gauss_f64_host: grid point %u is not finite", j); return PA_E_INVALID; }
  uint64_t valid = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (std::isinf(h_v[i])) { pa_set_error("pa_kde_gauss_f64_host: an infinite value among the data"); return PA_E_INVALID; }
    valid += h_v[i] == h_v[i];
  }
  if (!valid) { pa_set_error("pa_kde_gauss_f64_host: no value that is not NaN"); return PA_E_INVALID; }
  const double norm = 1.0 / ((double)valid * bw * sqrt(2.0 * M_PI));
  for (uint32_t j = 0; j < n_grid; ++j) {
    // every term is a double, as in the definition; the sum is kept wider than a double where the platform has such a
    // type, so that what the device is compared with carries no summation error of its own to speak of
    long double sum = 0.0L;
    for (uint64_t i = 0; i < n; ++i) {
      if (h_v[i] != h_v[i]) continue;
      const double z = (h_grid[j] - h_v[i]) / bw;
      sum += (long double)exp(-0.5 * (z * z));
    }
    h_density[j] = (double)sum * norm;
  }
  return PA_OK;
}

}  // extern "C"
