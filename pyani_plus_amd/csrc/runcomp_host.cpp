// runcomp_host.cpp -- host twins of runcomp.hip: the join of two runs and the minimum and maximum of a vector, as plain
// loops with the same results bit for bit.  They are what plot-run-comp uses without a GPU and what the device kernels
// are compared with; the histogram's twin is hist_host.cpp.  Built with -ffp-contract=off, as runcomp.hip is: the
// join's y - x stays a difference of its own on both sides.
#include <cmath>
#include <cstdint>

#include "pa_host.h"
#include "strict_fp.h"

extern "C" {

int pa_runcomp_join_host(const double *h_ref, uint32_t n_ref, const uint32_t *h_q, const uint32_t *h_s, const double *h_y, uint64_t n_rows,
                         double *h_x, double *h_y_out, double *h_diff, uint64_t *n_common) {
  if (!n_common) { pa_set_error("pa_runcomp_join_host: null argument"); return PA_E_INVALID; }
  if (n_ref > (1u << 16)) { pa_set_error("pa_runcomp_join_host: %u genomes in the reference run; at most 65536", n_ref); return PA_E_INVALID; }
  if (n_rows >= (1ULL << 32)) { pa_set_error("pa_runcomp_join_host: %llu rows; at most 2^32 - 1", (unsigned long long)n_rows); return PA_E_INVALID; }
  *n_common = 0;
  if (n_rows == 0) return PA_OK;
  if (!h_q || !h_s || !h_y || !h_x || !h_y_out || !h_diff || (n_ref && !h_ref)) { pa_set_error("pa_runcomp_join_host: null array"); return PA_E_INVALID; }
  uint64_t at = 0;
  for (uint64_t r = 0; r < n_rows; ++r) {
    const uint32_t q = h_q[r], s = h_s[r];
    const double y = h_y[r];
    if (q >= n_ref || s >= n_ref || y != y) continue;
    const double x = h_ref[(uint64_t)q * n_ref + s];
    if (x != x) continue;
    h_x[at] = x;
    h_y_out[at] = y;
    h_diff[at] = y - x;
    ++at;
  }
  *n_common = at;
  return PA_OK;
}

int pa_minmax_f64_host(const double *h_v, uint64_t n, double *out, uint64_t *n_valid) {
  if (!out || !n_valid || (n && !h_v)) { pa_set_error("pa_minmax_f64_host: null argument"); return PA_E_INVALID; }
  double lo = INFINITY, hi = -INFINITY;
  uint64_t valid = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const double x = h_v[i];
    if (x != x) continue;
    lo = x < lo ? x : lo;
    hi = x > hi ? x : hi;
    ++valid;
  }
  *n_valid = valid;
  if (valid) {
    out[0] = lo;
    out[1] = hi;
  }
  return PA_OK;
}

}  // extern "C"
