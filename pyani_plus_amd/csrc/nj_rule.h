// nj_rule.h -- the arithmetic and the order of neighbour joining, stated once for nj.hip and nj_host.cpp (DESIGN.md
// section 7h has the contract; the check of D is distmat_rule.h's).  Every function is one line of the contract, each
// operation rounded on its own (strict_fp.h).
#pragma once

#include <cstdint>

#include "pa_hd.h"
#include "strict_fp.h"

namespace nj {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // the `lo` of a candidate that stands for no pair

// A live pair's score with the ids it is ordered by: lo < hi are node ids, never storage slots.
struct Cand {
  double q;
  uint32_t lo, hi;
};

// q = ((m - 2) d(lo, hi) - r[lo]) - r[hi]: the product rounded, then r of the smaller id, then r of the larger
PA_HD double score(double m_minus_2, double d, double r_lo, double r_hi) {
  const double p = m_minus_2 * d;
  const double s = p - r_lo;
  return s - r_hi;
}

// The total order of the choice: smaller q, then smaller lo, then smaller hi; == on doubles, so -0.0 ties with 0.0.
// No pair loses to any pair.  Total (for q that are not NaN), so the shape of a reduction does not show in its result.
PA_HD bool better(const Cand &x, const Cand &than) {
  if (x.lo == kNone) return false;
  if (than.lo == kNone) return true;
  if (x.q < than.q) return true;
  if (!(x.q == than.q)) return false;
  return x.lo < than.lo || (x.lo == than.lo && x.hi < than.hi);
}

// len_lo = 0.5 d + (r[lo] - r[hi]) / (2 (m - 2)); len_hi = d - len_lo
PA_HD double length_lo(double m_minus_2, double d, double r_lo, double r_hi) {
  const double half = 0.5 * d;
  const double diff = r_lo - r_hi;
  const double den = 2.0 * m_minus_2;
  return half + diff / den;
}

// d(u, k) = 0.5 ((d(lo, k) + d(hi, k)) - d)
PA_HD double joined_distance(double d_lo_k, double d_hi_k, double d) {
  const double s = d_lo_k + d_hi_k;
  return 0.5 * (s - d);
}

// r[k] = ((r[k] - d(lo, k)) - d(hi, k)) + d(u, k)
PA_HD double row_sum_after(double r_k, double d_lo_k, double d_hi_k, double d_u_k) {
  const double a = r_k - d_lo_k;
  const double b = a - d_hi_k;
  return b + d_u_k;
}

// r[u] = 0.5 ((r[lo] + r[hi]) - m d)
PA_HD double row_sum_joined(double m, double d, double r_lo, double r_hi) {
  const double s = r_lo + r_hi;
  const double p = m * d;
  return 0.5 * (s - p);
}

}  // namespace nj
