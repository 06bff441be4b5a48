// pair_rule.h -- the aggregate of a pair's two cells of a run's matrix, stated once for classify and dereplicate-run,
// device and host (DESIGN.md sections 7b and 7k).  The mean is one rounded addition and one division on both sides
// (strict_fp.h).
#pragma once

#include <cstdint>

#include "../../include/pyani_hip.h"
#include "pa_hd.h"
#include "strict_fp.h"

namespace pair_rule {

PA_HD bool agg_ok(int how) { return how == PA_AGG_MIN || how == PA_AGG_MAX || how == PA_AGG_MEAN; }

// Python's min([a, b]), max([a, b]) and numpy.mean([a, b]) with a = M[hi,lo], b = M[lo,hi].  The built-ins keep the
// first argument unless the comparison with the second holds, so a NaN in a stays and a NaN in b is passed over.
PA_HD double agg2(int how, double a, double b) {
  if (how == PA_AGG_MIN) return b < a ? b : a;
  if (how == PA_AGG_MAX) return b > a ? b : a;
  const double s = a + b;
  return s / 2.0;
}

// The aggregated value of the pair (p, q) from its two cells: the cell of the larger index as the row comes first.
// p == q is the pair (p, p) by the same formula.
PA_HD double pair_value(int how, uint32_t p, uint32_t q, double m_pq, double m_qp) {
  return p < q ? agg2(how, m_qp, m_pq) : agg2(how, m_pq, m_qp);
}

}  // namespace pair_rule
