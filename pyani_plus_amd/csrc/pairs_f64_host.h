// pairs_f64_host.h -- the host twins' row loop of the all-pairs f64 row methods, stated once: one row against `count`
// consecutive rows, one accumulator per pair, acc = Term::add(acc, a[c], b[c]) over the columns c in ascending order.
// What pairs_f64_tile.h is on the device; pa_rowdist_euclid_host (linkage_host.cpp) and pa_tetra_corr_host
// (tetra_host.cpp) are its two users.  The terms are the kernels' (rowdist.hip's EuclidTerm, tetra.hip's DotTerm), each a
// rounded product and a rounded addition (strict_fp.h).
#ifndef PA_PAIRS_F64_HOST_H
#define PA_PAIRS_F64_HOST_H
#include <algorithm>
#include <cstdint>

#include "strict_fp.h"

namespace pairs_f64 {

struct EuclidTerm {
  static double add(double acc, double a, double b) { const double d = a - b, sq = d * d; return acc + sq; }
};
struct DotTerm {
  static double add(double acc, double a, double b) { const double p = a * b; return acc + p; }
};

// finish(u, acc) for u = 0 .. count - 1 with acc the sum of row a with row b0 + u * cols.  kSide pairs run side by side so
// that their dependent chains of additions overlap -- each chain keeps its own order.  The inner loop always runs kSide
// chains (a trip count the compiler knows: the accumulators stay in registers); a last group of fewer rows reads its last
// row in the spare chains, whose sums are dropped
template <class Term, class Finish>
inline void pair_row_accumulate(const double *a, const double *b0, uint32_t count, uint32_t cols, Finish &&finish) {
  constexpr uint32_t kSide = 8;
  for (uint32_t j = 0; j < count; j += kSide) {
    const uint32_t side = std::min(kSide, count - j);
    const double *b[kSide];
    for (uint32_t u = 0; u < kSide; ++u) b[u] = b0 + (uint64_t)(j + std::min(u, side - 1)) * cols;
    double acc[kSide] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t c = 0; c < cols; ++c) {
      const double ac = a[c];
      for (uint32_t u = 0; u < kSide; ++u) acc[u] = Term::add(acc[u], ac, b[u][c]);
    }
    for (uint32_t u = 0; u < side; ++u) finish(j + u, acc[u]);
  }
}

}  // namespace pairs_f64

#endif  // PA_PAIRS_F64_HOST_H
