// mantel_rule.h -- the constants, the arithmetic and the argument checks of mantel-run-comp, stated once for mantel.hip
// and mantel_host.cpp (DESIGN.md section 7j has the contract).  Every function is one line of the contract, each
// operation rounded on its own (strict_fp.h).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/pyani_hip.h"
#include "pa_hd.h"
#include "strict_fp.h"

namespace mantel {

// A row's terms go to kLanes accumulators, term j to accumulator j % kLanes in ascending j; the accumulators are then
// added as a tree: for w = 32, 16, 8, 4, 2, 1, a[l] = a[l] + a[l + w] for l < w.  The row's sum is a[0].
constexpr uint32_t kLanes = PA_MANTEL_LANES;
static_assert(kLanes == 64, "the tree starts at w = 32; on the device an accumulator is a lane of a wave");

// Every accumulator and every chain starts here: -0.0 + x is x for every x, signed zeros included, so the first term
// enters unchanged and an accumulator without terms stays -0.0.
constexpr double kSumStart = -0.0;

// The splitmix64 finaliser (the one pcoa_rule.h's start_value uses), mod 2^64
PA_HD uint64_t fin(uint64_t v) {
  uint64_t z = v + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// x[i, j] = X[i, j] - mean_x for i != j
PA_HD double centred(double v, double mean) { return v - mean; }

// One more term of an accumulator: the term rounded, then the addition
PA_HD double add_square(double acc, double x) {
  const double t = x * x;
  return acc + t;
}
PA_HD double add_product(double acc, double x, double y) {
  const double t = x * y;
  return acc + t;
}

// The sum of row i's terms term(j), i < j < n, in the order above.  Host code; on the device lane l is accumulator l
// and walks the same blocks of kLanes columns (mantel.hip).
template <typename Term>
inline double row_sum(uint32_t i, uint32_t n, Term &&term) {
  double a[kLanes];
  for (uint32_t l = 0; l < kLanes; ++l) a[l] = kSumStart;
  uint32_t j = i + 1;
  for (; j < n && j % kLanes; ++j) a[j % kLanes] = term(a[j % kLanes], j);  // up to the first whole block
  for (; j + kLanes <= n; j += kLanes)
    for (uint32_t l = 0; l < kLanes; ++l) a[l] = term(a[l], j + l);
  for (; j < n; ++j) a[j % kLanes] = term(a[j % kLanes], j);
  for (uint32_t w = kLanes / 2; w >= 1; w /= 2)
    for (uint32_t l = 0; l < w; ++l) a[l] = a[l] + a[l + w];
  return a[0];
}

// What pa_mantel and pa_mantel_host check before they read a matrix, in the contract's order: null arguments, the
// range of n, then every row of h_perms (a permutation of 0 .. n - 1).  On PA_OK `inverse` holds, row by row, the
// identity's inverse and then each row's: inverse[(1 + q) * n + h_perms[q * n + t]] = t.  mantel_host.cpp has the body.
int check_arguments(const void *X, const void *Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, const void *h_stats, const void *h_cross,
                    std::vector<uint32_t> *inverse);

}  // namespace mantel
