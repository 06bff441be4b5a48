// pcoa_rule.h -- the constants and the arithmetic of ordinate-run, stated once for pcoa.hip and pcoa_host.cpp (DESIGN.md
// section 7i has the contract).  Every function is one line of the contract, each operation rounded on its own
// (strict_fp.h).
#pragma once

#include <cstdint>

#include "pa_hd.h"
#include "strict_fp.h"

namespace pcoa {

// The tall product Y = A Q adds a row's products in chunks of kChunk columns, then the chunks' sums: the order of the
// additions is part of the contract, so this is the one place that states it (tests/pcoa_cases.py reads it from here).
constexpr int kChunk = 256;

// The accumulator of a sum "that starts from its first term": -0.0 + x is x for every x, signed zeros included, so a
// loop that starts from -0.0 and adds every term gives the bits of one that starts from the first term.
constexpr double kSumStart = -0.0;

// One more product of a chunk: the product rounded, then the addition
PA_HD double mul_add(double acc, double a, double q) {
  const double prod = a * q;
  return acc + prod;
}

// The start block of the eigen-solver: Q0[i, c] = start_value(i * p + c), the splitmix64 finaliser of the index mapped
// to (-1, 1): the top 52 bits u give ((u + 0.5) * 2^-51) - 1, every step exact.
PA_HD double start_value(uint64_t index) {
  uint64_t z = index + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  z = z ^ (z >> 31);
  const double u = (double)(z >> 12);
  const double half = u + 0.5;
  const double scaled = half * 0x1p-51;
  return scaled - 1.0;
}

// a[i, j] = D[i, j] * D[i, j]
PA_HD double squared(double d) { return d * d; }

// B[i, j] = -0.5 * ((a[i, j] - (r[i] + r[j])) + g): r[i] + r[j] is commutative, so B is bitwise symmetric
PA_HD double centred(double a, double r_i, double r_j, double g) {
  const double rows = r_i + r_j;
  const double diff = a - rows;
  const double with_g = diff + g;
  return -0.5 * with_g;
}

}  // namespace pcoa
