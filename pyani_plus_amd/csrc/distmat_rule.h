// distmat_rule.h -- the check of a distance matrix, stated once for every entry point that takes one (pa_nj,
// pa_gower_center, pa_mantel and their host twins): finite, not negative, the bits of its transpose, zero diagonal.
// distmat.hip has the device side (declared in pa_internal.h), distmat_host.cpp the host side and the one message.
#pragma once

#include <cstdint>

#include "pa_hd.h"

namespace distmat {

// A cell the contract refuses: not finite, below zero, not the bits of its transpose, or a diagonal cell that is not zero
PA_HD bool bad_cell(double v, double transposed, bool diagonal) {
  uint64_t a, b;
  __builtin_memcpy(&a, &v, 8);
  __builtin_memcpy(&b, &transposed, 8);
  const bool finite = (a & 0x7FF0000000000000ULL) != 0x7FF0000000000000ULL;
  return !finite || v < 0.0 || a != b || (diagonal && v != 0.0);
}

// The refusal (PA_E_INVALID, the message set): `bad` cells of the n x n matrix `name` break the rule, the first of them
// in row-major order at cell `first`.  `who` is the entry point the message begins with.
int refuse(const char *who, const char *name, uint32_t n, uint64_t bad, uint64_t first);

}  // namespace distmat

// The check of a host matrix: PA_OK, or the refusal above
int pa_check_distance_matrix_host(const char *who, const char *name, const double *M, uint32_t n);
