// msa_boot_rule.h -- the arithmetic of bootstrap-run, stated once for msa_boot.hip and msa_boot_host.cpp (DESIGN.md
// section 7l has the contract): the column a draw hits, the distance of a pair's weighted counts, and what both sides
// check of a batch of weights.  The distance is one conversion each, one division and one subtraction, each rounded on
// its own (strict_fp.h).
#pragma once

#include <cstdint>

#include "../../include/pyani_hip.h"
#include "mantel_rule.h"  // fin, the splitmix64 finaliser

namespace boot {

constexpr uint32_t kMaxWeight = 255;  // a weight is a uint8

// the high 64 bits of a * b (the draws are made on the host)
inline uint64_t mulhi64(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

// Replicate r of `seed` draws n_cols columns: draw t hits column mulhi64(fin(base + t), n_cols)
inline uint64_t replicate_base(uint64_t seed, uint64_t r) { return mantel::fin(mantel::fin(seed) + r); }
inline uint64_t drawn_column(uint64_t base, uint64_t t, uint64_t n_cols) { return mulhi64(mantel::fin(base + t), n_cols); }

// D[i, j] of a replicate from M[i, j], B[i, j] and the rows' weighted residue counts n_i = B[i, i], n_j = B[j, j]:
// the reference's identity M / aln_length with pa_msa_metrics' division, taken from 1.0; `missing` where the pair has
// no aligned column left; 0.0 on the diagonal
PA_HD double distance(uint32_t i, uint32_t j, uint32_t m, uint32_t b, uint32_t n_i, uint32_t n_j, double missing) {
  if (i == j) return 0.0;
  const uint64_t aln = (uint64_t)n_i + n_j - b;
  if (aln == 0) return missing;
  const double identity = (double)m / (double)aln;
  return 1.0 - identity;
}

// bit_length of the largest weight: the planes a batch's weights are sliced into
inline uint32_t weight_planes(uint32_t max_weight) {
  uint32_t nb = 0;
  while (max_weight >> nb) ++nb;
  return nb;
}

// What pa_msa_boot_counts and pa_msa_boot_counts_host check of n_reps rows of n_cols weights: every row sums to
// n_cols.  PA_OK with the largest weight in *max_weight, or PA_E_INVALID naming the first row that does not.
// msa_boot_host.cpp has the body.
int check_weights(const char *who, const uint8_t *h_weights, uint64_t n_cols, uint32_t n_reps, uint32_t *max_weight);

}  // namespace boot
