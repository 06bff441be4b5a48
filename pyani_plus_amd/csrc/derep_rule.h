// derep_rule.h -- the rules of dereplicate-run, stated once for derep.hip and derep_host.cpp (DESIGN.md section 7k has
// the contract): the edge of two genomes, the total order in which the cover mode chooses, and the total order in which a
// genome is given its representative.  The aggregate of a pair is pair_rule.h's.
#pragma once

#include <cstdint>

#include "../../include/pyani_hip.h"
#include "pair_rule.h"

namespace derep {

constexpr uint32_t kMaxN = 65535;
constexpr uint32_t kNone = PA_DEREP_NONE;  // the representative of a node that is adjacent to none

// classify's aggregators and the value of a pair from its two cells (pair_rule.h)
using pair_rule::agg_ok;
using pair_rule::pair_value;
PA_HD bool mode_ok(int mode) { return mode == PA_DEREP_GREEDY || mode == PA_DEREP_COVER; }
PA_HD uint32_t words(uint32_t n) { return (n + 63u) / 64u; }

// lo != hi are adjacent iff neither value is NaN, cov > cov_min (strict) and score >= min_score (inclusive)
PA_HD bool edge(double score, double cov, double min_score, double cov_min) {
  return score == score && cov == cov && cov > cov_min && score >= min_score;
}

// The cover mode's choice as one unsigned key, the largest of which wins: the gain (at most 65535), then a node that is
// itself uncovered before one that is covered, then the smaller index.  0 stands for no candidate: a gain of 0 never
// enters.
PA_HD uint64_t cover_key(uint32_t gain, bool uncovered, uint32_t p) {
  return gain == 0 ? 0ull : ((uint64_t)gain << 33) | ((uint64_t)(uncovered ? 1u : 0u) << 32) | (uint64_t)(0xFFFFFFFFu - p);
}
PA_HD uint32_t cover_key_gain(uint64_t key) { return (uint32_t)(key >> 33); }
PA_HD uint32_t cover_key_node(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

// The assignment's total order: the larger score, equal scores (== on doubles, so -0.0 equals 0.0) to the smaller
// representative.  Any representative beats none; a NaN score never enters (the callers pass it over).
struct Pick {
  double score;
  uint32_t rep;
};
PA_HD bool better(const Pick &x, const Pick &than) {
  if (x.rep == kNone) return false;
  if (than.rep == kNone) return true;
  if (x.score > than.score) return true;
  if (!(x.score == than.score)) return false;
  return x.rep < than.rep;
}

// The refusals of the three calls, device entry point and twin alike (derep_host.cpp): PA_OK, or PA_E_INVALID with the
// message set.  n, then null arguments, then the aggregators or the mode, then the thresholds.
int check_adjacency(const void *S, const void *C, uint32_t n, int agg_score, int agg_cov, double min_score, double cov_min, const void *bits);
int check_select(const void *bits, uint32_t n, int mode, const void *is_rep, const void *n_reps);
int check_assign(const void *S, uint32_t n, int agg_score, const void *bits, const void *is_rep, const void *rep, const void *rep_score);

}  // namespace derep
