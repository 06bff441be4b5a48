// hits_rule.h -- the rules of search-run's selection, stated once for hits.hip and hits_host.cpp (DESIGN.md section 7n
// has the contract): a hit's denominator under the two ranks, and the strict total order in which a query's hits are
// ranked.  Integers only: no floating point takes part.
#pragma once

#include <cstdint>

#include "../../include/pyani_hip.h"
#include "pa_hd.h"

namespace hits {

constexpr uint32_t kNone = PA_HITS_NONE;  // the subject of a missing rank

PA_HD bool rank_ok(int rank) { return rank == PA_HITS_RANK_IDENTITY || rank == PA_HITS_RANK_CONTAINMENT; }

// m: min(|Q|, |S|) under identity (the larger of the two containments), |Q| under containment
PA_HD uint32_t denominator(int rank, uint32_t q_size, uint32_t s_size) {
  return rank == PA_HITS_RANK_IDENTITY && s_size < q_size ? s_size : q_size;
}

// shared = I = |S_q n S_s|, denom = m, subject = the subject's index.  shared == 0 is no hit and comes after every hit.
struct Hit {
  uint32_t shared, denom, subject;
};
constexpr Hit kNoHit{0u, 0u, kNone};

// a comes before b: the larger I / m as exact u64 cross products (all four factors are below 2^32), then the larger I,
// then the lower subject index.  Indices are distinct, so of two different hits exactly one comes before the other.
PA_HD bool before(const Hit &a, const Hit &b) {
  if (a.shared == 0) return false;
  if (b.shared == 0) return true;
  const uint64_t ab = (uint64_t)a.shared * b.denom, ba = (uint64_t)b.shared * a.denom;
  if (ab != ba) return ab > ba;
  if (a.shared != b.shared) return a.shared > b.shared;
  return a.subject < b.subject;
}

// The refusals of pa_best_hits, device entry point and twin alike (hits_host.cpp): PA_OK, or PA_E_INVALID with the
// message set: top, rank, ld, the index range, then the null pointers (an array of no elements may be null).
int check(const void *counts, uint32_t nq, uint32_t ns, uint64_t ld, const void *q_size, const void *s_size, uint32_t s_base, int rank, uint32_t top,
          const void *hit_subject, const void *hit_shared, const void *hit_denom);

}  // namespace hits
