// hits_host.cpp -- search-run's selection on the host: the refusals of pa_best_hits (which the device entry point
// shares) and the twin pa_best_hits_host: what hits.hip is compared with, bit for bit, and what search-run uses with an
// engine that has no device selection.  include/pyani_hip.h and DESIGN.md section 7n have the contract; hits_rule.h has
// its rules, the same functions the kernel calls.
//
// The twin is the plain sequential algorithm: per query a list of `top` hits kept in order, every column with a count
// inserted where it belongs.  Queries are handed out to host-pool threads, each row made by one thread, so the number
// of threads does not show in a result.
#include <cstdint>

#include "pa_host.h"

#include "hits_rule.h"

namespace {

constexpr uint32_t kStrip = 16;  // queries a thread takes at a time

int refuse(const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
  pa_set_error(fmt, a, b);
  return PA_E_INVALID;
}

}  // namespace

int hits::check(const void *counts, uint32_t nq, uint32_t ns, uint64_t ld, const void *q_size, const void *s_size, uint32_t s_base, int rank,
                uint32_t top, const void *hit_subject, const void *hit_shared, const void *hit_denom) {
  if (top < 1 || top > PA_HITS_MAX_TOP) return refuse("pa_best_hits: top %llu (1 to %llu)", top, PA_HITS_MAX_TOP);
  if (!rank_ok(rank)) {
    pa_set_error("pa_best_hits: rank %d (PA_HITS_RANK_IDENTITY or PA_HITS_RANK_CONTAINMENT)", rank);
    return PA_E_INVALID;
  }
  if (ld < ns) return refuse("pa_best_hits: ld %llu is less than ns %llu", ld, ns);
  if ((uint64_t)s_base + ns >= kNone) return refuse("pa_best_hits: index overflow: s_base %llu + ns %llu reaches PA_HITS_NONE", s_base, ns);
  if (nq > 1 && ld > (~0ull / 4) / nq) return refuse("pa_best_hits: index overflow: nq %llu rows of ld %llu counts", nq, ld);
  if (nq && ns && !counts) return refuse("pa_best_hits: null counts");
  if (nq && !q_size) return refuse("pa_best_hits: null q_size");
  if (ns && !s_size) return refuse("pa_best_hits: null s_size");
  if (nq && !hit_subject) return refuse("pa_best_hits: null hit_subject");
  if (nq && !hit_shared) return refuse("pa_best_hits: null hit_shared");
  if (nq && !hit_denom) return refuse("pa_best_hits: null hit_denom");
  return PA_OK;
}

extern "C" int pa_best_hits_host(const uint32_t *h_counts, uint32_t nq, uint32_t ns, uint64_t ld, const uint32_t *h_q_size, const uint32_t *h_s_size,
                                 uint32_t s_base, int rank, uint32_t top, int accumulate, uint32_t *h_hit_subject, uint32_t *h_hit_shared,
                                 uint32_t *h_hit_denom, uint32_t n_threads) {
  if (const int s = hits::check(h_counts, nq, ns, ld, h_q_size, h_s_size, s_base, rank, top, h_hit_subject, h_hit_shared, h_hit_denom)) return s;
  for (uint32_t q = 0; q < nq; ++q)
    if (h_q_size[q] == 0) return refuse("pa_best_hits_host: q_size[%llu] is 0 (sizes are 1 to 2^32 - 1)", q);
  for (uint32_t c = 0; c < ns; ++c)
    if (h_s_size[c] == 0) return refuse("pa_best_hits_host: s_size[%llu] is 0 (sizes are 1 to 2^32 - 1)", c);
  return pa_host_guard("pa_best_hits_host", [&]() -> int {
    pa_for_chunks(0, nq, kStrip, pa_host_threads((uint64_t)nq * (ns + top), 1u << 16, n_threads), [&](uint32_t, uint64_t q0, uint64_t q1) {
      hits::Hit list[PA_HITS_MAX_TOP];  // best first; the ranks past `held` are missing
      for (uint64_t q = q0; q < q1; ++q) {
        uint32_t held = 0;
        const auto insert = [&](const hits::Hit &h) {
          if (held == top && !hits::before(h, list[top - 1])) return;
          uint32_t at = held < top ? held++ : top - 1;
          for (; at > 0 && hits::before(h, list[at - 1]); --at) list[at] = list[at - 1];
          list[at] = h;
        };
        uint32_t *subject = h_hit_subject + q * top, *shared = h_hit_shared + q * top, *denom = h_hit_denom + q * top;
        for (uint32_t r = 0; accumulate && r < top; ++r)
          if (subject[r] != hits::kNone && shared[r] != 0) insert(hits::Hit{shared[r], denom[r], subject[r]});
        const uint32_t *row = h_counts + q * ld;
        for (uint32_t c = 0; c < ns; ++c)
          if (row[c] != 0) insert(hits::Hit{row[c], hits::denominator(rank, h_q_size[q], h_s_size[c]), s_base + c});
        for (uint32_t r = 0; r < top; ++r) {
          const hits::Hit h = r < held ? list[r] : hits::kNoHit;
          subject[r] = h.subject;
          shared[r] = h.shared;
          denom[r] = h.denom;
        }
      }
    });
    return PA_OK;
  });
}
