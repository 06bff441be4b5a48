// hits.hip -- search-run's selection on the device (gfx950, wave64): for every query the `top` best subjects of a tile
// of intersection counts, merged with the lists the earlier tiles left, so that M x top numbers cross the bus and not
// M x N.
//
// The reference has no such command: DESIGN.md section 7n has the contract, tests/search_cases.py restates it
// independently, hits_host.cpp is the twin with the same bits and hits_rule.h states the order once for both.
//
//   pa_best_hits  best_hits_kernel: one workgroup of 256 lanes per query.  Lane t owns the columns t, t + 256, ... of the
//                 query's row and, when the call accumulates, entry t of the list so far.  Every lane keeps the best of
//                 what it owns that has not been ranked yet; a rank is one block_reduce of these 256 candidates under
//                 hits::before, and only the lane that owned the winner looks through its columns again, for its best
//                 candidate after the winner in the order.  The row is therefore read once by everybody and then
//                 `top` - 1 times by one lane each (ns / 256 columns, from L2), instead of `top` times by everybody, and
//                 no lane holds a list: the registers do not grow with `top`.  The walk ends at the first rank without
//                 a hit.
// The order is strict and total, the reduction tree is fixed and no atomics are used: the result does not depend on the
// arrival order, and is the same bits run to run and as the twin's.  Integer work only.  The list so far is read into
// registers before the first barrier and written after it, so the outputs may be the inputs.
#include "pa_internal.h"

#include "block_reduce_dev.h"
#include "hits_rule.h"

namespace {

constexpr int kThreads = 256;  // the columns-per-lane stride
static_assert(PA_HITS_MAX_TOP <= kThreads, "lane t holds entry t of the list so far");

__global__ __launch_bounds__(kThreads) void best_hits_kernel(const uint32_t *__restrict__ counts, uint32_t ns, uint64_t ld,
                                                             const uint32_t *__restrict__ q_size, const uint32_t *__restrict__ s_size,
                                                             uint32_t s_base, int rank, uint32_t top, int accumulate, uint32_t *hit_subject,
                                                             uint32_t *hit_shared, uint32_t *hit_denom) {
  __shared__ hits::Hit s_tree[kThreads];
  const uint32_t q = blockIdx.x, t = threadIdx.x;
  const uint32_t *row = counts + (uint64_t)q * ld;
  const uint32_t own_size = q_size[q];
  uint32_t *subject = hit_subject + (uint64_t)q * top, *shared = hit_shared + (uint64_t)q * top, *denom = hit_denom + (uint64_t)q * top;
  hits::Hit held = hits::kNoHit;  // entry t of the list so far
  if (accumulate && t < top && subject[t] != hits::kNone) held = hits::Hit{shared[t], denom[t], subject[t]};

  hits::Hit mine = hits::kNoHit, last = hits::kNoHit;  // last: the hit of the rank before
  for (uint32_t r = 0; r < top; ++r) {
    if (r == 0 || mine.subject == last.subject) {  // the first rank, or this lane owned the last one: its best after `last`
      mine = hits::kNoHit;
      const auto offer = [&](const hits::Hit &h) {
        if (h.shared != 0 && (r == 0 || hits::before(last, h)) && hits::before(h, mine)) mine = h;
      };
      offer(held);
      for (uint32_t c = t; c < ns; c += kThreads) {
        const uint32_t I = row[c];
        if (I != 0) offer(hits::Hit{I, hits::denominator(rank, own_size, s_size[c]), s_base + c});
      }
    }
    last = pa_dev::block_reduce<kThreads>(mine, s_tree, [](const hits::Hit &a, const hits::Hit &b) { return hits::before(b, a) ? b : a; });
    if (last.shared == 0) {  // uniform: no hit is left, this rank and the ranks after it are missing
      for (uint32_t e = r + t; e < top; e += kThreads) {
        subject[e] = hits::kNone;
        shared[e] = 0;
        denom[e] = 0;
      }
      return;
    }
    if (t == 0) {
      subject[r] = last.subject;
      shared[r] = last.shared;
      denom[r] = last.denom;
    }
  }
}

}  // namespace

extern "C" int pa_best_hits(pa_ctx *c, const uint32_t *d_counts, uint32_t nq, uint32_t ns, uint64_t ld, const uint32_t *d_q_size,
                            const uint32_t *d_s_size, uint32_t s_base, int rank, uint32_t top, int accumulate, uint32_t *d_hit_subject,
                            uint32_t *d_hit_shared, uint32_t *d_hit_denom) {
  PA_REQUIRE(c != nullptr, "pa_best_hits: null context");
  PA_TRY(hits::check(d_counts, nq, ns, ld, d_q_size, d_s_size, s_base, rank, top, d_hit_subject, d_hit_shared, d_hit_denom));
  if (ns == 0 && accumulate) return PA_OK;  // the lists so far stay as they are
  PA_HIP(hipSetDevice(c->device));
  return PA_LAUNCH(c, best_hits_kernel, nq, kThreads, 0, d_counts, ns, ld, d_q_size, d_s_size, s_base, rank, top, accumulate, d_hit_subject,
                   d_hit_shared, d_hit_denom);
}
