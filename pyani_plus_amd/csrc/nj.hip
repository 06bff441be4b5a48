// nj.hip -- the neighbour-joining tree of a distance matrix, every join on the device (gfx950, wave64).
//
// tree-run turns a finished run's identities into a tree file.  Canonical neighbour joining (Saitou & Nei 1987 in
// Studier & Keppler's form) scans every live pair before each of its n - 2 joins: about n^3 / 6 pair scores and as many
// 8-byte reads.  pa_nj does that scan, the join and the update of the matrix on the device and reads the join table back
// once.  The definition is this project's own (the reference has no tree): DESIGN.md section 7h has the contract,
// tests/tree_cases.py restates it independently, nj_host.cpp is the twin with the same bits.
//
// The contract, in short (nj_rule.h has each formula as one function, shared with the twin):
//   input   D, n x n f64 row-major, finite, >= 0, bitwise symmetric, zero diagonal, 1 <= n <= 65535; anything else is
//           PA_E_INVALID and the message names the first offending cell in row-major order (the check is distmat.hip's);
//   ids     leaves 0 .. n - 1, the node made by join t is n + t;
//   set-up  r[i] = D[i, 0] + ... + D[i, n - 1], added in this order into one accumulator; m = n live nodes;
//   while m > 2
//     score   of a live pair with ids lo < hi: q = ((double)(m - 2) * d(lo, hi) - r[lo]) - r[hi], the product rounded
//             before the subtractions (no FMA: contraction is off for this file, by strict_fp.h below and in the Makefile);
//     choice  the smallest q; among equal q (== on doubles) the smallest lo, then the smallest hi -- by node id, never
//             by where a node is stored, so the storage layout below does not show in the result;
//     join    d = d(lo, hi); len_lo = 0.5 * d + (r[lo] - r[hi]) / (2.0 * (double)(m - 2)); len_hi = d - len_lo; negative
//             lengths are kept; the record is (lo, hi, len_lo, len_hi);
//     update  for every other live k: d(u, k) = 0.5 * ((d(lo, k) + d(hi, k)) - d),
//             r[k] = ((r[k] - d(lo, k)) - d(hi, k)) + d(u, k); r[u] = 0.5 * ((r[lo] + r[hi]) - (double)m * d); m -= 1;
//   m = 2   the two remaining nodes a < b and d(a, b) are the last edge.  n = 2: no join, the last edge (0, 1, D[0, 1]);
//           n = 1: nothing.
// Inputs whose scores overflow (distances near 1e308) are outside the contract: every index stays in bounds, the tree is
// whatever IEEE arithmetic gives.
//
// Layout.  The live nodes occupy the storage slots 0 .. m - 1 of D (row stride n), both triangles kept; id[s] is the
// node in slot s and slot_of[v] the slot of node v.  A join puts u into the smaller of its two slots and moves the
// last slot's row and column into the larger one (swap-remove), so the live matrix stays compact and the scan reads
// whole contiguous row segments while the work shrinks as m^2.
//
// Three launches per join through the checked launcher, enqueued by a host that knows m = n - t; no read-back inside the
// loop, no grid-wide barrier, no graph capture, no floating-point atomics:
//   nj_scan_kernel    grid nt x nt of kTile x kTile slot tiles, the tiles below the diagonal return at once (as in
//                     rowdist.hip).  Lane = one column b, kThreads / kTile row groups; each row's kTile doubles are one
//                     coalesced segment.  r and id of the tile's rows are staged in LDS (every lane of a row group reads
//                     the same word: a broadcast), those of the column sit in registers.  Each lane keeps its best
//                     (q, lo, hi) under the total order; block_reduce gives the workgroup's, one candidate per tile.
//   nj_join_kernel    one workgroup: reduces the candidates, computes the two lengths, appends the record to the join
//                     table, publishes the pair, its slots, d and r[u] through the kNjPick slot.
//   nj_update_kernel  one lane per live slot k: u's new row and column, r[k], then the swap-remove.  Every lane reads
//                     column k of rows lo, hi and last only and writes cells no other lane reads (see the kernel).
// The memory system bounds the scan: 8 bytes per pair against a dozen f64 vector operations.
#include "pa_internal.h"

#include <memory>
#include <new>

#include "block_reduce_dev.h"
#include "nj_rule.h"

namespace {

using nj::Cand;
using nj::kNone;

constexpr int kThreads = 256;  // lanes per workgroup, every kernel of this file
constexpr int kTile = 128;     // slots per side of a scan tile: kTile * kTile pairs per workgroup
constexpr int kRowGroups = kThreads / kTile;
constexpr int kBatch = 8;  // loads of a lane in flight before the first is used
constexpr uint32_t kProfJoins = 512;  // joins timed per call when the event timer is on
constexpr int kSumThreads = 64;  // the row sums: one lane per row, small workgroups so that more of them stream
static_assert(kThreads % kTile == 0 && kTile <= kThreads, "a scan workgroup covers whole columns of its tile");

// The workgroup's best candidate, to every lane.  The candidates sit in LDS field by field and block_reduce runs over
// lane numbers, its operator comparing the candidates of two lanes: plain 32-bit values in the tree, nothing on the stack.
struct BestLds {
  double q[kThreads];
  uint32_t lo[kThreads], hi[kThreads], lane[kThreads];
};
__device__ __forceinline__ Cand block_best(const Cand &mine, BestLds &s) {
  s.q[threadIdx.x] = mine.q;
  s.lo[threadIdx.x] = mine.lo;
  s.hi[threadIdx.x] = mine.hi;  // visible after the barrier that follows block_reduce's own store
  const uint32_t w = pa_dev::block_reduce<kThreads>((uint32_t)threadIdx.x, s.lane, [&s](uint32_t i, uint32_t j) {
    return nj::better(Cand{s.q[j], s.lo[j], s.hi[j]}, Cand{s.q[i], s.lo[i], s.hi[i]}) ? j : i;
  });
  return Cand{s.q[w], s.lo[w], s.hi[w]};
}

// What the join kernel hands the update kernel (kNjPick)
struct NjPick {
  uint32_t lo, hi, slot_lo, slot_hi;
  double d, r_u;
};
static_assert(sizeof(NjPick) == kNjPick.bytes(), "NjPick fills its slot");

// The context's workspace: r, the join table as it is read back (f64 part, then u32 part), id, slot_of, candidates
struct NjWork {
  double *r, *len;      // len[2 (n - 2)], then last_len
  uint32_t *child;      // child[2 (n - 2)], then last[2]
  uint32_t *id, *slot_of;
  Cand *cand;
  uint64_t table_bytes;
};
uint64_t table_f64(uint32_t n) { return n > 2 ? 2ull * (n - 2) + 1 : 1; }
uint64_t table_u32(uint32_t n) { return n > 2 ? 2ull * (n - 2) + 2 : 2; }

// r[i] by walking k upwards: D[k, i] is D[i, k] bit for bit and is read coalesced across i.  Also id and slot_of.
__global__ __launch_bounds__(kSumThreads) void nj_rowsum_kernel(const double *__restrict__ D, uint32_t n, double *__restrict__ r,
                                                               uint32_t *__restrict__ id, uint32_t *__restrict__ slot_of) {
  const uint32_t i = blockIdx.x * kSumThreads + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (uint32_t k0 = 0; k0 < n; k0 += kBatch) {  // kBatch loads in flight, then the additions in order
    double v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = k0 + j < n ? D[(uint64_t)(k0 + j) * n + i] : 0.0;
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 + j < n) s = s + v[j];
  }
  r[i] = s;
  id[i] = i;
  slot_of[i] = i;
}

__global__ __launch_bounds__(kThreads) void nj_scan_kernel(const double *__restrict__ D, uint32_t n, uint32_t m, const double *__restrict__ r,
                                                         const uint32_t *__restrict__ id, Cand *__restrict__ cand) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  __shared__ double s_r[kTile];
  __shared__ uint32_t s_id[kTile];
  __shared__ BestLds s_best;
  const uint32_t a0 = ti * kTile;
  if (threadIdx.x < kTile) {
    const uint32_t a = a0 + threadIdx.x;
    s_r[threadIdx.x] = a < m ? r[a] : 0.0;
    s_id[threadIdx.x] = a < m ? id[a] : 0u;
  }
  __syncthreads();
  const uint32_t col = threadIdx.x % kTile, group = threadIdx.x / kTile;
  const uint32_t b = tj * kTile + col;
  Cand best{0.0, kNone, kNone};
  // The rows of this tile are the same for every lane (a0 + ar < m), so a batch of kBatch loads is issued before the
  // first of them is used; what differs per lane is which rows count: slots a < b, that is ar < col on the diagonal
  // tile and every row off it (a < (ti + 1) kTile <= tj kTile <= b), none for a column past the live slots, whose
  // lane reads column m - 1 instead and drops what it read.
  const uint32_t tile_rows = m - a0 < (uint32_t)kTile ? m - a0 : (uint32_t)kTile;
  const uint32_t mine = b >= m ? 0u : (ti == tj ? col : tile_rows);
  const uint32_t b_read = b < m ? b : m - 1;
  const double r_b = r[b_read], m_minus_2 = (double)(m - 2);
  const uint32_t id_b = id[b_read];
  const double *cell = D + (uint64_t)a0 * n + b_read;
  for (uint32_t ar0 = group; ar0 < tile_rows; ar0 += kRowGroups * kBatch) {
    double d[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const uint32_t ar = ar0 + i * kRowGroups;
      d[i] = ar < tile_rows ? cell[(uint64_t)ar * n] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const uint32_t ar = ar0 + i * kRowGroups;
      if (ar < mine) {
        const uint32_t id_a = s_id[ar];
        const double r_a = s_r[ar];
        const bool a_first = id_a < id_b;
        const Cand c{nj::score(m_minus_2, d[i], a_first ? r_a : r_b, a_first ? r_b : r_a), a_first ? id_a : id_b, a_first ? id_b : id_a};
        const bool take = nj::better(c, best);
        best.q = take ? c.q : best.q;
        best.lo = take ? c.lo : best.lo;
        best.hi = take ? c.hi : best.hi;
      }
    }
  }
  best = block_best(best, s_best);
  if (threadIdx.x == 0) cand[(uint64_t)ti * gridDim.x + tj] = best;
}

__global__ __launch_bounds__(kThreads) void nj_join_kernel(const double *__restrict__ D, uint32_t n, uint32_t m, uint32_t t, uint32_t nt,
                                                         const Cand *__restrict__ cand, const double *__restrict__ r,
                                                         const uint32_t *__restrict__ slot_of, double *__restrict__ len,
                                                         uint32_t *__restrict__ child, NjPick *__restrict__ pick) {
  __shared__ BestLds s_best;
  Cand best{0.0, kNone, kNone};
  for (uint32_t at = threadIdx.x; at < nt * nt; at += kThreads) {
    if (at % nt < at / nt) continue;  // a tile below the diagonal wrote nothing
    const Cand c = cand[at];
    if (nj::better(c, best)) best = c;
  }
  best = block_best(best, s_best);
  if (threadIdx.x != 0) return;
  NjPick p{best.lo, best.hi, 0u, 0u, 0.0, 0.0};
  if (best.lo != kNone) {  // always, with m >= 3 live nodes; the update kernel does nothing otherwise
    p.slot_lo = slot_of[best.lo];
    p.slot_hi = slot_of[best.hi];
    p.d = D[(uint64_t)p.slot_lo * n + p.slot_hi];
    const double r_lo = r[p.slot_lo], r_hi = r[p.slot_hi], m_minus_2 = (double)(m - 2);
    const double len_lo = nj::length_lo(m_minus_2, p.d, r_lo, r_hi);
    p.r_u = nj::row_sum_joined((double)m, p.d, r_lo, r_hi);
    child[2 * (uint64_t)t] = best.lo;
    child[2 * (uint64_t)t + 1] = best.hi;
    len[2 * (uint64_t)t] = len_lo;
    len[2 * (uint64_t)t + 1] = p.d - len_lo;
  }
  *pick = p;
}

// Lane k is live slot k.  With A, B the slots of lo and hi, P = min(A, B) the slot u takes, R = max(A, B) the slot
// that the last slot L = m - 1 moves into: lane k outside {A, B} reads cells (A, k), (B, k), (L, k) and r[k] only, and
// writes (P, k'), (k', P), (R, k), (k, R), r[k'] with k' = k, or R for k = L.  No lane writes a cell of row A, B or L
// in another lane's column, so no lane reads what another writes; rows and columns L are dead afterwards.
__global__ __launch_bounds__(kThreads) void nj_update_kernel(double *__restrict__ D, uint32_t n, uint32_t m, uint32_t u,
                                                           const NjPick *__restrict__ pick, double *__restrict__ r,
                                                           uint32_t *__restrict__ id, uint32_t *__restrict__ slot_of) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= m) return;
  const NjPick p = *pick;
  if (p.lo == kNone || p.slot_lo >= m || p.slot_hi >= m) return;
  const uint32_t A = p.slot_lo, B = p.slot_hi, P = A < B ? A : B, R = A < B ? B : A, L = m - 1;
  if (k == A || k == B) {
    if (k == P) {
      r[P] = p.r_u;
      id[P] = u;
      slot_of[u] = P;
    }
    return;
  }
  const double d_lo = D[(uint64_t)A * n + k], d_hi = D[(uint64_t)B * n + k];
  const double d_u = nj::joined_distance(d_lo, d_hi, p.d);
  const double r_k = nj::row_sum_after(r[k], d_lo, d_hi, d_u);
  if (k == L) {  // R != L here: the last slot's node moves into slot R
    D[(uint64_t)P * n + R] = d_u;
    D[(uint64_t)R * n + P] = d_u;
    r[R] = r_k;
    const uint32_t moved = id[L];
    id[R] = moved;
    slot_of[moved] = R;
    return;
  }
  const double d_last = D[(uint64_t)L * n + k];
  D[(uint64_t)P * n + k] = d_u;
  D[(uint64_t)k * n + P] = d_u;
  r[k] = r_k;
  if (R != L) {
    D[(uint64_t)R * n + k] = d_last;
    D[(uint64_t)k * n + R] = d_last;
  }
}

// m = 2: slots 0 and 1 hold the last edge
__global__ void nj_last_kernel(const double *__restrict__ D, uint32_t n, const uint32_t *__restrict__ id, double *__restrict__ last_len,
                               uint32_t *__restrict__ last) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t x = id[0], y = id[1];
  last[0] = x < y ? x : y;
  last[1] = x < y ? y : x;
  *last_len = D[1];
}

static_assert(alignof(uint32_t) <= alignof(double), "the join table -- len, last_len, child, last -- is read back as one block: no gap before child");
static_assert(alignof(Cand) <= 16 && sizeof(Cand) % 16 == 0, "cand on 16 bytes puts every candidate on 16 bytes");
int nj_workspace(pa_ctx *c, uint32_t n, NjWork *w) {
  const uint64_t nt = (n + kTile - 1) / kTile;
  return pa_carve(c->nj_work, "nj_work", [&](Carve &k) {
    w->r = k.take<double>(n);
    w->len = k.take<double>(table_f64(n));
    w->child = k.take<uint32_t>(table_u32(n));
    w->table_bytes = k.end() - n * sizeof(double);  // from len to here
    w->id = k.take<uint32_t>(n);
    w->slot_of = k.take<uint32_t>(2ull * n);
    const uint64_t skipped = k.align_to(16);  // out of the 16 bytes set aside for it: what it leaves is the tail
    w->cand = k.take<Cand>(nt * nt, 16);
    k.slack(16 - skipped);
  });
}

}  // namespace

extern "C" int pa_nj(pa_ctx *c, double *d_D, uint32_t n, uint32_t *h_child, double *h_len, uint32_t *h_last, double *h_last_len) {
  PA_REQUIRE(c != nullptr, "pa_nj: null context");
  PA_REQUIRE(n >= 1 && n <= 65535, "pa_nj: %u nodes; 1 to 65535", n);
  PA_REQUIRE(d_D != nullptr, "pa_nj: null matrix");
  PA_REQUIRE(n < 2 || (h_last != nullptr && h_last_len != nullptr), "pa_nj: null argument for the last edge");
  PA_REQUIRE(n < 3 || (h_child != nullptr && h_len != nullptr), "pa_nj: null argument for the join table");
  PA_HIP(hipSetDevice(c->device));
  NjWork w;
  PA_TRY(nj_workspace(c, n, &w));
  PA_TRY(pa_check_distance_matrix(c, "pa_nj", d_D, n));  // one read-back
  if (n == 1) return PA_OK;
  PA_TRY(PA_LAUNCH(c, nj_rowsum_kernel, (n + kSumThreads - 1) / kSumThreads, kSumThreads, 0, (const double *)d_D, n, w.r, w.id, w.slot_of));
  NjPick *d_pick = c->slot<NjPick>(kNjPick);
  // with the event timer on, every stride-th join is timed, at most kProfJoins of them: two events per launch of tens of
  // thousands of launches would be a load of their own.  The phases' totals are then those of the timed joins.
  const uint32_t prof_stride = n > 2 ? (n - 2 + kProfJoins - 1) / kProfJoins : 1;
  auto step = [c](int phase, bool timed, auto &&launch) -> int {
    if (!timed) return launch();
    ProfScope prof(c, phase);
    return launch();
  };
  for (uint32_t t = 0; t + 2 < n; ++t) {  // the host knows m: it only enqueues
    const uint32_t m = n - t, nt = (m + kTile - 1) / kTile;
    const bool timed = c->prof_on && t % prof_stride == 0;
    PA_TRY(step(PA_PROF_NJ_SCAN, timed, [&] {
      return PA_LAUNCH(c, nj_scan_kernel, LaunchDim(nt, nt), kThreads, 0, (const double *)d_D, n, m, (const double *)w.r, (const uint32_t *)w.id, w.cand);
    }));
    PA_TRY(step(PA_PROF_NJ_JOIN, timed, [&] {
      return PA_LAUNCH(c, nj_join_kernel, 1, kThreads, 0, (const double *)d_D, n, m, t, nt, (const Cand *)w.cand, (const double *)w.r,
                       (const uint32_t *)w.slot_of, w.len, w.child, d_pick);
    }));
    PA_TRY(step(PA_PROF_NJ_UPDATE, timed, [&] {
      return PA_LAUNCH(c, nj_update_kernel, (m + kThreads - 1) / kThreads, kThreads, 0, d_D, n, m, n + t, (const NjPick *)d_pick, w.r, w.id, w.slot_of);
    }));
  }
  const uint64_t joins2 = n > 2 ? 2ull * (n - 2) : 0;
  PA_TRY(PA_LAUNCH(c, nj_last_kernel, 1, 64, 0, (const double *)d_D, n, (const uint32_t *)w.id, w.len + joins2, w.child + joins2));
  // the join table: the other read-back
  std::unique_ptr<unsigned char[]> table(new (std::nothrow) unsigned char[w.table_bytes]);
  if (!table) {
    pa_set_error("pa_nj: out of host memory for the join table of %u nodes", n);
    return PA_E_NOMEM;
  }
  PA_TRY(pa_copy_to_host(c, table.get(), w.len, w.table_bytes));
  const unsigned char *u32_part = table.get() + table_f64(n) * 8;
  if (joins2) {
    memcpy(h_len, table.get(), joins2 * 8);
    memcpy(h_child, u32_part, joins2 * 4);
  }
  memcpy(h_last_len, table.get() + joins2 * 8, 8);
  memcpy(h_last, u32_part + joins2 * 4, 8);
  return PA_OK;
}
