// classify.hip -- the edge list of a run's genome graph, built and put into removal order on the device (gfx950,
// wave64).
//
// The reference builds a networkx graph pair by pair in Python (pyani_plus/classify.py:64-105: for every i < j,
// coverage = agg([C[j,i], C[i,j]]), score = agg([S[j,i], S[i,j]]), an edge iff neither is NaN and coverage >
// min_coverage) and then sorts the edge list again after every split (classify.py:157-158).  Here the N x N score and
// coverage matrices become, in one call, the edges in the order in which the reference's top level removes them:
// ascending score, equal scores by ascending (i, j).  The union-find pass over that list is host work
// (classify_host.cpp); DESIGN.md section 7b has the equivalence argument.
//
// Steps, all on the context's stream:
//   1. cls_edges_kernel<false>: one workgroup per 64 x 64 tile (ti <= tj) of the upper triangle, a wave per row of
//      the tile, a lane per column.  pair_tile_dev.h has the loader of a tile's values, shared with derep.hip: for
//      the pairs kept here (i < j) a value is agg(M[j,i], M[i,j]) (pair_rule.h's agg2).  Coverage and score go
//      through the same 33 KB LDS buffer one after the other.  Each wave counts the surviving pairs of its (row, tile)
//      with one ballot and writes the count to counts[i][tj].
//   2. pa_exclusive_scan_u32 over counts[n][nt], row-major: the offset of (row i, tile tj) is then the number of
//      edges before it in (i, j) order, because inside one (row, tile) the lanes are consecutive j.  The total E is
//      read back by the same call, pa_scan_total_u32: the call's only host synchronisation (the workspaces of the
//      next steps are sized by it).
//   3. cls_edges_kernel<true>: the same evaluation again; each surviving lane writes i, j, score, coverage, the
//      sort key and its own position at offset + popcount(ballot below the lane).  The compacted list is therefore
//      in (i, j) order and the value of element e is e.
//   4. pa_radix_sort_pairs over the 64 key bits.  The sort is stable, and the input is in (i, j) order, so equal keys
//      leave in (i, j) order: the tie rule holds by construction, with no second sort by pair index.  The key is the
//      usual order-preserving map of a double (negative: all bits flipped; else: sign bit set), taken after -0.0 has
//      been replaced by +0.0 so that the two zeros are one key, as they are one value to the reference's sort.  Only
//      the key is mapped: the score written is the one computed.
//   5. cls_gather_kernel: the four output arrays in sorted order.
#include "pa_internal.h"

#include "pair_tile_dev.h"

namespace {

using pair_rule::agg_ok;
using namespace pair_tile;  // kTile, kThreads, kRows, kPad, tile_values

__device__ __forceinline__ uint64_t score_key(double s) {
  uint64_t bits = (uint64_t)__double_as_longlong(s == 0.0 ? 0.0 : s);
  return (bits >> 63) ? ~bits : (bits | (1ULL << 63));
}

template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void cls_edges_kernel(const double *__restrict__ score, const double *__restrict__ cov, uint32_t n,
                                                             uint32_t nt, int agg_score, int agg_cov, double cov_min,
                                                             uint32_t *__restrict__ counts /*[n][nt]: counts out, or offsets in*/,
                                                             uint64_t n_edges, uint32_t *__restrict__ e_i, uint32_t *__restrict__ e_j,
                                                             double *__restrict__ e_score, double *__restrict__ e_cov,
                                                             uint64_t *__restrict__ e_key, uint32_t *__restrict__ e_val) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  __shared__ double tile[kTile][kPad];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t i0 = ti * kTile, j0 = tj * kTile;
  double c[kRows], s[kRows];
  tile_values<false>(cov, n, i0, j0, agg_cov, tile, c);
  tile_values<false>(score, n, i0, j0, agg_score, tile, s);
  const uint32_t j = j0 + lane;
  const uint64_t below = (lane == 0) ? 0ULL : (~0ULL >> (64 - lane));
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint32_t i = i0 + wave * kRows + k;
    if (i >= n) break;  // uniform in the wave
    const bool keep = j < n && j > i && c[k] == c[k] && s[k] == s[k] && c[k] > cov_min;
    const uint64_t mask = __ballot(keep);
    if (!SCATTER) {
      if (lane == 0) counts[(uint64_t)i * nt + tj] = (uint32_t)__popcll(mask);
    } else if (keep) {
      const uint64_t at = (uint64_t)counts[(uint64_t)i * nt + tj] + __popcll(mask & below);
      if (at < n_edges) {  // always: the offsets are the scan of the counts of the same evaluation
        e_i[at] = i;
        e_j[at] = j;
        e_score[at] = s[k];
        e_cov[at] = c[k];
        e_key[at] = score_key(s[k]);
        e_val[at] = (uint32_t)at;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void cls_gather_kernel(const uint32_t *__restrict__ order, uint64_t n_edges,
                                                              const uint32_t *__restrict__ e_i, const uint32_t *__restrict__ e_j,
                                                              const double *__restrict__ e_score, const double *__restrict__ e_cov,
                                                              uint32_t *__restrict__ o_i, uint32_t *__restrict__ o_j,
                                                              double *__restrict__ o_score, double *__restrict__ o_cov) {
  const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= n_edges) return;
  const uint32_t e = order[p];
  if (e >= n_edges) return;  // never: the values are a permutation of 0 .. n_edges - 1
  o_i[p] = e_i[e];
  o_j[p] = e_j[e];
  o_score[p] = e_score[e];
  o_cov[p] = e_cov[e];
}

}  // namespace

extern "C" int pa_classify_edges(pa_ctx *c, const double *d_score, const double *d_cov, uint32_t n, int agg_score, int agg_cov,
                                 double cov_min, uint64_t cap_edges, uint32_t *d_i, uint32_t *d_j, double *d_edge_score,
                                 double *d_edge_cov, uint64_t *n_edges) {
  PA_REQUIRE(c != nullptr && n_edges != nullptr, "pa_classify_edges: null argument");
  PA_REQUIRE(agg_ok(agg_score) && agg_ok(agg_cov), "pa_classify_edges: aggregators %d, %d (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)",
             agg_score, agg_cov);
  // the sort carries an edge's position as a u32 value: n (n - 1) / 2 < 2^32 holds up to n = 2^16
  PA_REQUIRE(n <= (1u << 16), "pa_classify_edges: %u genomes; the edge list is indexed with 32 bits, at most 65536 genomes", n);
  PA_REQUIRE(cov_min == cov_min, "pa_classify_edges: cov_min is NaN");
  *n_edges = 0;
  if (n < 2) return PA_OK;
  PA_REQUIRE(d_score && d_cov, "pa_classify_edges: null matrix");
  PA_HIP(hipSetDevice(c->device));
  const uint32_t nt = (n + kTile - 1) / kTile;
  const uint64_t n_counts = (uint64_t)n * nt;
  uint64_t E = 0;
  {
    ProfScope prof(c, PA_PROF_CLS_EDGES);
    PA_TRY(c->flags.reserve(n_counts * sizeof(uint32_t)));
    uint32_t *d_counts = c->flags.as<uint32_t>();
    // the tiles below the diagonal are not evaluated: their counts are zero
    PA_HIP(hipMemsetAsync(d_counts, 0, n_counts * sizeof(uint32_t), c->stream));
    const LaunchDim grid(nt, nt);
    PA_TRY(PA_LAUNCH(c, cls_edges_kernel<false>, grid, kThreads, 0, d_score, d_cov, n, nt, agg_score, agg_cov, cov_min, d_counts, 0ULL, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr));
    PA_TRY(pa_scan_total_u32(c, d_counts, d_counts, n_counts, c->slot<uint64_t>(kCompactTotal), &E));
    *n_edges = E;
    if (E > cap_edges) {
      pa_set_error("pa_classify_edges: %llu edges, caller gave room for %llu", (unsigned long long)E, (unsigned long long)cap_edges);
      return PA_E_CAPACITY;
    }
    if (E == 0) return PA_OK;
    PA_REQUIRE(d_i && d_j && d_edge_score && d_edge_cov, "pa_classify_edges: null output");
    PA_TRY(c->cls_i.reserve(E * sizeof(uint32_t)));
    PA_TRY(c->cls_j.reserve(E * sizeof(uint32_t)));
    PA_TRY(c->cls_score.reserve(E * sizeof(double)));
    PA_TRY(c->cls_cov.reserve(E * sizeof(double)));
    for (int b = 0; b < 2; ++b) {
      PA_TRY(c->cand_keys[b].reserve(E * sizeof(uint64_t)));
      PA_TRY(c->cand_vals[b].reserve(E * sizeof(uint32_t)));
    }
    PA_TRY(PA_LAUNCH(c, cls_edges_kernel<true>, grid, kThreads, 0, d_score, d_cov, n, nt, agg_score, agg_cov, cov_min, d_counts, E,
                     c->cls_i.as<uint32_t>(), c->cls_j.as<uint32_t>(), c->cls_score.as<double>(), c->cls_cov.as<double>(),
                     c->cand_keys[0].as<uint64_t>(), c->cand_vals[0].as<uint32_t>()));
  }
  ProfScope prof(c, PA_PROF_CLS_SORT);
  uint64_t *keys[2] = {c->cand_keys[0].as<uint64_t>(), c->cand_keys[1].as<uint64_t>()};
  uint32_t *vals[2] = {c->cand_vals[0].as<uint32_t>(), c->cand_vals[1].as<uint32_t>()};
  int which = 0;
  PA_TRY(pa_radix_sort_pairs(c, keys, vals, E, 0, 64, false, &which));
  return PA_LAUNCH(c, cls_gather_kernel, ceil_div(E, kThreads), kThreads, 0, vals[which], E, c->cls_i.as<uint32_t>(), c->cls_j.as<uint32_t>(),
                   c->cls_score.as<double>(), c->cls_cov.as<double>(), d_i, d_j, d_edge_score, d_edge_cov);
}
