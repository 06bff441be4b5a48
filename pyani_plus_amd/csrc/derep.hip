// derep.hip -- dereplicate-run on the device (gfx950, wave64): the threshold graph of a run as bit rows, the choice of
// one representative per group in rounds over that bit matrix, and every genome's representative.
//
// The reference has no such command: DESIGN.md section 7k has the contract, tests/derep_cases.py restates it
// independently, derep_host.cpp is the twin with the same bits and derep_rule.h states the rules once for both.
//
//   pa_derep_adjacency  derep_adjacency_kernel: one workgroup per 64 x 64 tile (ti <= tj) of the pairs, classify.hip's
//                       tiling and loader (pair_tile_dev.h): a wave per row of the tile, a lane per column, so that one
//                       ballot of the edge predicate is one word of the row.  The tile's 64 words go to LDS as well and
//                       lane t of the first wave gathers bit t of each: the word of row tj * 64 + t in the other
//                       triangle.  Every word of the matrix is written by exactly one plain vector store.
//   pa_derep_select     rounds of two small launches that the host enqueues PA_DEREP_BATCH at a time, in the manner of
//                       nj.hip; kDerepProgress holds the nodes settled so far and the rounds that had work, a round's
//                       first kernel returns at once when every node is settled, and the host reads the two words back
//                       once per batch.  One workgroup per word of 64 nodes, a wave per node, a lane per word of its row.
//     greedy  derep_greedy_pick_kernel: an undecided node with no undecided neighbour of lower index becomes a
//             representative (row & undecided over the words below it, a ballot per 64 words, left at the first hit);
//             derep_greedy_retire_kernel: the new representatives and every undecided node adjacent to one are settled.
//             The lowest undecided node always wins its round, and a node that wins has no earlier representative
//             beside it (that one would have retired it) while every earlier neighbour is retired, hence adjacent to an
//             earlier representative of its own: by induction the sequential rule, in at most n rounds.
//     cover   derep_cover_gain_kernel: gain = popcount(row & uncovered), the workgroup's best under the total order as
//             one 64-bit key (derep_rule.h), one candidate per workgroup; derep_cover_choose_kernel, one workgroup:
//             the best of the candidates, then uncovered &= ~row[best] -- or, once the best gain is 1, every node
//             still uncovered becomes a representative at once.
//   pa_derep_assign     derep_assign_kernel: one workgroup per node walks the set bits of its row that are
//                       representatives and reduces on (score, index) with block_reduce.
// No grid-wide barrier, no cooperative launch, no floating-point atomics; the integer atomicAdd of the settled count is
// order-free.  The results are the same bits run to run.
#include "pa_internal.h"

#include "block_reduce_dev.h"
#include "derep_rule.h"
#include "pair_tile_dev.h"
#include "wave_dev.h"

namespace {

using namespace pair_tile;  // kTile, kThreads, kPad, tile_values, and kRows: rows of a tile, or nodes of a word, per wave
static_assert(kTile == 64, "a tile's row is one word");

// kDerepProgress: [0] nodes settled (decided in greedy mode, covered in cover mode), [1] rounds that had work
constexpr uint32_t kSettled = 0, kRounds = 1;

__global__ __launch_bounds__(kThreads) void derep_adjacency_kernel(const double *__restrict__ score, const double *__restrict__ cov, uint32_t n,
                                                                   uint32_t W, int agg_score, int agg_cov, double min_score, double cov_min,
                                                                   uint64_t *__restrict__ bits) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  __shared__ double tile[kTile][kPad];
  __shared__ uint64_t s_word[kTile];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t a0 = ti * kTile, b0 = tj * kTile;
  double c[kRows], s[kRows];
  tile_values<true>(cov, n, a0, b0, agg_cov, tile, c);
  tile_values<true>(score, n, a0, b0, agg_score, tile, s);
  const uint32_t b = b0 + lane;
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const uint32_t r = wave * kRows + k, a = a0 + r;
    const bool adjacent = a < n && b < n && (a == b || derep::edge(s[k], c[k], min_score, cov_min));
    const uint64_t word = __ballot(adjacent);
    if (lane == 0) {
      s_word[r] = word;
      if (a < n) bits[(uint64_t)a * W + tj] = word;
    }
  }
  if (ti == tj) return;  // uniform; the diagonal tile holds both triangles
  __syncthreads();
  if (wave == 0 && b < n) {  // row b of the other triangle: bit r is adjacency(a0 + r, b)
    uint64_t word = 0;
#pragma unroll 8
    for (int r = 0; r < kTile; ++r) word |= ((s_word[r] >> lane) & 1ull) << r;
    bits[(uint64_t)b * W + ti] = word;
  }
}

// ---- greedy ----
// Workgroup = word wd of the nodes.  Writes newrep[wd]; reads undecided, which no workgroup of this launch writes.
__global__ __launch_bounds__(kThreads) void derep_greedy_pick_kernel(const uint64_t *__restrict__ bits, uint32_t n, uint32_t W,
                                                                     const uint64_t *__restrict__ undecided, uint64_t *__restrict__ newrep,
                                                                     uint32_t *__restrict__ progress) {
  if (progress[kSettled] >= n) return;  // written by the retire kernel only
  const uint32_t wd = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wd == 0 && threadIdx.x == 0) progress[kRounds] += 1;
  __shared__ uint32_t s_free[kTile];
  const uint64_t und = undecided[wd];
  if (und == 0) {  // uniform
    if (threadIdx.x == 0) newrep[wd] = 0;
    return;
  }
  for (int k = 0; k < kRows; ++k) {
    const uint32_t b = wave * kRows + k;
    bool is_free = false;
    if ((und >> b) & 1ull) {  // uniform in the wave
      const uint32_t p = wd * 64 + b;
      const uint64_t *row = bits + (uint64_t)p * W;
      is_free = true;
      for (uint32_t w0 = 0; w0 <= wd; w0 += 64) {
        const uint32_t w = w0 + lane;
        uint64_t lower = w <= wd ? row[w] & undecided[w] : 0ull;
        if (w == wd) lower &= (1ull << b) - 1ull;  // the nodes below p in its own word
        if (__ballot(lower != 0)) {
          is_free = false;
          break;
        }
      }
    }
    if (lane == 0) s_free[b] = is_free ? 1u : 0u;
  }
  __syncthreads();
  if (wave == 0) {
    const uint64_t word = __ballot(s_free[lane] != 0);
    if (lane == 0) newrep[wd] = word;
  }
}

// Workgroup = word wd.  Reads newrep (all of it) and its own word of undecided, which it alone writes.
__global__ __launch_bounds__(kThreads) void derep_greedy_retire_kernel(const uint64_t *__restrict__ bits, uint32_t n, uint32_t W,
                                                                       uint64_t *__restrict__ undecided, const uint64_t *__restrict__ newrep,
                                                                       uint8_t *__restrict__ is_rep, uint32_t *__restrict__ progress) {
  const uint32_t wd = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  __shared__ uint32_t s_hit[kTile];
  const uint64_t und = undecided[wd];
  if (und == 0) return;  // uniform: every round after the last, too
  const uint64_t fresh = newrep[wd] & und;
  for (int k = 0; k < kRows; ++k) {
    const uint32_t b = wave * kRows + k;
    bool hit = false;
    if (((und & ~fresh) >> b) & 1ull) {  // uniform in the wave
      const uint64_t *row = bits + (uint64_t)(wd * 64 + b) * W;
      for (uint32_t w0 = 0; w0 < W; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint64_t beside = w < W ? row[w] & newrep[w] : 0ull;
        if (__ballot(beside != 0)) {
          hit = true;
          break;
        }
      }
    }
    if (lane == 0) s_hit[b] = hit ? 1u : 0u;
  }
  __syncthreads();
  if (wave != 0) return;
  const uint64_t retired = __ballot(s_hit[lane] != 0);
  const uint32_t p = wd * 64 + lane;
  if (((fresh >> lane) & 1ull) && p < n) is_rep[p] = 1;
  if (lane == 0) {
    const uint64_t settled = fresh | retired;
    undecided[wd] = und & ~settled;
    atomicAdd(&progress[kSettled], (uint32_t)__popcll(und & settled));
  }
}

// ---- cover ----
__global__ __launch_bounds__(kThreads) void derep_cover_gain_kernel(const uint64_t *__restrict__ bits, uint32_t n, uint32_t W,
                                                                    const uint64_t *__restrict__ uncovered, uint64_t *__restrict__ cand,
                                                                    uint32_t *__restrict__ progress) {
  if (progress[kSettled] >= n) return;  // written by the choose kernel only
  const uint32_t wd = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wd == 0 && threadIdx.x == 0) progress[kRounds] += 1;
  __shared__ uint64_t s_best[kThreads];
  const uint64_t own = uncovered[wd];
  uint64_t best = 0;
  for (int k = 0; k < kRows; ++k) {
    const uint32_t b = wave * kRows + k, p = wd * 64 + b;
    if (p >= n) break;  // uniform in the wave
    const uint64_t *row = bits + (uint64_t)p * W;
    uint32_t gain = 0;
    for (uint32_t w = lane; w < W; w += 64) gain += (uint32_t)__popcll(row[w] & uncovered[w]);
    gain = pa_dev::wave_sum_dpp(gain);
    const uint64_t key = derep::cover_key(gain, (own >> b) & 1ull, p);
    best = key > best ? key : best;
  }
  best = pa_dev::block_reduce<kThreads>(best, s_best, [](uint64_t x, uint64_t y) { return x > y ? x : y; });
  if (threadIdx.x == 0) cand[wd] = best;
}

__global__ __launch_bounds__(kThreads) void derep_cover_choose_kernel(const uint64_t *__restrict__ bits, uint32_t n, uint32_t W,
                                                                      uint64_t *__restrict__ uncovered, const uint64_t *__restrict__ cand,
                                                                      uint8_t *__restrict__ is_rep, uint32_t *__restrict__ progress) {
  if (progress[kSettled] >= n) return;  // this workgroup is its only writer
  __shared__ uint64_t s_best[kThreads];
  __shared__ uint32_t s_sum[kThreads];
  uint64_t best = 0;
  for (uint32_t w = threadIdx.x; w < W; w += kThreads) best = cand[w] > best ? cand[w] : best;
  best = pa_dev::block_reduce<kThreads>(best, s_best, [](uint64_t x, uint64_t y) { return x > y ? x : y; });
  const uint32_t gain = derep::cover_key_gain(best), p = derep::cover_key_node(best);
  if (gain == 0 || p >= n) return;  // a bit matrix without its diagonal: the host gives up after n rounds
  if (gain == 1) {  // every node still uncovered covers itself alone
    for (uint32_t w = threadIdx.x; w < W; w += kThreads) {
      for (uint64_t m = uncovered[w]; m; m &= m - 1) {
        const uint32_t q = w * 64 + (uint32_t)__builtin_ctzll(m);
        if (q < n) is_rep[q] = 1;
      }
      uncovered[w] = 0;
    }
    if (threadIdx.x == 0) progress[kSettled] = n;
    return;
  }
  const uint64_t *row = bits + (uint64_t)p * W;
  uint32_t newly = 0;
  for (uint32_t w = threadIdx.x; w < W; w += kThreads) {
    const uint64_t u = uncovered[w], r = row[w];
    newly += (uint32_t)__popcll(u & r);
    uncovered[w] = u & ~r;
  }
  newly = pa_dev::block_reduce<kThreads>(newly, s_sum, [](uint32_t x, uint32_t y) { return x + y; });
  if (threadIdx.x == 0) {
    is_rep[p] = 1;
    progress[kSettled] += newly;
  }
}

// every node undecided or uncovered: ones below n, zeros in the padding
__global__ __launch_bounds__(kThreads) void derep_all_nodes_kernel(uint32_t n, uint32_t W, uint64_t *__restrict__ words) {
  const uint32_t w = blockIdx.x * kThreads + threadIdx.x;
  if (w >= W) return;
  const uint32_t first = w * 64;
  words[w] = n - first >= 64 ? ~0ull : (~0ull >> (64 - (n - first)));
}

__global__ __launch_bounds__(kThreads) void derep_count_kernel(const uint8_t *__restrict__ is_rep, uint32_t n, uint32_t *__restrict__ count) {
  __shared__ uint32_t s_sum[kThreads];
  uint32_t mine = 0;
  for (uint32_t p = threadIdx.x; p < n; p += kThreads) mine += is_rep[p] ? 1u : 0u;
  mine = pa_dev::block_reduce<kThreads>(mine, s_sum, [](uint32_t x, uint32_t y) { return x + y; });
  if (threadIdx.x == 0) *count = mine;
}

// ---- assignment ----
struct PickLds {
  double score[kThreads];
  uint32_t rep[kThreads], lane[kThreads];
};

__global__ __launch_bounds__(kThreads) void derep_assign_kernel(const double *__restrict__ S, uint32_t n, uint32_t W, int agg_score,
                                                                const uint64_t *__restrict__ bits, const uint8_t *__restrict__ is_rep,
                                                                uint32_t *__restrict__ rep, double *__restrict__ rep_score) {
  const uint32_t p = blockIdx.x;
  if (p >= n) return;
  if (is_rep[p]) {  // uniform
    if (threadIdx.x == 0) {
      const double own = S[(uint64_t)p * n + p];
      rep[p] = p;
      rep_score[p] = derep::pair_value(agg_score, p, p, own, own);
    }
    return;
  }
  __shared__ PickLds s;
  derep::Pick best{__builtin_nan(""), derep::kNone};
  const uint64_t *row = bits + (uint64_t)p * W;
  for (uint32_t w = threadIdx.x; w < W; w += kThreads)
    for (uint64_t m = row[w]; m; m &= m - 1) {
      const uint32_t q = w * 64 + (uint32_t)__builtin_ctzll(m);
      if (q >= n || q == p || !is_rep[q]) continue;
      const derep::Pick c{derep::pair_value(agg_score, p, q, S[(uint64_t)p * n + q], S[(uint64_t)q * n + p]), q};
      if (c.score == c.score && derep::better(c, best)) best = c;
    }
  s.score[threadIdx.x] = best.score;
  s.rep[threadIdx.x] = best.rep;  // visible after the barrier that follows block_reduce's own store
  const uint32_t winner = pa_dev::block_reduce<kThreads>((uint32_t)threadIdx.x, s.lane, [](uint32_t i, uint32_t j) {
    return derep::better(derep::Pick{s.score[j], s.rep[j]}, derep::Pick{s.score[i], s.rep[i]}) ? j : i;
  });
  if (threadIdx.x == 0) {
    rep[p] = s.rep[winner];
    rep_score[p] = s.score[winner];
  }
}

}  // namespace

extern "C" int pa_derep_adjacency(pa_ctx *c, const double *d_S, const double *d_C, uint32_t n, int agg_score, int agg_cov, double min_score,
                                  double cov_min, uint64_t *d_bits) {
  PA_REQUIRE(c != nullptr, "pa_derep_adjacency: null context");
  PA_TRY(derep::check_adjacency(d_S, d_C, n, agg_score, agg_cov, min_score, cov_min, d_bits));
  PA_HIP(hipSetDevice(c->device));
  const uint32_t W = derep::words(n);
  return PA_LAUNCH(c, derep_adjacency_kernel, LaunchDim(W, W), kThreads, 0, d_S, d_C, n, W, agg_score, agg_cov, min_score, cov_min, d_bits);
}

extern "C" int pa_derep_select(pa_ctx *c, const uint64_t *d_bits, uint32_t n, int mode, uint8_t *d_is_rep, uint32_t *n_reps, uint32_t *n_rounds) {
  PA_REQUIRE(c != nullptr, "pa_derep_select: null context");
  PA_TRY(derep::check_select(d_bits, n, mode, d_is_rep, n_reps));
  PA_HIP(hipSetDevice(c->device));
  const uint32_t W = derep::words(n);
  // the workspace: the undecided / uncovered nodes, then the new representatives / the workgroups' candidates
  uint64_t *d_open, *d_aux;
  PA_TRY(pa_carve(c->derep_work, "derep_work", [&](Carve &k) { d_open = k.take<uint64_t>(W); d_aux = k.take<uint64_t>(W); }));
  uint32_t *d_progress = c->slot<uint32_t>(kDerepProgress);
  PA_HIP(hipMemsetAsync(d_progress, 0, kDerepProgress.bytes(), c->stream));
  PA_HIP(hipMemsetAsync(d_is_rep, 0, n, c->stream));
  PA_TRY(PA_LAUNCH(c, derep_all_nodes_kernel, ceil_div(W, kThreads), kThreads, 0, n, W, d_open));
  uint32_t progress[2] = {0, 0};
  // each round settles at least one node, so n rounds are enough; the host enqueues, the device decides
  for (uint64_t enqueued = 0; progress[kSettled] < n && enqueued < n; enqueued += PA_DEREP_BATCH) {
    for (int r = 0; r < PA_DEREP_BATCH; ++r) {
      if (mode == PA_DEREP_GREEDY) {
        PA_TRY(PA_LAUNCH(c, derep_greedy_pick_kernel, W, kThreads, 0, d_bits, n, W, (const uint64_t *)d_open, d_aux, d_progress));
        PA_TRY(PA_LAUNCH(c, derep_greedy_retire_kernel, W, kThreads, 0, d_bits, n, W, d_open, (const uint64_t *)d_aux, d_is_rep, d_progress));
      } else {
        PA_TRY(PA_LAUNCH(c, derep_cover_gain_kernel, W, kThreads, 0, d_bits, n, W, (const uint64_t *)d_open, d_aux, d_progress));
        PA_TRY(PA_LAUNCH(c, derep_cover_choose_kernel, 1, kThreads, 0, d_bits, n, W, d_open, (const uint64_t *)d_aux, d_is_rep, d_progress));
      }
    }
    PA_TRY(pa_read_back(c, (const uint32_t *)d_progress, progress, 2));
  }
  PA_REQUIRE(progress[kSettled] >= n, "pa_derep_select: %u nodes are in no row's neighbourhood: the diagonal of the bit matrix is not set",
             n - progress[kSettled]);
  // the count goes through the settled word, which nothing reads any more
  PA_TRY(PA_LAUNCH(c, derep_count_kernel, 1, kThreads, 0, (const uint8_t *)d_is_rep, n, d_progress));
  PA_TRY(pa_read_back(c, (const uint32_t *)d_progress, n_reps));
  if (n_rounds) *n_rounds = progress[kRounds];
  return PA_OK;
}

extern "C" int pa_derep_assign(pa_ctx *c, const double *d_S, uint32_t n, int agg_score, const uint64_t *d_bits, const uint8_t *d_is_rep,
                               uint32_t *d_rep, double *d_rep_score) {
  PA_REQUIRE(c != nullptr, "pa_derep_assign: null context");
  PA_TRY(derep::check_assign(d_S, n, agg_score, d_bits, d_is_rep, d_rep, d_rep_score));
  PA_HIP(hipSetDevice(c->device));
  return PA_LAUNCH(c, derep_assign_kernel, n, kThreads, 0, d_S, n, derep::words(n), agg_score, d_bits, d_is_rep, d_rep, d_rep_score);
}
