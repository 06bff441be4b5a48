// subst.hip -- phylo-run on the device (gfx950, wave64): the three substitution counts of every pair of an alignment's
// rows, unweighted and under the column weights of a batch of bootstrap replicates, and the distance matrices of the
// models p, JC69 and K80.
//
// The definitions are this project's own: include/pyani_hip.h and DESIGN.md section 7m have the contract,
// tests/subst_cases.py restates it independently, subst_host.cpp has the twins, subst_rule.h the code table, the
// logarithm and the distance of both sides.  Every count is an integer sum, so the order of the additions (and the
// atomics of the split form) cannot show in a result.
//
// The rows are packed by pa_msa_pack with pa_subst_code's table at bits = 3: four planes a word, plane 0 the base
// within the class, plane 1 the class, plane 2 "is a nucleotide", plane 3 the non-gap plane, which equals plane 2
// because every code but 0 has bit 2.  The kernels stage planes 0, 1 and 3 only.  Per pair and 32 columns:
//   valid = q3 & s3                                      v_and
//   tv = (q1 ^ s1) & valid,  d0 = (q0 ^ s0) & valid      v_bitop3 each
//   ts = d0 & ~tv                                        v_bitop3 (= valid & ~(q1 ^ s1) & (q0 ^ s0))
//   V += popcount(valid), S += popcount(ts), T += popcount(tv)    three v_bcnt_u32_b32, which accumulate
// seven VALU instructions: with the two exclusive-ors as instructions of their own it would be eight, and v_bitop3
// takes each together with the AND that follows it.  Under weights the three words are formed once and
//   count += popcount(word & W_beta) << beta   for beta < nb      v_and, v_bcnt, v_lshl_add each
// as msa_boot.hip does for its two, with the weight planes, the workspace and the batch on the grid's z axis of
// msa_boot_dev.h.
#include "msa_boot_dev.h"

#include "msa_boot_rule.h"
#include "pa_host.h"
#include "subst_rule.h"

namespace {
using namespace msa_tile;

constexpr int kLayoutPlanes = PA_SUBST_BITS + 1;  // what pa_msa_pack wrote a word
constexpr uint32_t kXorAnd = (0xf0u ^ 0xccu) & 0xaau;  // (a ^ b) & c

// the three words of the pair (query a, subject b) from the staged planes: [0] base bit, [1] class bit, [2] non-gap
__device__ inline void subst_words(const uint32_t (&qv)[3][4], const uint32_t (&sv)[3][4], int a, int b, uint32_t &valid, uint32_t &ts, uint32_t &tv) {
  valid = qv[2][a] & sv[2][b];
  tv = bitop3_t<kXorAnd>(qv[1][a], sv[1][b], valid);
  ts = bitop3_t<kAndNot>(tv, bitop3_t<kXorAnd>(qv[0][a], sv[0][b], valid), 0u);
}

// One block: a 64 x 64 tile of the pairs of rows [0, n), on or above the diagonal, over the words of blockIdx.y's slice
__global__ __launch_bounds__(kThreads) void subst_pairs_kernel(const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t n_words,
                                                               uint32_t words_per_split, uint32_t n, uint32_t n_tiles, int accumulate,
                                                               uint32_t *__restrict__ valid, uint32_t *__restrict__ ts, uint32_t *__restrict__ tv) {
  __shared__ Stage<3> stage;
  const TileGeom g = tile_geom(n_tiles, 1, n_words, words_per_split);
  const Ranges r{0u, n, 0u, n};
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  uint32_t v[4][4] = {{0}}, s[4][4] = {{0}}, t[4][4] = {{0}};
  for (uint32_t wc = g.w_lo; wc < g.w_hi; wc += kChunk) {
    __syncthreads();
    stage_three_planes<kLayoutPlanes, 0, 1, 3>(stage, planes, n_pad, wc, g, r, tid);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      uint32_t qv[3][4], sv[3][4];
      load_rows<3>(stage, k, tx, ty, qv, sv);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          uint32_t wv, ws, wt;
          subst_words(qv, sv, a, b, wv, ws, wt);
          v[a][b] += __builtin_popcount(wv);
          s[a][b] += __builtin_popcount(ws);
          t[a][b] += __builtin_popcount(wt);
        }
      }
    }
  }
  write_counts3(v, s, t, g, r, tx, ty, accumulate, valid, ts, tv);
}

// The same for replicate blockIdx.z under its weight planes; valid, ts and tv: the replicates' n x n matrices one after
// the other
__global__ __launch_bounds__(kThreads) void subst_boot_pairs_kernel(const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t n_words,
                                                                    uint32_t words_per_split, uint32_t n, uint32_t n_tiles,
                                                                    const uint32_t *__restrict__ wplanes, uint32_t nb, int accumulate,
                                                                    uint32_t *__restrict__ valid, uint32_t *__restrict__ ts, uint32_t *__restrict__ tv) {
  __shared__ Stage<3> stage;
  __shared__ uint32_t sw[kChunk][kMaxBits];
  const TileGeom g = tile_geom(n_tiles, 1, n_words, words_per_split);
  const Ranges r{0u, n, 0u, n};
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  const uint32_t *wp = wplanes + (uint64_t)blockIdx.z * n_words * kMaxBits;
  uint32_t v[4][4] = {{0}}, s[4][4] = {{0}}, t[4][4] = {{0}};
  for (uint32_t wc = g.w_lo; wc < g.w_hi; wc += kChunk) {
    __syncthreads();
    stage_three_planes<kLayoutPlanes, 0, 1, 3>(stage, planes, n_pad, wc, g, r, tid);
    stage_weight_words(sw, wp, wc, g.w_hi, tid);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      uint32_t wv[4][4], ws[4][4], wt[4][4];
      {
        uint32_t qv[3][4], sv[3][4];
        load_rows<3>(stage, k, tx, ty, qv, sv);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int b = 0; b < 4; ++b) subst_words(qv, sv, a, b, wv[a][b], ws[a][b], wt[a][b]);
        }
      }
#pragma unroll 1
      for (uint32_t beta = 0; beta < nb; ++beta) {
        const uint32_t W = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[k][beta]);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            v[a][b] += (uint32_t)__builtin_popcount(wv[a][b] & W) << beta;
            s[a][b] += (uint32_t)__builtin_popcount(ws[a][b] & W) << beta;
            t[a][b] += (uint32_t)__builtin_popcount(wt[a][b] & W) << beta;
          }
        }
      }
    }
  }
  const uint64_t at = (uint64_t)blockIdx.z * n * n;
  write_counts3(v, s, t, g, r, tx, ty, accumulate, valid + at, ts + at, tv + at);
}

// msa_mirror_kernel for three counts a pair: (r, c) with tile(c) < tile(r) takes (c, r); blockIdx.z: which matrix
__global__ __launch_bounds__(kThreads) void subst_mirror_kernel(uint32_t n, uint32_t *__restrict__ valid, uint32_t *__restrict__ ts,
                                                                uint32_t *__restrict__ tv) {
  const uint64_t at = (uint64_t)blockIdx.z * n * n;
  valid += at;
  ts += at;
  tv += at;
  for (uint32_t r = blockIdx.y; r < n; r += gridDim.y) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= (r / kTile) * kTile) continue;
    valid[(uint64_t)r * n + c] = valid[(uint64_t)c * n + r];
    ts[(uint64_t)r * n + c] = ts[(uint64_t)c * n + r];
    tv[(uint64_t)r * n + c] = tv[(uint64_t)c * n + r];
  }
}

// D[m][i][j] of subst_rule.h's distance, a lane per cell of the n_mats matrices that start at valid, ts, tv and D;
// undefined[2 m], undefined[2 m + 1]: the pairs i < j of matrix m without a shared nucleotide column, and the saturated
__global__ __launch_bounds__(kThreads) void subst_distances_kernel(const uint32_t *__restrict__ valid, const uint32_t *__restrict__ ts,
                                                                   const uint32_t *__restrict__ tv, uint32_t n, uint64_t cells, int model,
                                                                   double missing, double *__restrict__ D, unsigned long long *__restrict__ undefined) {
  const uint64_t nn = (uint64_t)n * n;
  for (uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x; at < cells; at += (uint64_t)gridDim.x * kThreads) {
    const uint64_t mat = at / nn, cell = at - mat * nn;
    const uint32_t i = (uint32_t)(cell / n), j = (uint32_t)(cell % n);
    int why;
    D[at] = subst::distance(i, j, valid[at], ts[at], tv[at], model, missing, &why);
    // integer atomics, so no order shows; the lanes of the matrix of the wave's first active lane vote and that lane adds
    // for them, a lane of another matrix (a wave spans two at the most when n >= 8) adds for itself
    const int kind = i < j ? why : subst::kDefined;
    const uint32_t m32 = (uint32_t)mat, lead_mat = (uint32_t)__builtin_amdgcn_readfirstlane((int)m32);
    const bool leads = (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)__ballot(1)) - 1u;
    for (int what = subst::kNoColumns; what <= subst::kSaturated; ++what) {
      const unsigned long long votes = __ballot(kind == what && m32 == lead_mat);
      if (leads && votes) atomicAdd(&undefined[2 * lead_mat + (what - 1)], (unsigned long long)__popcll(votes));
      if (kind == what && m32 != lead_mat) atomicAdd(&undefined[2 * m32 + (what - 1)], 1ull);
    }
  }
}

constexpr uint32_t kDistanceBatch = kSubstUndefined.words / 4;  // matrices a launch of the distances: two 64-bit words each

// pa_msa_subst_counts behind its checks; the caller waits for the stream, which still reads h_weights
int subst_counts_device(pa_ctx *c, const uint32_t *d_planes, uint32_t n, uint64_t n_cols, const uint8_t *h_weights, uint32_t n_reps, uint32_t nb,
                        uint32_t *d_valid, uint32_t *d_ts, uint32_t *d_tv) {
  ProfScope prof(c, PA_PROF_MSA_PAIRS);
  const uint32_t n_words = (uint32_t)n_words_of(n_cols);
  const uint64_t nn = (uint64_t)n * n;
  uint32_t *const out[3] = {d_valid, d_ts, d_tv};
  if (n_words == 0) {
    for (uint32_t *p : out) PA_HIP(hipMemsetAsync(p, 0, nn * n_reps * 4u, c->stream));
    return PA_OK;
  }
  const uint32_t nt = (n + kTile - 1) / kTile;
  const uint64_t tiles = (uint64_t)nt * (nt + 1) / 2;
  PA_REQUIRE(tiles < (1ull << 31), "pa_msa_subst_counts: %llu tiles", (unsigned long long)tiles);
  const uint32_t np = n_pad_of(n);
  Work w{};
  if (h_weights) PA_TRY(pa_carve(c->boot_work, "boot_work", [&](Carve &k) { w.layout(k, n_words); }));
  for (uint32_t r0 = 0; r0 < n_reps; r0 += kBatch) {
    const uint32_t count = std::min(kBatch, n_reps - r0);
    if (h_weights) PA_TRY(upload_weight_planes(c, w, h_weights, r0, count, n_cols, n_words));
    const ColumnSplit split = split_columns(c, tiles * count, n_words);
    const int accumulate = split.splits > 1;
    uint32_t *valid = d_valid + (uint64_t)r0 * nn, *ts = d_ts + (uint64_t)r0 * nn, *tv = d_tv + (uint64_t)r0 * nn;
    if (accumulate)
      for (uint32_t *p : {valid, ts, tv}) PA_HIP(hipMemsetAsync(p, 0, nn * count * 4u, c->stream));
    const LaunchDim grid(tiles, split.splits, count);
    if (h_weights)
      PA_TRY(PA_LAUNCH(c, subst_boot_pairs_kernel, grid, kThreads, 0, d_planes, np, n_words, split.words_per_split, n, nt, (const uint32_t *)w.wplanes, nb,
                       accumulate, valid, ts, tv));
    else
      PA_TRY(PA_LAUNCH(c, subst_pairs_kernel, grid, kThreads, 0, d_planes, np, n_words, split.words_per_split, n, nt, accumulate, valid, ts, tv));
    if (nt > 1)
      PA_TRY(PA_LAUNCH(c, subst_mirror_kernel, LaunchDim((n + kThreads - 1) / kThreads, n < 65535u ? n : 65535u, count), kThreads, 0, n, valid, ts, tv));
  }
  return PA_OK;
}

}  // namespace

extern "C" {

int pa_msa_subst_counts(pa_ctx *c, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights, uint32_t n_reps,
                        uint32_t *d_valid, uint32_t *d_ts, uint32_t *d_tv) {
  PA_REQUIRE(c != nullptr, "pa_msa_subst_counts: null context");
  PA_REQUIRE(n_rows == 0 || n_reps == 0 || (d_valid && d_ts && d_tv && (d_planes || n_cols == 0)), "pa_msa_subst_counts: null argument");
  PA_REQUIRE(h_weights || n_reps <= 1, "pa_msa_subst_counts: %u replicates without weights; 1 without them", n_reps);
  PA_REQUIRE(n_cols < (1ull << 32), "pa_msa_subst_counts: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols);
  PA_REQUIRE(n_rows <= 65535, "pa_msa_subst_counts: %u rows; at most 65535", n_rows);
  if (n_rows == 0 || n_reps == 0) return PA_OK;
  uint32_t max_weight = 0;
  if (h_weights) PA_TRY(boot::check_weights("pa_msa_subst_counts", h_weights, n_cols, n_reps, &max_weight));
  PA_HIP(hipSetDevice(c->device));
  const int status = subst_counts_device(c, d_planes, n_rows, n_cols, h_weights, n_reps, boot::weight_planes(max_weight), d_valid, d_ts, d_tv);
  const hipError_t waited = hipStreamSynchronize(c->stream);  // copies from h_weights may still be queued
  if (status != PA_OK) return status;
  PA_HIP(waited);
  return PA_OK;
}

int pa_subst_distances(pa_ctx *c, const uint32_t *d_valid, const uint32_t *d_ts, const uint32_t *d_tv, uint32_t n, uint32_t n_reps, int model,
                       double missing, double *d_D, uint64_t *h_undefined) {
  PA_REQUIRE(c != nullptr, "pa_subst_distances: null context");
  PA_REQUIRE(n_reps == 0 || (h_undefined && (n == 0 || (d_valid && d_ts && d_tv && d_D))), "pa_subst_distances: null argument");
  PA_REQUIRE(subst::known_model(model), "pa_subst_distances: unknown model %d (0: p, 1: jc69, 2: k80)", model);
  PA_REQUIRE(missing >= 0.0 && missing <= 1.79769313486231570815e308, "pa_subst_distances: the distance of a pair without columns must be finite and not negative");
  for (uint64_t m = 0; m < 2ull * n_reps; ++m) h_undefined[m] = 0;
  const uint64_t nn = (uint64_t)n * n;
  if (nn == 0 || n_reps == 0) return PA_OK;
  PA_HIP(hipSetDevice(c->device));
  ProfScope prof(c, PA_PROF_MSA_BOOT_DIST);
  unsigned long long *d_undefined = c->slot<unsigned long long>(kSubstUndefined);
  for (uint32_t r0 = 0; r0 < n_reps; r0 += kDistanceBatch) {
    const uint32_t count = std::min(kDistanceBatch, n_reps - r0);
    const uint64_t at = (uint64_t)r0 * nn, cells = nn * count;
    PA_HIP(hipMemsetAsync(d_undefined, 0, kSubstUndefined.bytes(), c->stream));
    PA_TRY(PA_LAUNCH(c, subst_distances_kernel, stride_blocks(cells), kThreads, 0, d_valid + at, d_ts + at, d_tv + at, n, cells, model, missing, d_D + at,
                     d_undefined));
    unsigned long long got[2 * kDistanceBatch] = {};
    PA_TRY(pa_read_back(c, (const unsigned long long *)d_undefined, got, 2u * count));
    for (uint32_t m = 0; m < 2u * count; ++m) h_undefined[2ull * r0 + m] = got[m];
  }
  return PA_OK;
}

}  // extern "C"
