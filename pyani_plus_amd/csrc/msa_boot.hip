// msa_boot.hip -- bootstrap-run on the device (gfx950, wave64): the pair counts of an alignment under the column
// weights of a batch of bootstrap replicates, and the replicates' distance matrices.
//
// The definitions are this project's own: include/pyani_hip.h and DESIGN.md section 7l have the contract,
// tests/bootstrap_cases.py restates it independently, msa_boot_host.cpp has the twins and the check of the weights,
// msa_boot_rule.h the formulas of both sides.  Every count is an integer sum, so the order of the additions (and the
// atomics of the split form) cannot show in a result.
//
// Bit-sliced weights.  A replicate's weights w[c] < 2^nb become nb planes of words: bit j of word w of plane beta is bit
// beta of w[32 w + j].  With eq and both of a pair and 32 columns as msa.hip forms them (msa_tile_dev.h),
//   M += popcount(eq & W_beta) << beta,   B += popcount(both & W_beta) << beta      for beta < nb:
// v_and, v_bcnt, v_lshl_add each, 6 nb VALU instructions on top of the b + 2 that form eq and both.  The weight words are
// the same for every pair of a tile: they are staged beside the tile's rows, 8 per word, and read back as one broadcast
// LDS read that is made wave-uniform (an SGPR operand of the v_and).
//
// One launch takes up to PA_MSA_BOOT_BATCH replicates on the grid's z axis: eq is formed again per replicate, which is
// the small part (b + 2 of b + 2 + 6 nb), and a register tile stays at one replicate's 32 accumulators.  The batch on the
// grid is what fills the device when the genomes are few: at N = 100 there are 3 tiles, and 32 replicates make 96
// blocks before the columns have to be split and added with atomics.
#include <cstdlib>

#include "msa_boot_dev.h"

#include "msa_boot_rule.h"
#include "pa_host.h"

namespace {
using namespace msa_tile;

// One block: replicate blockIdx.z, a 64 x 64 tile of the pairs of rows [0, n) over the words of blockIdx.y's slice, as
// msa_pairs_kernel in its symmetric form.  match and both: the replicates' n x n matrices one after the other.
template <int P>
__global__ __launch_bounds__(kThreads) void msa_boot_pairs_kernel(const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t n_words,
                                                                  uint32_t words_per_split, uint32_t n, uint32_t n_tiles,
                                                                  const uint32_t *__restrict__ wplanes, uint32_t nb, int accumulate,
                                                                  uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
  __shared__ Stage<P> stage;
  __shared__ uint32_t sw[kChunk][kMaxBits];
  const TileGeom g = tile_geom(n_tiles, 1, n_words, words_per_split);
  const Ranges r{0u, n, 0u, n};
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  const uint32_t *wp = wplanes + (uint64_t)blockIdx.z * n_words * kMaxBits;
  uint32_t m[4][4] = {{0}}, bo[4][4] = {{0}};
  for (uint32_t wc = g.w_lo; wc < g.w_hi; wc += kChunk) {
    __syncthreads();
    stage_words<P>(stage, planes, n_pad, wc, g, r, tid);
    stage_weight_words(sw, wp, wc, g.w_hi, tid);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      uint32_t eq[4][4], bt[4][4];
      {
        uint32_t qv[P][4], sv[P][4];
        load_rows<P>(stage, k, tx, ty, qv, sv);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            eq[a][b] = eq_word<P>(qv, sv, a, b);
            bt[a][b] = both_word<P>(qv, sv, a, b);
          }
        }
      }
#pragma unroll 1
      for (uint32_t beta = 0; beta < nb; ++beta) {
        const uint32_t W = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[k][beta]);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            m[a][b] += (uint32_t)__builtin_popcount(eq[a][b] & W) << beta;
            bo[a][b] += (uint32_t)__builtin_popcount(bt[a][b] & W) << beta;
          }
        }
      }
    }
  }
  const uint64_t at = (uint64_t)blockIdx.z * n * n;
  write_counts(m, bo, g, r, tx, ty, accumulate, match + at, both + at);
}

// D[rep][i][j] of msa_boot_rule.h's distance, a lane per cell
__global__ __launch_bounds__(kThreads) void msa_boot_distances_kernel(const uint32_t *__restrict__ match, const uint32_t *__restrict__ both, uint32_t n,
                                                                      uint64_t cells, double missing, double *__restrict__ D) {
  const uint64_t nn = (uint64_t)n * n;
  for (uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x; at < cells; at += (uint64_t)gridDim.x * kThreads) {
    const uint64_t base = at / nn * nn, cell = at - base;
    const uint32_t i = (uint32_t)(cell / n), j = (uint32_t)(cell % n);
    D[at] = boot::distance(i, j, match[at], both[at], both[base + (uint64_t)i * n + i], both[base + (uint64_t)j * n + j], missing);
  }
}

// pa_msa_boot_counts behind its checks; the caller waits for the stream, which still reads h_weights
int boot_counts_device(pa_ctx *c, const uint32_t *d_planes, uint32_t n, uint64_t n_cols, uint32_t bits, const uint8_t *h_weights, uint32_t n_reps,
                       uint32_t nb, uint32_t *d_match, uint32_t *d_both) {
  ProfScope prof(c, PA_PROF_MSA_BOOT);
  const uint32_t n_words = (uint32_t)n_words_of(n_cols);
  const uint64_t nn = (uint64_t)n * n;
  if (n_words == 0) {
    PA_HIP(hipMemsetAsync(d_match, 0, nn * n_reps * 4u, c->stream));
    PA_HIP(hipMemsetAsync(d_both, 0, nn * n_reps * 4u, c->stream));
    return PA_OK;
  }
  Work w;
  PA_TRY(pa_carve(c->boot_work, "boot_work", [&](Carve &k) { w.layout(k, n_words); }));
  const uint32_t nt = (n + kTile - 1) / kTile;
  const uint64_t tiles = (uint64_t)nt * (nt + 1) / 2;
  PA_REQUIRE(tiles < (1ull << 31), "pa_msa_boot_counts: %llu tiles", (unsigned long long)tiles);
  const uint32_t np = n_pad_of(n);
  for (uint32_t r0 = 0; r0 < n_reps; r0 += kBatch) {
    const uint32_t count = std::min(kBatch, n_reps - r0);
    PA_TRY(upload_weight_planes(c, w, h_weights, r0, count, n_cols, n_words));
    const ColumnSplit split = split_columns(c, tiles * count, n_words);
    const int accumulate = split.splits > 1;
    uint32_t *match = d_match + (uint64_t)r0 * nn, *both = d_both + (uint64_t)r0 * nn;
    if (accumulate) {
      PA_HIP(hipMemsetAsync(match, 0, nn * count * 4u, c->stream));
      PA_HIP(hipMemsetAsync(both, 0, nn * count * 4u, c->stream));
    }
    const LaunchDim grid(tiles, split.splits, count);
    int status = PA_OK;
    auto launch_pairs = [&](auto planes) {
      status = PA_LAUNCH(c, msa_boot_pairs_kernel<planes()>, grid, kThreads, 0, d_planes, np, n_words, split.words_per_split, n, nt,
                         (const uint32_t *)w.wplanes, nb, accumulate, match, both);
    };
    if (!dispatch_value(bits + 1, value_list<2, 7>{}, launch_pairs)) launch_pairs(std::integral_constant<int, 9>{});
    PA_TRY(status);
    if (nt > 1) PA_TRY(launch_mirror(c, n, count, match, both));
  }
  return PA_OK;
}

}  // namespace

extern "C" {

int pa_msa_boot_weights(uint64_t seed, uint64_t n_cols, uint64_t first, uint64_t count, uint8_t *h_weights) {
  PA_REQUIRE(count == 0 || n_cols == 0 || h_weights, "pa_msa_boot_weights: null argument");
  PA_REQUIRE(n_cols < (1ull << 32), "pa_msa_boot_weights: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols);
  if (count == 0 || n_cols == 0) return PA_OK;
  // the tools build can lower the limit, so that the refusal can be met: 256 hits on one column do not happen by chance
  const char *lowered = PA_TOOL_ENV("PA_BOOT_WEIGHT_LIMIT");
  const uint32_t limit = lowered ? std::min<uint32_t>(boot::kMaxWeight, (uint32_t)atoi(lowered)) : boot::kMaxWeight;
  return pa_host_guard("pa_msa_boot_weights", [&]() -> int {
    constexpr uint64_t kNone = ~0ull;
    std::vector<uint64_t> over(count, kNone);  // per replicate, the column of the first draw that went past the limit
    HostPool::get().run(pa_host_threads(count * n_cols, 1u << 18, 0), [&](uint32_t id, uint32_t n_workers) {
      for (uint64_t r = id; r < count; r += n_workers) {
        uint8_t *row = h_weights + r * n_cols;
        memset(row, 0, n_cols);
        const uint64_t base = boot::replicate_base(seed, first + r);
        for (uint64_t t = 0; t < n_cols; ++t) {
          const uint64_t col = boot::drawn_column(base, t, n_cols);
          if (row[col] >= limit) { over[r] = col; break; }
          ++row[col];
        }
      }
    });
    for (uint64_t r = 0; r < count; ++r)
      if (over[r] != kNone) {
        pa_set_error("pa_msa_boot_weights: replicate %llu draws column %llu more than %u times: a weight is a uint8", (unsigned long long)(first + r),
                     (unsigned long long)over[r], limit);
        return PA_E_INVALID;
      }
    return PA_OK;
  });
}

int pa_msa_boot_counts(pa_ctx *c, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, uint32_t bits, const uint8_t *h_weights,
                       uint32_t n_reps, uint32_t *d_match, uint32_t *d_both) {
  PA_REQUIRE(c != nullptr, "pa_msa_boot_counts: null context");
  PA_REQUIRE(n_rows == 0 || n_reps == 0 || (d_planes && d_match && d_both && (h_weights || n_cols == 0)), "pa_msa_boot_counts: null argument");
  PA_REQUIRE(bits >= 1 && bits <= kMaxBits, "pa_msa_boot_counts: bits must be 1 to 8, not %u", bits);
  PA_REQUIRE(n_cols < (1ull << 32), "pa_msa_boot_counts: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols);
  PA_REQUIRE(n_rows <= 65535, "pa_msa_boot_counts: %u rows; at most 65535", n_rows);
  if (n_rows == 0 || n_reps == 0) return PA_OK;
  uint32_t max_weight = 0;
  PA_TRY(boot::check_weights("pa_msa_boot_counts", h_weights, n_cols, n_reps, &max_weight));
  PA_HIP(hipSetDevice(c->device));
  const int status = boot_counts_device(c, d_planes, n_rows, n_cols, bits, h_weights, n_reps, boot::weight_planes(max_weight), d_match, d_both);
  const hipError_t waited = hipStreamSynchronize(c->stream);  // copies from h_weights may still be queued
  if (status != PA_OK) return status;
  PA_HIP(waited);
  return PA_OK;
}

int pa_msa_boot_distances(pa_ctx *c, const uint32_t *d_match, const uint32_t *d_both, uint32_t n, uint32_t n_reps, double missing, double *d_D) {
  PA_REQUIRE(c != nullptr, "pa_msa_boot_distances: null context");
  PA_REQUIRE(n == 0 || n_reps == 0 || (d_match && d_both && d_D), "pa_msa_boot_distances: null argument");
  PA_REQUIRE(missing >= 0.0 && missing <= 1.79769313486231570815e308, "pa_msa_boot_distances: the distance of a pair without columns must be finite and not negative");
  const uint64_t cells = (uint64_t)n * n * n_reps;
  if (cells == 0) return PA_OK;
  PA_HIP(hipSetDevice(c->device));
  ProfScope prof(c, PA_PROF_MSA_BOOT_DIST);
  return PA_LAUNCH(c, msa_boot_distances_kernel, stride_blocks(cells), kThreads, 0, d_match, d_both, n, cells, missing, d_D);
}

}  // extern "C"
