// msa.hip -- external-alignment-hip on the device (gfx950, wave64): the pair counts of an MSA.
//
// The reference compares every query row with the subject row byte by byte, ten numpy passes per pair
// (pyani_plus/methods/external_alignment.py:118-156).  Everything it reports follows from two counts per pair
// (DESIGN.md section 8):
//   M = columns where q == s and q != '-',   B = columns where neither is '-'.
// Each row is first bit-sliced (msa_pack_kernel): a residue byte gets a code (gap 0, the A residues of the alphabet
// 1..A), the b = ceil(log2(A + 1)) bits of the codes of 32 columns make b words, and a last word holds the non-gap
// bits.  Then per pair and 32 columns (msa_pairs_kernel):
//   d = OR_p (q_p ^ s_p)          b instructions (one v_xor, then v_bitop3 (x ^ y) | z)
//   M += popcount(~d & ng_q)      v_bitop3 + v_bcnt_u32_b32 (which accumulates)
//   B += popcount(ng_q & ng_s)    v_and + v_bcnt
// b + 4 VALU instructions for 32 columns of one pair.
//
// msa_tile_dev.h has the plane layout and the tile that this kernel shares with the weighted counts of msa_boot.hip.
#include <algorithm>

#include "msa_tile_dev.h"

namespace {
using namespace msa_tile;

struct CodeTable {
  uint32_t w[64];  // byte c -> code (w[c / 4] >> (8 * (c % 4))) & 0xff
};

// Block: 64 rows (one per lane) x the words of blockIdx.y's range, the four waves taking every fourth word.  d_rows is
// 16-byte aligned and row_stride a multiple of 32 that covers every word, so the 32 bytes of a word are two aligned
// 16-byte loads; columns at or past n_cols are gap whatever the bytes say.
__global__ __launch_bounds__(kThreads) void msa_pack_kernel(const uint8_t *__restrict__ rows, uint64_t row_stride, uint32_t row0,
                                                            uint32_t n_chunk_rows, uint32_t n_pad, uint64_t n_cols, uint32_t n_words,
                                                            uint32_t words_per_block, CodeTable table, uint32_t bits,
                                                            uint32_t *__restrict__ planes, uint32_t *__restrict__ nongap) {
  __shared__ uint8_t code[256];
  code[threadIdx.x] = (uint8_t)(table.w[threadIdx.x >> 2] >> (8u * (threadIdx.x & 3u)));
  __syncthreads();
  const uint32_t local = blockIdx.x * 64u + (threadIdx.x & 63u);
  if (local >= n_chunk_rows) return;
  const uint32_t row = row0 + local;
  const uint32_t P = bits + 1u;
  const uint32_t w_lo = blockIdx.y * words_per_block;
  const uint32_t w_hi = min(n_words, w_lo + words_per_block);
  const uint8_t *src = rows + (uint64_t)local * row_stride;
  uint32_t count = 0;
  for (uint32_t w = w_lo + (threadIdx.x >> 6); w < w_hi; w += kThreads / 64) {
    const uint4 *p16 = reinterpret_cast<const uint4 *>(src + (uint64_t)w * 32u);
    const uint4 v0 = p16[0], v1 = p16[1];
    const uint32_t words[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t out[kMaxBits + 1] = {0};
    const uint64_t col0 = (uint64_t)w * 32u;
    const uint32_t valid = n_cols - col0 >= 32u ? 0xffffffffu : ((1u << (uint32_t)(n_cols - col0)) - 1u);
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t c = (valid >> j) & 1u ? (uint32_t)code[(words[j >> 2] >> (8 * (j & 3))) & 0xffu] : 0u;
#pragma unroll
      for (uint32_t p = 0; p < kMaxBits; ++p) out[p] |= ((c >> p) & 1u) << j;
      out[kMaxBits] |= (c != 0u ? 1u : 0u) << j;
    }
    uint32_t *dst = planes + (uint64_t)w * P * n_pad + row;
    for (uint32_t p = 0; p < bits; ++p) dst[(uint64_t)p * n_pad] = out[p];
    dst[(uint64_t)bits * n_pad] = out[kMaxBits];
    count += __builtin_popcount(out[kMaxBits]);
  }
  if (count) atomicAdd(nongap + row, count);
}

// One block: a 64 x 64 tile of pairs over the words of blockIdx.y's slice (msa_tile::tile_geom; split-K: the partial
// counts are added with atomics).  b + 4 VALU instructions for 32 columns of one pair.
template <int P>
__global__ __launch_bounds__(kThreads) void msa_pairs_kernel(const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t n_words,
                                                             uint32_t words_per_split, uint32_t q0, uint32_t nq, uint32_t s0, uint32_t ns,
                                                             uint32_t n_tiles_s, int symmetric, int accumulate,
                                                             uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
  __shared__ Stage<P> stage;
  const TileGeom g = tile_geom(n_tiles_s, symmetric, n_words, words_per_split);
  const Ranges r{q0, nq, s0, ns};
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  uint32_t m[4][4] = {{0}}, bo[4][4] = {{0}};
  for (uint32_t wc = g.w_lo; wc < g.w_hi; wc += kChunk) {
    __syncthreads();
    stage_words<P>(stage, planes, n_pad, wc, g, r, tid);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      uint32_t qv[P][4], sv[P][4];
      load_rows<P>(stage, k, tx, ty, qv, sv);
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          m[a][b] += __builtin_popcount(eq_word<P>(qv, sv, a, b));
          bo[a][b] += __builtin_popcount(both_word<P>(qv, sv, a, b));
        }
      }
    }
  }
  write_counts(m, bo, g, r, tx, ty, accumulate, match, both);
}

}  // namespace

extern "C" {

uint64_t pa_msa_plane_words(uint32_t n_rows, uint64_t n_cols, uint32_t bits) {
  return (uint64_t)n_pad_of(n_rows) * n_words_of(n_cols) * (bits + 1u);
}

int pa_msa_pack(pa_ctx *c, const uint8_t *d_rows, uint64_t row_stride, uint32_t row0, uint32_t n_chunk_rows, uint32_t n_rows,
                uint64_t n_cols, const uint8_t *h_code256, uint32_t bits, uint32_t *d_planes, uint32_t *d_nongap) {
  PA_REQUIRE(c && h_code256 && d_planes && d_nongap && (d_rows || n_chunk_rows == 0), "pa_msa_pack: null argument");
  PA_REQUIRE(bits >= 1 && bits <= kMaxBits, "pa_msa_pack: bits must be 1 to 8, not %u", bits);
  PA_REQUIRE(n_cols < (1ull << 32), "pa_msa_pack: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols);
  PA_REQUIRE((uint64_t)row0 + n_chunk_rows <= n_rows, "pa_msa_pack: rows [%u, %llu) past %u rows", row0,
             (unsigned long long)row0 + n_chunk_rows, n_rows);
  const uint64_t n_words = n_words_of(n_cols);
  PA_REQUIRE(row_stride % 32u == 0 && row_stride >= n_words * 32u, "pa_msa_pack: row stride %llu must be a multiple of 32 and at least %llu",
             (unsigned long long)row_stride, (unsigned long long)(n_words * 32u));
  PA_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 15u) == 0, "pa_msa_pack: rows must be 16-byte aligned");
  PA_REQUIRE(h_code256['-'] == 0, "pa_msa_pack: the gap '-' must have code 0");
  CodeTable table{};
  for (int b = 0; b < 256; ++b) {
    PA_REQUIRE(h_code256[b] < (1u << bits), "pa_msa_pack: byte %d has code %u, not below 2^%u", b, h_code256[b], bits);
    table.w[b >> 2] |= (uint32_t)h_code256[b] << (8 * (b & 3));
  }
  if (n_chunk_rows == 0 || n_words == 0) return PA_OK;
  PA_HIP(hipSetDevice(c->device));
  ProfScope prof(c, PA_PROF_MSA_PACK);
  // about 4 blocks per CU, each with a run of words of its rows
  const uint32_t row_blocks = (n_chunk_rows + 63u) / 64u;
  const uint64_t want = 4ull * (uint64_t)c->prop.multiProcessorCount;
  uint64_t splits = (want + row_blocks - 1) / row_blocks;
  splits = std::max<uint64_t>(1, std::min<uint64_t>({splits, (n_words + 15) / 16, 65535}));
  const uint32_t wpb = (uint32_t)((n_words + splits - 1) / splits);
  splits = (n_words + wpb - 1) / wpb;
  return PA_LAUNCH(c, msa_pack_kernel, LaunchDim(row_blocks, splits), kThreads, 0, d_rows, row_stride, row0, n_chunk_rows, n_pad_of(n_rows), n_cols,
                   (uint32_t)n_words, wpb, table, bits, d_planes, d_nongap);
}

int pa_msa_pair_counts(pa_ctx *c, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, uint32_t bits, uint32_t q0, uint32_t q1,
                       uint32_t s0, uint32_t s1, int symmetric, uint32_t *d_match, uint32_t *d_both) {
  PA_REQUIRE(c != nullptr, "pa_msa_pair_counts: null context");
  PA_REQUIRE((q0 == q1 || s0 == s1) || (d_planes && d_match && d_both), "pa_msa_pair_counts: null argument");
  PA_REQUIRE(bits >= 1 && bits <= kMaxBits, "pa_msa_pair_counts: bits must be 1 to 8, not %u", bits);
  PA_REQUIRE(n_cols < (1ull << 32), "pa_msa_pair_counts: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols);
  PA_REQUIRE(q0 <= q1 && q1 <= n_rows && s0 <= s1 && s1 <= n_rows, "pa_msa_pair_counts: ranges [%u, %u) x [%u, %u) outside %u rows", q0, q1,
             s0, s1, n_rows);
  PA_REQUIRE(!symmetric || (q0 == s0 && q1 == s1), "pa_msa_pair_counts: the symmetric form needs equal query and subject ranges");
  const uint32_t nq = q1 - q0, ns = s1 - s0;
  if (nq == 0 || ns == 0) return PA_OK;
  PA_HIP(hipSetDevice(c->device));
  ProfScope prof(c, PA_PROF_MSA_PAIRS);
  const uint32_t n_words = (uint32_t)n_words_of(n_cols);
  const uint32_t tq = (nq + kTile - 1) / kTile, ts = (ns + kTile - 1) / kTile;
  const uint64_t tiles = symmetric ? (uint64_t)tq * (tq + 1) / 2 : (uint64_t)tq * ts;
  PA_REQUIRE(tiles < (1ull << 31), "pa_msa_pair_counts: %llu tiles", (unsigned long long)tiles);
  const ColumnSplit split = split_columns(c, tiles, n_words);
  const uint32_t splits = split.splits, wps = split.words_per_split;
  const int accumulate = splits > 1;
  if (accumulate || n_words == 0) {
    PA_HIP(hipMemsetAsync(d_match, 0, (uint64_t)nq * ns * 4u, c->stream));
    PA_HIP(hipMemsetAsync(d_both, 0, (uint64_t)nq * ns * 4u, c->stream));
  }
  if (n_words) {
    const LaunchDim grid(tiles, splits);
    const uint32_t np = n_pad_of(n_rows);
    int status = PA_OK;
    auto launch_pairs = [&](auto planes) {
      status = PA_LAUNCH(c, msa_pairs_kernel<planes()>, grid, kThreads, 0, d_planes, np, n_words, wps, q0, nq, s0, ns, symmetric ? tq : ts, symmetric,
                         accumulate, d_match, d_both);
    };
    if (!dispatch_value(bits + 1, value_list<2, 7>{}, launch_pairs)) launch_pairs(std::integral_constant<int, 9>{});
    PA_TRY(status);
  }
  if (symmetric && tq > 1) PA_TRY(launch_mirror(c, nq, 1, d_match, d_both));
  return PA_OK;
}

}  // extern "C"
