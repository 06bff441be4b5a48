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
// Plane layout (word-major, so that the 64 rows of a tile are one 256-byte load per plane and word):
//   planes[(w * P + p) * n_pad + row],  P = b + 1 (plane b = non-gap),  n_pad = n_rows rounded up to 64.
#include <algorithm>

#include "pa_internal.h"

namespace {
constexpr int kTile = 64;     // rows of a pair tile, queries and subjects alike
constexpr int kThreads = 256; // 16 x 16 lanes of 4 x 4 pairs each
constexpr int kChunk = 8;     // words of a stage through LDS
constexpr uint32_t kMaxBits = 8;

// v_bitop3_b32 (gfx950): bit i of the result is bit (a_i << 2 | b_i << 1 | c_i) of the table; the table of f(a, b, c) is
// f(0xf0, 0xcc, 0xaa).  The compiler does not always fuse these itself (it kept v_xor + v_or + v_not + v_and here).
constexpr uint32_t kXorOr = (0xf0u ^ 0xccu) | 0xaau;  // (a ^ b) | c
constexpr uint32_t kAndNot = ~0xf0u & 0xccu & 0xffu;   // ~a & b
template <uint32_t T>
__device__ inline uint32_t bitop3_t(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, T); }

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

// Upper-triangle tile t (row-major over the pairs ti <= tj of nt x nt tiles) -> (ti, tj)
__device__ inline void tri_tile(uint32_t t, uint32_t nt, uint32_t &ti, uint32_t &tj) {
  // tiles before row i: i * nt - i * (i - 1) / 2
  const double b = 2.0 * nt + 1.0;
  uint32_t i = (uint32_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (i >= nt) i = nt - 1;
  auto start = [nt](uint32_t r) { return (uint64_t)r * nt - (uint64_t)r * (r - 1u) / 2u; };
  while (i > 0 && start(i) > t) --i;
  while (i + 1 < nt && start(i + 1) <= t) ++i;
  ti = i;
  tj = i + (uint32_t)(t - start(i));
}

// One block: a 64 x 64 tile of pairs over the words [blockIdx.y * words_per_split, ...) -- the whole row when
// words_per_split covers it, a slice of it otherwise (split-K: the partial counts are added with atomics).
// Thread (tx, ty) owns queries ty*4 .. ty*4+3 and subjects tx*4 .. tx*4+3 of the tile.  Rows outside [q0, q1) or
// [s0, s1), and words past the last, are staged as zero: no gap bit, so they count nothing.
template <int P>
__global__ __launch_bounds__(kThreads) void msa_pairs_kernel(const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t n_words,
                                                             uint32_t words_per_split, uint32_t q0, uint32_t nq, uint32_t s0, uint32_t ns,
                                                             uint32_t n_tiles_s, int symmetric, int accumulate,
                                                             uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
  __shared__ uint32_t stage[2][kChunk][P][kTile];  // [0] queries, [1] subjects
  uint32_t ti, tj;
  if (symmetric) tri_tile(blockIdx.x, n_tiles_s, ti, tj);
  else { ti = blockIdx.x / n_tiles_s; tj = blockIdx.x % n_tiles_s; }
  const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
  const uint32_t w_lo = blockIdx.y * words_per_split;
  const uint32_t w_hi = min(n_words, w_lo + words_per_split);
  const uint32_t q_tile = ti * kTile, s_tile = tj * kTile;
  uint32_t m[4][4] = {{0}}, bo[4][4] = {{0}};
  constexpr uint32_t kHalf = kChunk * P * kTile;
  for (uint32_t wc = w_lo; wc < w_hi; wc += kChunk) {
    __syncthreads();
    for (uint32_t i = tid; i < 2u * kHalf; i += kThreads) {
      const uint32_t half = i / kHalf, rem = i % kHalf, r = rem % kTile, wp = rem / kTile;
      const uint32_t w = wc + wp / P, p = wp % P;
      const uint32_t local = (half ? s_tile : q_tile) + r;
      const bool ok = w < w_hi && local < (half ? ns : nq);
      const uint32_t row = (half ? s0 : q0) + local;
      (&stage[0][0][0][0])[i] = ok ? planes[((uint64_t)w * P + p) * n_pad + row] : 0u;
    }
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kChunk; ++k) {
      uint32_t qv[P][4], sv[P][4];
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const uint4 x = *reinterpret_cast<const uint4 *>(&stage[0][k][p][ty * 4u]);
        const uint4 y = *reinterpret_cast<const uint4 *>(&stage[1][k][p][tx * 4u]);
        qv[p][0] = x.x; qv[p][1] = x.y; qv[p][2] = x.z; qv[p][3] = x.w;
        sv[p][0] = y.x; sv[p][1] = y.y; sv[p][2] = y.z; sv[p][3] = y.w;
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          uint32_t d = qv[0][a] ^ sv[0][b];
#pragma unroll
          for (int p = 1; p < P - 1; ++p) d = bitop3_t<kXorOr>(qv[p][a], sv[p][b], d);
          m[a][b] += __builtin_popcount(bitop3_t<kAndNot>(d, qv[P - 1][a], 0u));
          bo[a][b] += __builtin_popcount(qv[P - 1][a] & sv[P - 1][b]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t qi = q_tile + ty * 4u + a;
    if (qi >= nq) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t sj = s_tile + tx * 4u + b;
      if (sj >= ns) continue;
      const uint64_t idx = (uint64_t)qi * ns + sj;
      if (accumulate) {
        atomicAdd(match + idx, m[a][b]);
        atomicAdd(both + idx, bo[a][b]);
      } else {
        match[idx] = m[a][b];
        both[idx] = bo[a][b];
      }
    }
  }
}

// Symmetric form: the tiles below the diagonal were not evaluated; (r, c) with tile(c) < tile(r) takes (c, r).
__global__ __launch_bounds__(kThreads) void msa_mirror_kernel(uint32_t n, uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
  for (uint32_t r = blockIdx.y; r < n; r += gridDim.y) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= (r / kTile) * kTile) continue;
    match[(uint64_t)r * n + c] = match[(uint64_t)c * n + r];
    both[(uint64_t)r * n + c] = both[(uint64_t)c * n + r];
  }
}

inline uint32_t n_pad_of(uint32_t n_rows) { return (n_rows + kTile - 1u) / kTile * kTile; }
inline uint64_t n_words_of(uint64_t n_cols) { return (n_cols + 31u) / 32u; }

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
  // split the columns when the tiles alone leave CUs idle: about 8 blocks per CU, each slice at least 64 words
  const uint64_t want = 8ull * (uint64_t)c->prop.multiProcessorCount;
  uint64_t splits = tiles >= want ? 1 : (want + tiles - 1) / tiles;
  splits = std::max<uint64_t>(1, std::min<uint64_t>({splits, (n_words + 63) / 64, 65535}));
  uint32_t wps = (uint32_t)((n_words + splits - 1) / splits);
  wps = (wps + kChunk - 1) / kChunk * kChunk;
  if (wps == 0) wps = kChunk;
  splits = (n_words + wps - 1) / wps;
  if (splits == 0) splits = 1;
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
  if (symmetric && tq > 1)
    PA_TRY(PA_LAUNCH(c, msa_mirror_kernel, LaunchDim((nq + kThreads - 1) / kThreads, nq < 65535u ? nq : 65535u), kThreads, 0, nq, d_match, d_both));
  return PA_OK;
}

}  // extern "C"
