// msa_tile_dev.h -- the 64 x 64 pair tile over an alignment's bit planes, stated once for msa.hip (the pair counts of
// external-alignment-hip), msa_boot.hip (the counts of bootstrap-run under column weights) and subst.hip (the three
// substitution counts of phylo-run, which stage three planes of four): the tile's geometry, its
// staging through LDS, the two words a pair and 32 columns come down to, the write of a tile's counts, the mirror of
// the symmetric form and the split of the columns over the grid.
//
// Plane layout (word-major, so that the 64 rows of a tile are one 256-byte load per plane and word):
//   planes[(w * P + p) * n_pad + row],  P = b + 1 (plane b = non-gap),  n_pad = n_rows rounded up to 64.
#pragma once

#include <algorithm>

#include "pa_internal.h"

namespace msa_tile {

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

// The rows a block compares: queries [q0, q0 + nq) against subjects [s0, s0 + ns) of the planes
struct Ranges {
  uint32_t q0, nq, s0, ns;
};

// What block (blockIdx.x, blockIdx.y) has: the first query and subject of its tile, relative to the ranges, and its
// words [w_lo, w_hi) -- the whole row when words_per_split covers it, a slice of it otherwise (split-K)
struct TileGeom {
  uint32_t q_tile, s_tile, w_lo, w_hi;
};
__device__ inline TileGeom tile_geom(uint32_t n_tiles_s, int symmetric, uint32_t n_words, uint32_t words_per_split) {
  uint32_t ti, tj;
  if (symmetric) tri_tile(blockIdx.x, n_tiles_s, ti, tj);
  else { ti = blockIdx.x / n_tiles_s; tj = blockIdx.x % n_tiles_s; }
  const uint32_t w_lo = blockIdx.y * words_per_split;
  return TileGeom{ti * kTile, tj * kTile, w_lo, min(n_words, w_lo + words_per_split)};
}

// The words [wc, wc + kChunk) of a tile's rows in LDS: [0] queries, [1] subjects.  Aligned for load_rows' 16-byte reads
// (ds_read_b128; with the alignment of a uint32_t the compiler splits each into two ds_read2_b32).
template <int P>
struct alignas(16) Stage {
  uint32_t w[2][kChunk][P][kTile];
};

// Rows outside the ranges, and words at or past w_hi, are staged as zero: no gap bit, so they count nothing.
template <int P>
__device__ inline void stage_words(Stage<P> &stage, const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t wc, const TileGeom &g,
                                   const Ranges &r, uint32_t tid) {
  constexpr uint32_t kHalf = kChunk * P * kTile;
  for (uint32_t i = tid; i < 2u * kHalf; i += kThreads) {
    const uint32_t half = i / kHalf, rem = i % kHalf, row_in_tile = rem % kTile, wp = rem / kTile;
    const uint32_t w = wc + wp / P, p = wp % P;
    const uint32_t local = (half ? g.s_tile : g.q_tile) + row_in_tile;
    const bool ok = w < g.w_hi && local < (half ? r.ns : r.nq);
    const uint32_t row = (half ? r.s0 : r.q0) + local;
    (&stage.w[0][0][0][0])[i] = ok ? planes[((uint64_t)w * P + p) * n_pad + row] : 0u;
  }
}

// Three of the P planes, A, B and C, as the planes 0, 1 and 2 of a three-plane stage (subst.hip reads the two code bits
// it compares and the non-gap plane of a four-plane layout): stage_words with a stride; load_rows<3> reads it back.
template <int P, int A, int B, int C>
__device__ inline void stage_three_planes(Stage<3> &stage, const uint32_t *__restrict__ planes, uint32_t n_pad, uint32_t wc, const TileGeom &g,
                                          const Ranges &r, uint32_t tid) {
  static_assert(A < P && B < P && C < P, "a plane of the layout");
  constexpr uint32_t kHalf = kChunk * 3 * kTile;
  for (uint32_t i = tid; i < 2u * kHalf; i += kThreads) {
    const uint32_t half = i / kHalf, rem = i % kHalf, row_in_tile = rem % kTile, wp = rem / kTile;
    const uint32_t w = wc + wp / 3u, slot = wp % 3u, p = slot == 0 ? A : slot == 1 ? B : C;
    const uint32_t local = (half ? g.s_tile : g.q_tile) + row_in_tile;
    const bool ok = w < g.w_hi && local < (half ? r.ns : r.nq);
    const uint32_t row = (half ? r.s0 : r.q0) + local;
    (&stage.w[0][0][0][0])[i] = ok ? planes[((uint64_t)w * P + p) * n_pad + row] : 0u;
  }
}

// Thread (tx, ty) owns queries ty*4 .. ty*4+3 and subjects tx*4 .. tx*4+3 of the tile: their planes of staged word k
template <int P>
__device__ inline void load_rows(const Stage<P> &stage, int k, uint32_t tx, uint32_t ty, uint32_t (&qv)[P][4], uint32_t (&sv)[P][4]) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const uint4 x = *reinterpret_cast<const uint4 *>(&stage.w[0][k][p][ty * 4u]);
    const uint4 y = *reinterpret_cast<const uint4 *>(&stage.w[1][k][p][tx * 4u]);
    qv[p][0] = x.x; qv[p][1] = x.y; qv[p][2] = x.z; qv[p][3] = x.w;
    sv[p][0] = y.x; sv[p][1] = y.y; sv[p][2] = y.z; sv[p][3] = y.w;
  }
}

// 32 columns of the pair (query a, subject b): the columns where q == s and q is no gap, and those where neither is
//   d = OR_p (q_p ^ s_p)     b instructions (one v_xor, then v_bitop3 (x ^ y) | z)
//   eq = ~d & ng_q           v_bitop3
//   both = ng_q & ng_s       v_and
template <int P>
__device__ inline uint32_t eq_word(const uint32_t (&qv)[P][4], const uint32_t (&sv)[P][4], int a, int b) {
  uint32_t d = qv[0][a] ^ sv[0][b];
#pragma unroll
  for (int p = 1; p < P - 1; ++p) d = bitop3_t<kXorOr>(qv[p][a], sv[p][b], d);
  return bitop3_t<kAndNot>(d, qv[P - 1][a], 0u);
}
template <int P>
__device__ inline uint32_t both_word(const uint32_t (&qv)[P][4], const uint32_t (&sv)[P][4], int a, int b) {
  return qv[P - 1][a] & sv[P - 1][b];
}

// A thread's 4 x 4 counts to match[qi * ns + sj] and both[...]: stored, or added with atomics when the columns are split
__device__ inline void write_counts(const uint32_t (&m)[4][4], const uint32_t (&bo)[4][4], const TileGeom &g, const Ranges &r, uint32_t tx,
                                    uint32_t ty, int accumulate, uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t qi = g.q_tile + ty * 4u + a;
    if (qi >= r.nq) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t sj = g.s_tile + tx * 4u + b;
      if (sj >= r.ns) continue;
      const uint64_t idx = (uint64_t)qi * r.ns + sj;
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

// The same for three counts a pair
__device__ inline void write_counts3(const uint32_t (&x)[4][4], const uint32_t (&y)[4][4], const uint32_t (&z)[4][4], const TileGeom &g,
                                     const Ranges &r, uint32_t tx, uint32_t ty, int accumulate, uint32_t *__restrict__ out_x,
                                     uint32_t *__restrict__ out_y, uint32_t *__restrict__ out_z) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t qi = g.q_tile + ty * 4u + a;
    if (qi >= r.nq) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t sj = g.s_tile + tx * 4u + b;
      if (sj >= r.ns) continue;
      const uint64_t idx = (uint64_t)qi * r.ns + sj;
      if (accumulate) {
        atomicAdd(out_x + idx, x[a][b]);
        atomicAdd(out_y + idx, y[a][b]);
        atomicAdd(out_z + idx, z[a][b]);
      } else {
        out_x[idx] = x[a][b];
        out_y[idx] = y[a][b];
        out_z[idx] = z[a][b];
      }
    }
  }
}

// Symmetric form: the tiles below the diagonal were not evaluated; (r, c) with tile(c) < tile(r) takes (c, r).
// blockIdx.z: which of the n x n matrices that follow one another in match and in both.
static __global__ __launch_bounds__(kThreads) void msa_mirror_kernel(uint32_t n, uint32_t *__restrict__ match, uint32_t *__restrict__ both) {
  const uint64_t at = (uint64_t)blockIdx.z * n * n;
  match += at;
  both += at;
  for (uint32_t r = blockIdx.y; r < n; r += gridDim.y) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= (r / kTile) * kTile) continue;
    match[(uint64_t)r * n + c] = match[(uint64_t)c * n + r];
    both[(uint64_t)r * n + c] = both[(uint64_t)c * n + r];
  }
}
inline int launch_mirror(pa_ctx *c, uint32_t n, uint32_t n_matrices, uint32_t *d_match, uint32_t *d_both) {
  return PA_LAUNCH(c, msa_mirror_kernel, LaunchDim((n + kThreads - 1) / kThreads, n < 65535u ? n : 65535u, n_matrices), kThreads, 0, n, d_match, d_both);
}

inline uint32_t n_pad_of(uint32_t n_rows) { return (n_rows + kTile - 1u) / kTile * kTile; }
inline uint64_t n_words_of(uint64_t n_cols) { return (n_cols + 31u) / 32u; }

// The split of the columns when `blocks` (the tiles, times whatever else the grid has) alone leave CUs idle: about 8
// blocks per CU, each slice at least 64 words and a whole number of stages
struct ColumnSplit {
  uint32_t splits, words_per_split;
};
inline ColumnSplit split_columns(const pa_ctx *c, uint64_t blocks, uint32_t n_words) {
  const uint64_t want = 8ull * (uint64_t)c->prop.multiProcessorCount;
  uint64_t splits = blocks >= want ? 1 : (want + blocks - 1) / blocks;
  splits = std::max<uint64_t>(1, std::min<uint64_t>({splits, ((uint64_t)n_words + 63) / 64, 65535}));
  uint32_t wps = (uint32_t)((n_words + splits - 1) / splits);
  wps = (wps + kChunk - 1) / kChunk * kChunk;
  if (wps == 0) wps = kChunk;
  splits = ((uint64_t)n_words + wps - 1) / wps;
  if (splits == 0) splits = 1;
  return ColumnSplit{(uint32_t)splits, wps};
}

}  // namespace msa_tile
