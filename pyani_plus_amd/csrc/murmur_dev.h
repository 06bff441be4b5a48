// murmur_dev.h -- device helpers shared by the k-mer hashing kernels (gfx950).
//
// MurmurHash3_x64_128 (Appleby, public-domain algorithm), seed 42, first 64-bit word: the hash
// sourmash applies to canonical k-mers (call site pyani_plus/methods/sourmash.py:67-83) and, in its
// low 32 bits, the one fastANI/Mashmap applies to both strands of every k-mer
// (call site pyani_plus/private_cli.py:1044-1063).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "murmur_words.h"  // kC1, kC2, ascii4, ascii_group and the entries of the second-product tables: device and host

namespace pa_dev {

__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
  return __builtin_amdgcn_alignbit(hi, lo, sh);
}

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// 64-bit rotate as two funnel shifts (v_alignbit_b32); r is a compile-time constant in 1..63
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) {
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  if (r == 32) return u64_of(hi, lo);
  if (r < 32) return u64_of(alignbit(lo, hi, 32 - r), alignbit(hi, lo, 32 - r));
  return u64_of(alignbit(hi, lo, 64 - r), alignbit(lo, hi, 64 - r));
}

__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

// ---- MurmurHash3_x64_128(seed 42).h1, split at the first multiply -----------------
// The K ASCII bytes form up to four little-endian 64-bit words; word j is a "k1" word
// (j even: k*c1, rotl 31, *c2, xor into h1) or a "k2" word (j odd: k*c2, rotl 33, *c1,
// xor into h2), in the 16-byte blocks and in the tail alike.  P[j] is the FIRST product
// (word * c1 or c2), Kw[j] the second one (rotated first product * c2 or c1); everything after it is computed here.

// h*5 + c.  Left to itself hipcc turns this into two v_mad_u64_u32 plus fix-ups; gfx950 has a 64-bit
// shift-and-add (v_lshl_add_u64, shift 0..4), so (h << 2) + h is one instruction and + c a second.
__device__ __forceinline__ uint64_t times5_plus(uint64_t h, uint64_t c) {
  uint64_t t;
  asm("v_lshl_add_u64 %0, %1, 2, %1" : "=v"(t) : "v"(h));
  return t + c;
}

constexpr uint64_t kF1 = 0xff51afd7ed558ccdULL, kF2 = 0xc4ceb9fe1a85ec53ULL;  // fmix64 multipliers

// Everything up to, but not including, the LAST multiply of the two fmix64 calls: with U and V the values this
// returns, the hash is h = fin(U*kF2) + fin(V*kF2), fin(x) = x ^ (x >> 33).  fin only touches the low 31 bits, so
// the high word of h is hi32(U*kF2) + hi32(V*kF2) + at most one carry -- and that sum of two high words is linear:
//   hi32(U*c) + hi32(V*c) = mulhi(U.lo, c.lo) + mulhi(V.lo, c.lo) + (U.lo + V.lo)*c.hi + (U.hi + V.hi)*c.lo  (mod 2^32)
// which is what the FracMinHash screen of kmer_hash.hip tests before anything else of the last step is computed.
// (The 64-bit multiplies are left to hipcc: v_mad_u64_u32 + 2 v_mul_lo_u32 + v_add3_u32.  A hand-written
// chain of three v_mad_u64_u32 + one add was measured at the same speed.)
template <int K, int N>
__device__ __forceinline__ void murmur3_pre_last_mul(const uint64_t (&P)[N], uint64_t &U, uint64_t &V) {
  static_assert(N >= (K + 7) / 8, "one first product per 8-byte word of the k-mer");
  uint64_t h1 = 42, h2 = 42;
  constexpr int nblocks = K / 16;
  constexpr int tail = K % 16;
#pragma unroll
  for (int i = 0; i < nblocks; ++i) {
    const uint64_t k1 = rotl64(P[2 * i], 31) * kC2;
    h1 ^= k1;
    if (i == 0) {  // h2 is still the seed: (rotl(h1) + 42) * 5 + c = rotl(h1) * 5 + (5 * 42 + c), one 64-bit add less
      h1 = times5_plus(rotl64(h1, 27), 5ULL * 42ULL + 0x52dce729ULL);
    } else {
      h1 = rotl64(h1, 27) + h2;
      h1 = times5_plus(h1, 0x52dce729ULL);
    }
    const uint64_t k2 = rotl64(P[2 * i + 1], 33) * kC1;
    h2 ^= k2;
    h2 = rotl64(h2, 31) + h1;
    h2 = times5_plus(h2, 0x38495ab5ULL);
  }
  if constexpr (tail > 8) h2 ^= rotl64(P[2 * nblocks + 1], 33) * kC1;
  if constexpr (tail > 0) h1 ^= rotl64(P[2 * nblocks], 31) * kC2;
  h1 ^= (uint64_t)K; h2 ^= (uint64_t)K;
  h1 += h2; h2 += h1;
  h1 ^= h1 >> 33; h1 *= kF1; h1 ^= h1 >> 33;
  h2 ^= h2 >> 33; h2 *= kF1; h2 ^= h2 >> 33;
  U = h1;
  V = h2;
}

// the same from the second products Kw[j] (second_product below): the four rotates and 64 x 64 multiplies are gone
template <int K, int N>
__device__ __forceinline__ void murmur3_pre_last_mul_of_seconds(const uint64_t (&Kw)[N], uint64_t &U, uint64_t &V) {
  static_assert(N >= (K + 7) / 8, "one second product per 8-byte word of the k-mer");
  uint64_t h1 = 42, h2 = 42;
  constexpr int nblocks = K / 16;
  constexpr int tail = K % 16;
#pragma unroll
  for (int i = 0; i < nblocks; ++i) {
    h1 ^= Kw[2 * i];
    if (i == 0) {
      h1 = times5_plus(rotl64(h1, 27), 5ULL * 42ULL + 0x52dce729ULL);
    } else {
      h1 = rotl64(h1, 27) + h2;
      h1 = times5_plus(h1, 0x52dce729ULL);
    }
    h2 ^= Kw[2 * i + 1];
    // the rotated value as one register pair: left to itself hipcc adds its two halves to h1 one by one, each paired
    // with a zero (a v_mov and two v_lshl_add_u64 where one 64-bit add does)
    uint64_t r2 = rotl64(h2, 31);
    asm("" : "+v"(r2));
    h2 = times5_plus(r2 + h1, 0x38495ab5ULL);
  }
  if constexpr (tail > 8) h2 ^= Kw[2 * nblocks + 1];
  if constexpr (tail > 0) h1 ^= Kw[2 * nblocks];
  h1 ^= (uint64_t)K; h2 ^= (uint64_t)K;
  h1 += h2; h2 += h1;
  h1 ^= h1 >> 33; h1 *= kF1; h1 ^= h1 >> 33;
  h2 ^= h2 >> 33; h2 *= kF1; h2 ^= h2 >> 33;
  U = h1;
  V = h2;
}

// the same for a run-time k (uniform over the launch, at most 64); P holds eight first products, the unused ones 0
__device__ __forceinline__ void murmur3_pre_last_mul_rt(const uint64_t (&P)[8], uint32_t k, uint64_t &U, uint64_t &V) {
  uint64_t h1 = 42, h2 = 42;
  const uint32_t nblocks = k >> 4, tail = k & 15u;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    if (i >= nblocks) break;
    h1 ^= rotl64(P[2 * i], 31) * kC2;
    h1 = rotl64(h1, 27) + h2;
    h1 = times5_plus(h1, 0x52dce729ULL);
    h2 ^= rotl64(P[2 * i + 1], 33) * kC1;
    h2 = rotl64(h2, 31) + h1;
    h2 = times5_plus(h2, 0x38495ab5ULL);
  }
  uint64_t t1 = 0, t2 = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i)
    if (i == nblocks) { t1 = P[2 * i]; t2 = P[2 * i + 1]; }
  if (tail > 8) h2 ^= rotl64(t2, 33) * kC1;
  if (tail > 0) h1 ^= rotl64(t1, 31) * kC2;
  h1 ^= (uint64_t)k;
  h2 ^= (uint64_t)k;
  h1 += h2;
  h2 += h1;
  h1 ^= h1 >> 33; h1 *= kF1; h1 ^= h1 >> 33;
  h2 ^= h2 >> 33; h2 *= kF1; h2 ^= h2 >> 33;
  U = h1;
  V = h2;
}

// X.hi + Y.hi + 1 (mod 2^32) for X = U*kF2, Y = V*kF2, without forming X and Y (see above)
__device__ __forceinline__ uint32_t last_mul_high_sum_plus1(uint64_t U, uint64_t V) {
  constexpr uint32_t c0 = (uint32_t)kF2, c1 = (uint32_t)(kF2 >> 32);
  const uint32_t u0 = (uint32_t)U, u1 = (uint32_t)(U >> 32), v0 = (uint32_t)V, v1 = (uint32_t)(V >> 32);
  return (__umulhi(u0, c0) + __umulhi(v0, c0) + 1u) + ((u0 + v0) * c1 + (u1 + v1) * c0);
}

// The last step for a FracMinHash with threshold max_hash, in two parts: the screen, then -- for the windows it lets
// through -- the last multiply and the fold.
// Screen on the high words: hash = (X ^ X>>33) + (Y ^ Y>>33) has high word X.hi + Y.hi + carry, so it can be
// <= max_hash only if X.hi + Y.hi is <= max_hash.hi or is 0xffffffff (the carry wraps it to 0) -- one unsigned compare
// of X.hi + Y.hi + 1 against screen_hi = max_hash.hi + 1.  The 999 in 1000 windows that are dropped never form X and
// Y: 2 mul_hi + 2 mul_lo + 4 adds + 1 compare instead of two 64-bit multiplies, an add and 2 compares.
// take_all = (max_hash.hi == 0xffffffff), scaled = 1: no screen.  Both are per-thread constants of the caller.
__device__ __forceinline__ bool passes_screen(uint64_t U, uint64_t V, bool take_all, uint32_t screen_hi) {
  return take_all || last_mul_high_sum_plus1(U, V) <= screen_hi;
}
__device__ __forceinline__ uint64_t last_mul_and_fold(uint64_t U, uint64_t V) {
  const uint64_t X = U * kF2, Y = V * kF2;
  return (X ^ (X >> 33)) + (Y ^ (Y >> 33));
}

template <int K, int N>
__device__ __forceinline__ uint64_t murmur3_from_products(const uint64_t (&P)[N]) {
  uint64_t U, V;
  murmur3_pre_last_mul<K, N>(P, U, V);
  return last_mul_and_fold(U, V);
}

// ---- the first multiply of every murmur word, looked up -----------------------------
// Word j of the k-mer (bases 8j .. 8j+7, the last one partial) is two 4-base groups (lo, hi), and
//   word*c_j = (ascii(lo) + ascii(hi)*2^32)*c_j = s_lo[j][lo] + (s_hi[j][hi] << 32)   (mod 2^64)
// with s_lo[j][b] = ascii(b)*c_j (64 bit) and s_hi[j][b] = low32(ascii(b)*c_j): two LDS reads and one add replace the
// ASCII expansion (8 VALU) and a 64-bit multiply (3 quarter-rate VALU).
// Fills the tables of a k-mer of k bases, thread `tid` of 256 one entry of each; k may be a compile-time or a
// run-time value.  The caller puts a barrier between this and the first look-up.
template <int W, class KInt>
__device__ __forceinline__ void fill_first_products(uint64_t (&s_lo)[W][256], uint32_t (&s_hi)[W][256], uint32_t tid, KInt k_) {
  const int k = (int)k_;
  const int n_words = (int)(((uint32_t)k + 7u) >> 3);
#pragma unroll
  for (int j = 0; j < n_words; ++j) {
    const uint64_t cj = (j & 1) ? kC2 : kC1;
    s_lo[j][tid] = (uint64_t)ascii_group(tid, k - 8 * j) * cj;
    s_hi[j][tid] = (uint32_t)((uint64_t)ascii_group(tid, k - 8 * j - 4) * cj);
  }
}

// P[j] from the tables; src is the 32-bit word j/2 of the k-mer (base i at bits 2i), which holds word j's two groups
template <int W>
__device__ __forceinline__ uint64_t first_product(const uint64_t (&s_lo)[W][256], const uint32_t (&s_hi)[W][256], uint32_t j, uint32_t src) {
  const uint32_t glo = (src >> (16u * (j & 1u))) & 0xffu, ghi = (src >> (16u * (j & 1u) + 8u)) & 0xffu;
  const uint64_t lo = s_lo[j][glo];
  return u64_of((uint32_t)lo, (uint32_t)(lo >> 32) + s_hi[j][ghi]);
}

// ---- the second multiply of every murmur word, from tables and one 32 x 64 bit product ------------------------------
// murmur_words.h has the identity and the entries.  s_w[j][lo group] = {T, A.hi} (16 bytes, one ds_read_b128),
// s_b[j][hi group] = B; thread `tid` of 256 fills one entry of each.  The caller puts a barrier between this and the
// first look-up.
template <int W>
__device__ __forceinline__ void fill_second_products(uint4 (&s_w)[W][256], uint32_t (&s_b)[W][256], uint32_t tid, int k) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const WordLoEntry e = word_lo_entry(j, k, tid);
    s_w[j][tid] = make_uint4(e.t_lo, e.t_hi, e.a_hi, e.pad);
    s_b[j][tid] = word_hi_entry(j, k, tid);
  }
}

// byte `byte` of src, times 2^SH: the byte offset of a table entry, one SDWA shift whichever byte it is (left to
// itself hipcc spends a shift and an `and` on byte 0)
template <uint32_t SH>
__device__ __forceinline__ uint32_t byte_offset(uint32_t src, uint32_t byte) {
  uint32_t r;
  const uint32_t sh = SH;
  switch (byte) {
    case 0: asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(sh), "v"(src)); break;
    case 1: asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(sh), "v"(src)); break;
    case 2: asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(sh), "v"(src)); break;
    default: asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(sh), "v"(src)); break;
  }
  return r;
}

// k_j from the tables; src is the 32-bit word j/2 of the k-mer (base i at bits 2i), which holds word j's two groups
template <int W>
__device__ __forceinline__ uint64_t second_product(const uint4 (&s_w)[W][256], const uint32_t (&s_b)[W][256], int j, uint32_t src) {
  const uint32_t off_w = byte_offset<4>(src, 2u * (j & 1)), off_b = byte_offset<2>(src, 2u * (j & 1) + 1u);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4 e = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const char *>(&s_w[j][0]) + off_w);
  // the whole entry in one aligned register quad: without this hipcc drops the pad and reads the rest in two pieces
  asm("" : "+v"(e));
  const uint32_t b = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(&s_b[j][0]) + off_b);
  return second_product_of(j, e.x, e.y, e.z, b);
}

}  // namespace pa_dev
