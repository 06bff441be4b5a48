// murmur_words.h -- the table entries of a murmur word and what is computed from them, in plain C++ for device and host.
//
// One statement of the formulas for the kernels (murmur_dev.h fills the LDS tables from them and looks them up) and for
// the host-side check of the identity (tests/test_murmur_word_tables.py compiles them into a small program).
//
// MurmurHash3_x64_128 takes the K ASCII bytes of a k-mer as little-endian 64-bit words.  Word j (bases 8j .. 8j+7, the
// last one partial) is multiplied by cA, rotated left by r and multiplied by cB:
//   j even: (cA, cB) = (c1, c2), r = 31        j odd: (cA, cB) = (c2, c1), r = 33
// The word is two 4-base groups, lo and hi (8 bits each, base i at bits 2i).  With
//   A = ascii(lo)*cA (64 bit),  B = low32(ascii(hi)*cA),  S = A.hi + B (mod 2^32)
// the first product is P = (S << 32) + A.lo, and k_j = rotl(P, r)*cB splits into a part that is linear in A.lo alone --
// a function of the lo group, tabled as T -- and a 32 x 64 bit product of S:
//   j odd:   rotl(P, 33) = (A.lo << 33) + 2*S + (A.lo >> 31)
//            k_j = S*(2*cB) + T,                       T = ((A.lo << 33) + (A.lo >> 31))*cB
//   j even:  rotl(P, 31) = (A.lo << 31) + (S << 63) + (S >> 1),  and cB is odd, so
//            k_j = (S >> 1)*cB + ((S & 1) << 63) + T,  T = (A.lo << 31)*cB
// all modulo 2^64.  No rotate is left, and of the 64 x 64 multiply one v_mad_u64_u32 and one v_mul_lo_u32.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "pa_hd.h"

namespace pa_dev {

constexpr uint64_t kC1 = 0x87c37b91114253d5ULL, kC2 = 0x4cf5ad432745937fULL;

// 4 bases (8 bits, base j at bits 2j) -> 4 ASCII bytes (base j in byte j)
PA_HD uint32_t ascii4(uint32_t b8) {
#if defined(__HIP_DEVICE_COMPILE__)
  // spread the 2-bit codes to one per byte, then use v_perm_b32 as a 4-entry LUT.
  uint32_t u = (b8 | (b8 << 12)) & 0x000F000Fu;
  uint32_t v = (u | (u << 6)) & 0x03030303u;
  // selector byte value 0..3 picks that byte of the second source: "ACGT" little-endian
  return __builtin_amdgcn_perm(0u, 0x54474341u, v);
#else
  uint32_t a = 0;
  for (int i = 0; i < 4; ++i) a |= ((0x54474341u >> (8 * ((b8 >> (2 * i)) & 3u))) & 0xffu) << (8 * i);
  return a;
#endif
}

// the 4-base group `b8` (base j at bits 2j) as ASCII, keeping only its first `nv` bytes
PA_HD uint32_t ascii_group(uint32_t b8, int nv) {
  const uint32_t a = ascii4(b8);
  return nv >= 4 ? a : (nv <= 0 ? 0u : (a & ((1u << (8 * nv)) - 1u)));
}

PA_HD constexpr uint64_t word_c_first(int j) { return (j & 1) ? kC2 : kC1; }
PA_HD constexpr uint64_t word_c_second(int j) { return (j & 1) ? kC1 : kC2; }

// the entry of lo group `g` of word j of a k-mer of k bases: T and A.hi.  16 bytes, T first: one ds_read_b128 brings
// it, and T lands in an aligned register pair, the 64-bit addend of the v_mad_u64_u32.
struct WordLoEntry {
  uint32_t t_lo, t_hi, a_hi, pad;
};

PA_HD WordLoEntry word_lo_entry(int j, int k, uint32_t g) {
  const uint64_t a = (uint64_t)ascii_group(g, k - 8 * j) * word_c_first(j);
  const uint32_t a_lo = (uint32_t)a;
  const uint64_t cb = word_c_second(j);
  const uint64_t t = (j & 1) ? (((uint64_t)a_lo << 33) + (a_lo >> 31)) * cb : ((uint64_t)a_lo << 31) * cb;
  return WordLoEntry{(uint32_t)t, (uint32_t)(t >> 32), (uint32_t)(a >> 32), 0u};
}

// the entry of hi group `g`: B
PA_HD uint32_t word_hi_entry(int j, int k, uint32_t g) {
  return (uint32_t)((uint64_t)ascii_group(g, k - 8 * j - 4) * word_c_first(j));
}

// k_j from the two entries of word j.  The 32 x 64 bit product is one 32 x 32 -> 64 bit multiply-add onto T and one
// 32 x 32 -> 32 bit multiply into the high word; the halves are kept apart so that what goes into the high word is
// added as 32-bit values.
PA_HD uint64_t second_product_of(int j, uint32_t t_lo, uint32_t t_hi, uint32_t a_hi, uint32_t b) {
  const uint32_t s = a_hi + b;
  const uint64_t t = ((uint64_t)t_hi << 32) | t_lo;
  if (j & 1) {
    const uint64_t c = word_c_second(j) << 1;  // 2*cB mod 2^64
    const uint64_t m = (uint64_t)s * (uint32_t)c + t;
    return ((uint64_t)((uint32_t)(m >> 32) + s * (uint32_t)(c >> 32)) << 32) | (uint32_t)m;
  }
  const uint64_t c = word_c_second(j);
  const uint32_t x = s >> 1;
  const uint64_t m = (uint64_t)x * (uint32_t)c + t;
  return ((uint64_t)((uint32_t)(m >> 32) + (x * (uint32_t)(c >> 32) + (s << 31))) << 32) | (uint32_t)m;
}

}  // namespace pa_dev
