// subst_rule.h -- the arithmetic of phylo-run, stated once for subst.hip and subst_host.cpp (DESIGN.md section 7m has
// the contract): the nucleotide code of a byte, the natural logarithm L, and the distance of a pair's three counts
// under the models p, JC69 and K80.  Every operation is rounded on its own (strict_fp.h); L uses + - * / and integer
// operations on the exponent alone -- no libm, no device intrinsic -- so that host and device give the same bits.
#pragma once

#include <cstdint>

#include "../../include/pyani_hip.h"
#include "pa_hd.h"
#include "strict_fp.h"

namespace subst {

// A a -> 4, G g -> 5, C c -> 6, T t U u -> 7, every other byte 0: bit 2 "is a nucleotide", bit 1 the class (0 purine,
// 1 pyrimidine), bit 0 the base within the class
PA_HD uint8_t code_of(uint32_t byte) {
  switch (byte) {
    case 'A': case 'a': return 4;
    case 'G': case 'g': return 5;
    case 'C': case 'c': return 6;
    case 'T': case 't': case 'U': case 'u': return 7;
    default: return 0;
  }
}
static_assert(PA_SUBST_BITS == 3, "the code is three bits");

PA_HD uint64_t bits_of(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
PA_HD double double_of(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

// L(x), the natural logarithm, in fdlibm's scheme.  x = 2^k m with m in [sqrt(1/2), sqrt(2)) taken from the bits;
// f = m - 1 (exact), s = f / (2 + f), z = s^2, R(z) the degree-7 minimax polynomial of (log(1 + s) - log(1 - s) - 2 s) / s,
// in even and odd halves; log m = f - (f^2/2 - s (f^2/2 + R)); ln 2 is split into a high part with 21 trailing zero
// bits, so that k * ln2_hi is exact, and a low part that goes into the correction.  L(1.0) is +0.0.  Not a positive
// finite number: NaN for x < 0 and NaN, -infinity for +-0.0, +infinity for +infinity.
PA_HD double log_strict(double x) {
  constexpr double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10;
  constexpr double kLg1 = 6.666666666666735130e-01, kLg2 = 3.999999999940941908e-01, kLg3 = 2.857142874366239149e-01,
                   kLg4 = 2.222219843214978396e-01, kLg5 = 1.818357216161805012e-01, kLg6 = 1.531383769920937332e-01,
                   kLg7 = 1.479819860511658591e-01;
  constexpr uint64_t kMantissa = (1ull << 52) - 1;
  uint64_t u = bits_of(x);
  if ((u << 1) == 0) return double_of(0xfff0000000000000ull);
  if (u >> 63 || (u >> 52) == 0x7ff) return (u << 1) > (0x7ffull << 53) || u >> 63 ? double_of(0x7ff8000000000000ull) : x;
  int64_t k = 0;
  if ((u >> 52) == 0) {  // subnormal: 2^54 x is normal
    u = bits_of(x * 18014398509481984.0);
    k = -54;
  }
  k += (int64_t)(u >> 52) - 1023;
  const uint64_t mant = u & kMantissa;
  const bool upper = (mant >> 32) >= 0x6a09cu;  // m >= sqrt(2), about: halve it
  k += upper ? 1 : 0;
  const double m = double_of(mant | ((upper ? 0x3feull : 0x3ffull) << 52));
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (kLg2 + w * (kLg4 + w * kLg6));
  const double t2 = z * (kLg1 + w * (kLg3 + w * (kLg5 + w * kLg7)));
  const double r = t2 + t1;
  const double hfsq = (0.5 * f) * f;
  const double dk = (double)k;
  return dk * kLn2Hi - ((hfsq - (s * (hfsq + r) + dk * kLn2Lo)) - f);
}

// why a cell is `missing`
constexpr int kDefined = 0, kNoColumns = 1, kSaturated = 2;

PA_HD bool known_model(int model) { return model == PA_SUBST_MODEL_P || model == PA_SUBST_MODEL_JC69 || model == PA_SUBST_MODEL_K80; }

// D[i, j] from V (columns with a nucleotide in both rows), S (transitions among them) and T (transversions); *why says
// whether the pair is defined
PA_HD double distance(uint32_t i, uint32_t j, uint32_t v, uint32_t s, uint32_t t, int model, double missing, int *why) {
  *why = kDefined;
  if (i == j) return 0.0;
  if (v == 0) { *why = kNoColumns; return missing; }
  const uint64_t changed = (uint64_t)s + t;
  if (changed == 0) return 0.0;
  const double dv = (double)v;
  if (model == PA_SUBST_MODEL_P) return (double)changed / dv;
  if (model == PA_SUBST_MODEL_JC69) {
    const double a = 1.0 - (4.0 * (double)changed) / (3.0 * dv);
    if (a <= 0.0) { *why = kSaturated; return missing; }
    return -0.75 * log_strict(a);
  }
  const double p = (double)s / dv, q = (double)t / dv;
  const double a = (1.0 - 2.0 * p) - q, b = 1.0 - 2.0 * q;
  if (a <= 0.0 || b <= 0.0) { *why = kSaturated; return missing; }
  const double la = -0.5 * log_strict(a), lb = 0.25 * log_strict(b);
  return la - lb;
}

}  // namespace subst
