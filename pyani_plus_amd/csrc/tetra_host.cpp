// tetra_host.cpp -- host side of the TETRA-hip method: the host twins of tetra.hip's two kernels (what a machine
// without a GPU uses and what the kernels are compared with) and the step between them that has no device form, the
// tetranucleotide Z-scores and their unit rows (256 values per genome).
//
// Replaces nothing in the reference: pyani-plus has no TETRA method.  include/pyani_hip.h states the definition, which
// is this project's own contract (after Teeling et al. 2004); DESIGN.md section 7g has the layout and the measurements.
//
// Every floating-point step below is one IEEE double operation in the order the header gives; a compiler that may use
// FMA instructions would contract a * b + c and change the last bit, so contraction is off for this file (strict_fp.h
// and -ffp-contract=off from the Makefile).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "pa_host.h"

#include "pairs_f64_host.h"

namespace {

constexpr uint32_t kBins = PA_TETRA_BINS, kWords = PA_TETRA_WORDS, kOff3 = 256, kOff2 = 320;

// reverse complement of a word of k digits (first base most significant): the digits reversed, each d -> 3 - d
inline uint32_t rc_word(uint32_t w, int k) {
  uint32_t r = 0;
  for (int i = 0; i < k; ++i) r |= (3u - ((w >> (2 * i)) & 3u)) << (2 * (k - 1 - i));
  return r;
}

// forward counts of the positions [p0, p1) of one genome: a rolling word and the length of the run of valid positions
void count_genome(const uint32_t *packed, const uint32_t *mask, uint64_t p0, uint64_t p1, uint64_t *f) {
  uint32_t word = 0, run = 0;
  for (uint64_t p = p0; p < p1; ++p) {
    if ((mask[p >> 5] >> (p & 31u)) & 1u) {
      run = 0;
      continue;
    }
    word = ((word << 2) | ((packed[p >> 4] >> (2 * (p & 15u))) & 3u)) & 0xffu;
    if (run < 4) ++run;
    if (run >= 2) ++f[kOff2 + (word & 0xfu)];
    if (run >= 3) ++f[kOff3 + (word & 0x3fu)];
    if (run >= 4) ++f[word];
  }
}

inline double finish_r(double acc, bool same) {
  if (acc != acc) return acc;
  if (same) return 1.0;
  return acc > 1.0 ? 1.0 : (acc < -1.0 ? -1.0 : acc);
}

}  // namespace

extern "C" {

int pa_tetra_counts_host(const uint32_t *h_packed, const uint32_t *h_mask, uint64_t arena_bases, const uint64_t *h_genome_start,
                         uint32_t n_genomes, uint64_t *h_counts, uint32_t n_threads) {
  if (!h_genome_start || (n_genomes && !h_counts) || (arena_bases && (!h_packed || !h_mask))) {
    pa_set_error("pa_tetra_counts_host: null argument");
    return PA_E_INVALID;
  }
  if (arena_bases % PA_ALIGN_BASES || h_genome_start[n_genomes] != arena_bases) {
    pa_set_error("pa_tetra_counts_host: arena_bases %llu must be a multiple of %u and equal genome_start[n]", (unsigned long long)arena_bases,
                 PA_ALIGN_BASES);
    return PA_E_INVALID;
  }
  for (uint32_t g = 0; g <= n_genomes; ++g) {
    const uint64_t s = h_genome_start[g];
    if (s % PA_ALIGN_BASES || (g && s < h_genome_start[g - 1]) || s > arena_bases) {
      pa_set_error("pa_tetra_counts_host: genome_start[%u]=%llu must be an ascending multiple of %u inside the arena", g, (unsigned long long)s,
                   PA_ALIGN_BASES);
      return PA_E_INVALID;
    }
  }
  return pa_host_guard("pa_tetra_counts_host", [&]() -> int {
    if (n_genomes) memset(h_counts, 0, (size_t)n_genomes * kBins * sizeof(uint64_t));
    const uint32_t nt = std::min<uint32_t>(pa_host_threads(arena_bases, 1u << 20, n_threads), std::max<uint32_t>(n_genomes, 1u));
    pa_for_each(0, n_genomes, 1, nt, [&](uint64_t g) {  // genomes are handed out one at a time
      count_genome(h_packed, h_mask, h_genome_start[g], h_genome_start[g + 1], h_counts + g * kBins);
    });
    return PA_OK;
  });
}

int pa_tetra_zscores_host(const uint64_t *h_counts, uint32_t n_genomes, double *h_Z, double *h_U) {
  if (n_genomes && (!h_counts || !h_Z || !h_U)) {
    pa_set_error("pa_tetra_zscores_host: null argument");
    return PA_E_INVALID;
  }
  for (uint32_t g = 0; g < n_genomes; ++g) {
    const uint64_t *f = h_counts + (uint64_t)g * kBins;
    double c4[256], c3[64], c2[16];
    for (uint32_t w = 0; w < 256; ++w) c4[w] = (double)(f[w] + f[rc_word(w, 4)]);
    for (uint32_t w = 0; w < 64; ++w) c3[w] = (double)(f[kOff3 + w] + f[kOff3 + rc_word(w, 3)]);
    for (uint32_t w = 0; w < 16; ++w) c2[w] = (double)(f[kOff2 + w] + f[kOff2 + rc_word(w, 2)]);
    double *z = h_Z + (uint64_t)g * kWords, *u = h_U + (uint64_t)g * kWords;
    for (uint32_t w = 0; w < 256; ++w) {
      const double N = c4[w], L = c3[w >> 2], R = c3[w & 63u], M = c2[(w >> 2) & 15u];
      double zw = 0.0;
      if (M != 0.0) {
        const double E = (L * R) / M;
        const double ml = M - L, mr = M - R;
        const double prod = ml * mr;
        const double num = E * prod;
        const double mm = M * M;
        const double V = num / mm;
        if (V > 0.0) {
          const double diff = N - E;
          zw = diff / std::sqrt(V);
        }
      }
      z[w] = zw;
    }
    double sum = 0.0;
    for (uint32_t w = 0; w < 256; ++w) sum = sum + z[w];
    const double mean = sum / 256.0;
    double ss = 0.0;
    for (uint32_t w = 0; w < 256; ++w) {
      const double d = z[w] - mean;
      const double sq = d * d;
      ss = ss + sq;
    }
    if (ss == 0.0) {
      for (uint32_t w = 0; w < 256; ++w) u[w] = std::numeric_limits<double>::quiet_NaN();
    } else {
      const double norm = std::sqrt(ss);
      for (uint32_t w = 0; w < 256; ++w) {
        const double d = z[w] - mean;
        u[w] = d / norm;
      }
    }
  }
  return PA_OK;
}

int pa_tetra_corr_host(const double *h_U, uint32_t n, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, int symmetric, double *h_out,
                       uint32_t n_threads) {
  if (!(q0 <= q1 && q1 <= n && s0 <= s1 && s1 <= n)) {
    pa_set_error("pa_tetra_corr_host: ranges [%u, %u) x [%u, %u) outside the %u genomes", q0, q1, s0, s1, n);
    return PA_E_INVALID;
  }
  if (symmetric && (q0 != s0 || q1 != s1)) {
    pa_set_error("pa_tetra_corr_host: symmetric needs the same query and subject range, not [%u, %u) x [%u, %u)", q0, q1, s0, s1);
    return PA_E_INVALID;
  }
  if (q0 == q1 || s0 == s1) return PA_OK;
  if (!h_U || !h_out) {
    pa_set_error("pa_tetra_corr_host: null argument");
    return PA_E_INVALID;
  }
  return pa_host_guard("pa_tetra_corr_host", [&]() -> int {
    const uint64_t ns = s1 - s0;
    const uint32_t nt = pa_host_threads((uint64_t)(q1 - q0) * ns * kWords, 1u << 20, n_threads);
    pa_for_each(q0, q1, 1, nt, [&](uint32_t i) {
      double *out = h_out + (uint64_t)(i - q0) * ns;
      const uint32_t j_first = symmetric ? i : s0;  // symmetric: row i from the diagonal on, mirrored
      auto finish = [&](uint32_t u, double acc) {
        const uint32_t j = j_first + u;
        const double r = finish_r(acc, i == j);
        out[j - s0] = r;
        if (symmetric) h_out[(uint64_t)(j - q0) * ns + (i - s0)] = r;
      };
      pairs_f64::pair_row_accumulate<pairs_f64::DotTerm>(h_U + (uint64_t)i * kWords, h_U + (uint64_t)j_first * kWords, s1 - j_first, kWords, finish);
    });
    return PA_OK;
  });
}

}  // extern "C"
