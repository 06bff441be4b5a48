// derep_host.cpp -- dereplicate-run on the host: the refusals of the three calls (which the device entry points share)
// and the twins pa_derep_adjacency_host, pa_derep_select_host and pa_derep_assign_host: what derep.hip is compared with,
// bit for bit, and what dereplicate-run uses on a machine without a GPU.  include/pyani_hip.h and DESIGN.md section 7k
// have the contract; derep_rule.h has its rules, the same functions the kernels call, compiled here too with contraction
// off (strict_fp.h and the Makefile).
//
// The twins are the plain sequential algorithms.  Adjacency and assignment hand out rows to host-pool threads, each row
// made by one thread, so the number of threads does not show in a result; the selection is one thread's loop.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "pa_host.h"

#include "derep_rule.h"

namespace {

constexpr uint32_t kStrip = 64;  // rows a thread takes at a time: one word of the columns they are transposed from

int refuse_n(const char *who, uint32_t n) {
  pa_set_error("%s: %u genomes; 1 to %u", who, n, derep::kMaxN);
  return PA_E_INVALID;
}

inline bool bit(const uint64_t *words, uint32_t p) { return (words[p >> 6] >> (p & 63u)) & 1u; }

}  // namespace

int derep::check_adjacency(const void *S, const void *C, uint32_t n, int agg_score, int agg_cov, double min_score, double cov_min, const void *bits) {
  if (n < 1 || n > kMaxN) return refuse_n("pa_derep_adjacency", n);
  if (!S || !C || !bits) { pa_set_error("pa_derep_adjacency: null argument"); return PA_E_INVALID; }
  if (!agg_ok(agg_score) || !agg_ok(agg_cov)) {
    pa_set_error("pa_derep_adjacency: aggregators %d, %d (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)", agg_score, agg_cov);
    return PA_E_INVALID;
  }
  if (min_score != min_score) { pa_set_error("pa_derep_adjacency: min_score is NaN"); return PA_E_INVALID; }
  if (cov_min != cov_min) { pa_set_error("pa_derep_adjacency: cov_min is NaN"); return PA_E_INVALID; }
  return PA_OK;
}

int derep::check_select(const void *bits, uint32_t n, int mode, const void *is_rep, const void *n_reps) {
  if (n < 1 || n > kMaxN) return refuse_n("pa_derep_select", n);
  if (!bits || !is_rep || !n_reps) { pa_set_error("pa_derep_select: null argument"); return PA_E_INVALID; }
  if (!mode_ok(mode)) { pa_set_error("pa_derep_select: mode %d (PA_DEREP_GREEDY or PA_DEREP_COVER)", mode); return PA_E_INVALID; }
  return PA_OK;
}

int derep::check_assign(const void *S, uint32_t n, int agg_score, const void *bits, const void *is_rep, const void *rep, const void *rep_score) {
  if (n < 1 || n > kMaxN) return refuse_n("pa_derep_assign", n);
  if (!S || !bits || !is_rep || !rep || !rep_score) { pa_set_error("pa_derep_assign: null argument"); return PA_E_INVALID; }
  if (!agg_ok(agg_score)) { pa_set_error("pa_derep_assign: aggregator %d (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)", agg_score); return PA_E_INVALID; }
  return PA_OK;
}

extern "C" int pa_derep_adjacency_host(const double *h_S, const double *h_C, uint32_t n, int agg_score, int agg_cov, double min_score, double cov_min,
                                       uint64_t *h_bits, uint32_t n_threads) {
  if (const int s = derep::check_adjacency(h_S, h_C, n, agg_score, agg_cov, min_score, cov_min, h_bits)) return s;
  return pa_host_guard("pa_derep_adjacency_host", [&]() -> int {
    const uint64_t N = n, W = derep::words(n);
    // A strip of rows a0 .. a0 + rows - 1: the columns of the same numbers are transposed first (kStrip contiguous doubles
    // of every row b), so that the pair loop reads both directions along b.
    pa_for_chunks(0, n, kStrip, pa_host_threads(N * N, 1u << 16, n_threads), [&](uint32_t, uint64_t a0, uint64_t a1) {
      const uint32_t rows = (uint32_t)(a1 - a0);
      std::vector<double> t_s((size_t)kStrip * N), t_c((size_t)kStrip * N);
      for (uint64_t b = 0; b < N; ++b)
        for (uint32_t r = 0; r < rows; ++r) {
          t_s[r * N + b] = h_S[b * N + a0 + r];
          t_c[r * N + b] = h_C[b * N + a0 + r];
        }
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t a = (uint32_t)a0 + r;
        uint64_t *out = h_bits + a * W;
        for (uint64_t w = 0; w < W; ++w) {
          uint64_t word = 0;
          for (uint32_t k = 0; k < 64 && w * 64 + k < N; ++k) {
            const uint32_t b = (uint32_t)(w * 64 + k);
            bool adjacent = a == b;
            if (!adjacent) {
              const double score = derep::pair_value(agg_score, a, b, h_S[a * N + b], t_s[r * N + b]);
              const double cov = derep::pair_value(agg_cov, a, b, h_C[a * N + b], t_c[r * N + b]);
              adjacent = derep::edge(score, cov, min_score, cov_min);
            }
            word |= (uint64_t)adjacent << k;
          }
          out[w] = word;
        }
      }
    });
    return PA_OK;
  });
}

extern "C" int pa_derep_select_host(const uint64_t *h_bits, uint32_t n, int mode, uint8_t *h_is_rep, uint32_t *n_reps) {
  if (const int s = derep::check_select(h_bits, n, mode, h_is_rep, n_reps)) return s;
  return pa_host_guard("pa_derep_select_host", [&]() -> int {
    const uint64_t W = derep::words(n);
    uint32_t reps = 0;
    memset(h_is_rep, 0, n);
    if (mode == PA_DEREP_GREEDY) {
      std::vector<uint64_t> taken(W, 0);  // the closed neighbourhoods of the representatives so far
      for (uint32_t p = 0; p < n; ++p) {
        if (bit(taken.data(), p)) continue;
        h_is_rep[p] = 1;
        ++reps;
        const uint64_t *row = h_bits + p * W;
        for (uint64_t w = 0; w < W; ++w) taken[w] |= row[w];
      }
      *n_reps = reps;
      return PA_OK;
    }
    std::vector<uint64_t> uncovered(W, ~0ull);
    if (n % 64) uncovered[W - 1] = ~0ull >> (64 - n % 64);
    for (uint32_t left = n; left > 0;) {
      uint64_t best = 0;
      for (uint32_t p = 0; p < n; ++p) {
        const uint64_t *row = h_bits + p * W;
        uint32_t gain = 0;
        for (uint64_t w = 0; w < W; ++w) gain += (uint32_t)__builtin_popcountll(row[w] & uncovered[w]);
        best = std::max(best, derep::cover_key(gain, bit(uncovered.data(), p), p));
      }
      const uint32_t gain = derep::cover_key_gain(best), p = derep::cover_key_node(best);
      if (gain == 0 || p >= n) {  // a matrix whose diagonal is not set: outside the contract, and no loop without end
        pa_set_error("pa_derep_select: %u nodes are in no row's neighbourhood: the diagonal of the bit matrix is not set", left);
        return PA_E_INVALID;
      }
      if (gain == 1) {  // the rule above chooses the uncovered nodes one after the other, each covering itself alone
        for (uint32_t q = 0; q < n; ++q)
          if (bit(uncovered.data(), q)) {
            h_is_rep[q] = 1;
            ++reps;
          }
        break;
      }
      h_is_rep[p] = 1;
      ++reps;
      left -= gain;
      const uint64_t *row = h_bits + p * W;
      for (uint64_t w = 0; w < W; ++w) uncovered[w] &= ~row[w];
    }
    *n_reps = reps;
    return PA_OK;
  });
}

extern "C" int pa_derep_assign_host(const double *h_S, uint32_t n, int agg_score, const uint64_t *h_bits, const uint8_t *h_is_rep, uint32_t *h_rep,
                                    double *h_rep_score, uint32_t n_threads) {
  if (const int s = derep::check_assign(h_S, n, agg_score, h_bits, h_is_rep, h_rep, h_rep_score)) return s;
  return pa_host_guard("pa_derep_assign_host", [&]() -> int {
    const uint64_t N = n, W = derep::words(n);
    pa_for_chunks(0, n, kStrip, pa_host_threads(N * W, 1u << 16, n_threads), [&](uint32_t, uint64_t p0, uint64_t p1) {
      for (uint32_t p = (uint32_t)p0; p < p1; ++p) {
        derep::Pick best{std::numeric_limits<double>::quiet_NaN(), derep::kNone};
        if (h_is_rep[p]) {
          best = derep::Pick{derep::pair_value(agg_score, p, p, h_S[p * N + p], h_S[p * N + p]), p};
        } else {
          const uint64_t *row = h_bits + p * W;
          for (uint64_t w = 0; w < W; ++w)
            for (uint64_t m = row[w]; m; m &= m - 1) {
              const uint32_t q = (uint32_t)(w * 64 + (uint32_t)__builtin_ctzll(m));
              if (q >= n || q == p || !h_is_rep[q]) continue;
              const derep::Pick c{derep::pair_value(agg_score, p, q, h_S[p * N + q], h_S[q * N + p]), q};
              if (c.score == c.score && derep::better(c, best)) best = c;
            }
        }
        h_rep[p] = best.rep;
        h_rep_score[p] = best.score;
      }
    });
    return PA_OK;
  });
}
