// mantel_host.cpp -- mantel-run-comp on the host: the permutations of a seed (pa_mantel_permutations, which both paths
// use), the argument checks of both entry points, and pa_mantel_host, the twin of pa_mantel (what mantel.hip is compared
// with, bit for bit, and what mantel-run-comp uses on a machine without a GPU).  include/pyani_hip.h and DESIGN.md
// section 7j have the contract; mantel_rule.h has its constants and formulas, the same functions the kernels call,
// compiled here too with contraction off (strict_fp.h and the Makefile).
//
// The twin hands out rows of X to host-pool threads, a batch of permutations at a time, so that a row of X stays in
// cache across the batch.  A row's sum is made by one thread in the contract's order and the chains over the rows by the
// calling thread, so neither the number of threads nor the batch shows in a result.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pa_host.h"

#include "distmat_rule.h"
#include "mantel_rule.h"

namespace {

using mantel::kSumStart;

constexpr uint32_t kRowsPerTurn = 8;   // rows a thread takes at a time
constexpr uint64_t kHostBatch = 64;    // permutations a row of X is kept for
constexpr uint32_t kNoPlace = 0xFFFFFFFFu;

// (((-0.0 + v[0]) + v[1]) + ...) + v[n - 1]
double chain(const double *v, uint32_t n) {
  double s = kSumStart;
  for (uint32_t i = 0; i < n; ++i) s = s + v[i];
  return s;
}

}  // namespace

// inv[row[t]] = t for a row that is a permutation; otherwise false at the first value that is out of range or repeated,
// which is then at position *at (inv starts as kNoPlace throughout)
static bool invert_row(const uint32_t *row, uint32_t n, uint32_t *inv, uint32_t *at) {
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t v = row[t];
    if (v >= n || inv[v] != kNoPlace) { *at = t; return false; }
    inv[v] = t;
  }
  return true;
}

int mantel::check_arguments(const void *X, const void *Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, const void *h_stats,
                            const void *h_cross, std::vector<uint32_t> *inverse) {
  if (!X || !Y || !h_stats || !h_cross || (n_perms && !h_perms)) { pa_set_error("pa_mantel: null argument"); return PA_E_INVALID; }
  if (n < 3 || n > PA_MANTEL_MAX_N) { pa_set_error("pa_mantel: %u genomes; 3 to %d", n, PA_MANTEL_MAX_N); return PA_E_INVALID; }
  return pa_host_guard("pa_mantel", [&]() -> int {
    inverse->assign((size_t)(n_perms + 1) * n, kNoPlace);
    for (uint32_t t = 0; t < n; ++t) (*inverse)[t] = t;
    // the rows are independent: host-pool threads invert them and keep the number of the first that is no permutation
    constexpr uint64_t kRowsATurn = 16;
    std::atomic<uint64_t> first_bad{UINT64_MAX};
    pa_for_each(0, n_perms, kRowsATurn, pa_host_threads(n_perms * n, 1u << 18, 0), [&](uint64_t q) {
      uint32_t at = 0;
      if (invert_row(h_perms + q * n, n, inverse->data() + (q + 1) * n, &at)) return;
      uint64_t seen = first_bad.load(std::memory_order_relaxed);
      while (q < seen && !first_bad.compare_exchange_weak(seen, q, std::memory_order_relaxed)) {}
    });
    const uint64_t q = first_bad.load();
    if (q == UINT64_MAX) return PA_OK;
    const uint32_t *row = h_perms + q * n;
    std::vector<uint32_t> inv(n, kNoPlace);
    uint32_t at = 0;
    (void)invert_row(row, n, inv.data(), &at);
    if (row[at] >= n)
      pa_set_error("pa_mantel: row %llu of the permutations holds %u at position %u: out of range for %u genomes", (unsigned long long)q, row[at], at, n);
    else
      pa_set_error("pa_mantel: row %llu of the permutations holds %u at position %u: repeated from position %u", (unsigned long long)q, row[at], at,
                   inv[row[at]]);
    return PA_E_INVALID;
  });
}

extern "C" int pa_mantel_permutations(uint64_t seed, uint32_t n, uint64_t first, uint64_t count, uint32_t *h_perms) {
  if (n < 1 || n > PA_MANTEL_MAX_N) { pa_set_error("pa_mantel_permutations: %u genomes; 1 to %d", n, PA_MANTEL_MAX_N); return PA_E_INVALID; }
  if (count && !h_perms) { pa_set_error("pa_mantel_permutations: null argument"); return PA_E_INVALID; }
  const uint64_t seeded = mantel::fin(seed);
  for (uint64_t r = 0; r < count; ++r) {
    uint32_t *row = h_perms + r * n;
    const uint64_t base = mantel::fin(seeded + (first + r));
    for (uint32_t t = 0; t < n; ++t) row[t] = t;
    // the modulo prefers the small remainders by less than (t + 1) / 2^64 < 2^-48 for t < 2^14: no rejection
    for (uint32_t t = n - 1; t >= 1; --t) std::swap(row[t], row[mantel::fin(base + t) % ((uint64_t)t + 1)]);
  }
  return PA_OK;
}

extern "C" int pa_mantel_host(const double *h_X, const double *h_Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, double *h_stats,
                              double *h_cross, uint32_t n_threads) {
  return pa_host_guard("pa_mantel_host", [&]() -> int {
    std::vector<uint32_t> inverse;
    if (const int s = mantel::check_arguments(h_X, h_Y, n, h_perms, n_perms, h_stats, h_cross, &inverse)) return s;
    const uint64_t N = n;
    const uint32_t *identity = inverse.data();
    const std::pair<const char *, const double *> matrices[2] = {{"X", h_X}, {"Y", h_Y}};
    for (const auto &[name, M] : matrices)
      if (const int s = pa_check_distance_matrix_host("pa_mantel", name, M, n)) return s;
    // the moments
    std::vector<double> rows(N * std::min<uint64_t>(kHostBatch, n_perms + 1));
    const double pairs = (double)(N * (N - 1) / 2);
    double mean[2], ss[2];
    for (int m = 0; m < 2; ++m) {
      const double *M = matrices[m].second;
      pa_for_each(0, n, kRowsPerTurn, pa_host_threads(N * (N / 2), 1u << 16, n_threads), [&](uint32_t i) {
        const double *row = M + i * N;
        rows[i] = mantel::row_sum(i, n, [row](double acc, uint32_t j) { return acc + row[j]; });
      });
      const double mu = mean[m] = chain(rows.data(), n) / pairs;
      pa_for_each(0, n, kRowsPerTurn, pa_host_threads(N * (N / 2), 1u << 16, n_threads), [&](uint32_t i) {
        const double *row = M + i * N;
        rows[i] = mantel::row_sum(i, n, [row, mu](double acc, uint32_t j) { return mantel::add_square(acc, mantel::centred(row[j], mu)); });
      });
      ss[m] = chain(rows.data(), n);
    }
    h_stats[0] = mean[0], h_stats[1] = mean[1], h_stats[2] = ss[0], h_stats[3] = ss[1];
    // the cross sums: entry 0 is the identity's, entry 1 + q that of row q
    const double mean_x = mean[0], mean_y = mean[1];
    for (uint64_t g0 = 0; g0 <= n_perms; g0 += kHostBatch) {
      const uint64_t g1 = std::min(g0 + kHostBatch, n_perms + 1);
      pa_for_each(0, n, kRowsPerTurn, pa_host_threads(N * (N / 2 * (g1 - g0)), 1u << 16, n_threads), [&](uint32_t i) {
        const double *x_row = h_X + i * N;
        for (uint64_t g = g0; g < g1; ++g) {
          const uint32_t *pi = g ? h_perms + (g - 1) * N : identity;
          const double *y_row = h_Y + pi[i] * N;
          rows[(g - g0) * N + i] = mantel::row_sum(i, n, [=](double acc, uint32_t j) {
            return mantel::add_product(acc, mantel::centred(x_row[j], mean_x), mantel::centred(y_row[pi[j]], mean_y));
          });
        }
      });
      for (uint64_t g = g0; g < g1; ++g) h_cross[g] = chain(rows.data() + (g - g0) * N, n);
    }
    return PA_OK;
  });
}
