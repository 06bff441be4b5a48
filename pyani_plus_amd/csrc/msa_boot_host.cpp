// msa_boot_host.cpp -- bootstrap-run on the host: the check of a batch of weights (which both paths use), and the
// twins pa_msa_boot_counts_host and pa_msa_boot_distances_host of msa_boot.hip (what the kernels are compared with, bit
// for bit, and what bootstrap-run uses on a machine without a GPU).  include/pyani_hip.h and DESIGN.md section 7l have
// the contract; msa_boot_rule.h has the distance's formula, the same function the kernel calls, compiled here too with
// contraction off (strict_fp.h and the Makefile).
//
// The counts work from the rows as bytes.  A thread takes a pair (i <= j), writes the pair's two masks once -- 0xff
// where the column counts for M, and for B -- and then adds, per replicate, the weights under each mask: two loops of
// byte ANDs that the compiler vectorises.  The sums are integers, so no order shows.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pa_host.h"

#include "msa_boot_rule.h"

int boot::check_weights(const char *who, const uint8_t *h_weights, uint64_t n_cols, uint32_t n_reps, uint32_t *max_weight) {
  uint32_t largest = 0;
  for (uint32_t r = 0; r < n_reps; ++r) {
    const uint8_t *row = h_weights + (uint64_t)r * n_cols;
    uint64_t sum = 0;
    uint8_t top = 0;
    for (uint64_t c = 0; c < n_cols; ++c) {
      sum += row[c];
      top = std::max(top, row[c]);
    }
    if (sum != n_cols) {
      pa_set_error("%s: the weights of replicate %u add up to %llu, not to the %llu columns", who, r, (unsigned long long)sum, (unsigned long long)n_cols);
      return PA_E_INVALID;
    }
    largest = std::max<uint32_t>(largest, top);
  }
  *max_weight = largest;
  return PA_OK;
}

namespace {

constexpr uint8_t kGap = '-';

// the sum of w[c] over the columns where mask[c] is 0xff
inline uint32_t masked_sum(const uint8_t *w, const uint8_t *mask, uint64_t n) {
  uint32_t total = 0;
  for (uint64_t c0 = 0; c0 < n; c0 += 1u << 16) {  // a block's sum of bytes fits 32 bits with room: the compiler keeps narrow lanes
    const uint64_t c1 = std::min<uint64_t>(n, c0 + (1u << 16));
    uint32_t part = 0;
    for (uint64_t c = c0; c < c1; ++c) part += (uint32_t)(w[c] & mask[c]);
    total += part;
  }
  return total;
}

}  // namespace

extern "C" int pa_msa_boot_counts_host(const uint8_t *h_rows, uint64_t row_stride, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights,
                                       uint32_t n_reps, uint32_t *h_match, uint32_t *h_both, uint32_t n_threads) {
  if (n_rows && n_reps && (!h_match || !h_both || (n_cols && (!h_rows || !h_weights)))) {
    pa_set_error("pa_msa_boot_counts_host: null argument");
    return PA_E_INVALID;
  }
  if (n_cols >= (1ull << 32)) { pa_set_error("pa_msa_boot_counts_host: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols); return PA_E_INVALID; }
  if (n_rows > 65535) { pa_set_error("pa_msa_boot_counts_host: %u rows; at most 65535", n_rows); return PA_E_INVALID; }
  if (row_stride < n_cols) {
    pa_set_error("pa_msa_boot_counts_host: row stride %llu below the %llu columns", (unsigned long long)row_stride, (unsigned long long)n_cols);
    return PA_E_INVALID;
  }
  if (n_rows == 0 || n_reps == 0) return PA_OK;
  uint32_t max_weight = 0;
  if (const int s = boot::check_weights("pa_msa_boot_counts_host", h_weights, n_cols, n_reps, &max_weight)) return s;
  return pa_host_guard("pa_msa_boot_counts_host", [&]() -> int {
    const uint64_t n = n_rows, nn = n * n, pairs = n * (n + 1) / 2;
    const uint32_t nt = pa_host_threads(pairs * std::max<uint64_t>(n_cols, 1) * n_reps, 1u << 20, n_threads);
    ChunkQueue queue(0, pairs, 1);  // one pair at a time
    HostPool::get().run(nt, [&](uint32_t, uint32_t) {
      std::vector<uint8_t> eq(n_cols), bt(n_cols);
      uint64_t i = 0, row_start = 0;  // pairs before row i: the pairs (i', j >= i') of the rows above
      for (uint64_t p, p_end; queue.take(p, p_end);) {
        while (p >= row_start + (n - i)) { row_start += n - i; ++i; }  // p only grows for a thread
        const uint64_t j = i + (p - row_start);
        const uint8_t *q = h_rows + i * row_stride, *s = h_rows + j * row_stride;
        for (uint64_t c = 0; c < n_cols; ++c) {
          eq[c] = (q[c] == s[c] && q[c] != kGap) ? 0xff : 0;
          bt[c] = (q[c] != kGap && s[c] != kGap) ? 0xff : 0;
        }
        for (uint64_t r = 0; r < n_reps; ++r) {
          const uint8_t *w = h_weights + r * n_cols;
          const uint32_t m = masked_sum(w, eq.data(), n_cols), b = masked_sum(w, bt.data(), n_cols);
          h_match[r * nn + i * n + j] = h_match[r * nn + j * n + i] = m;
          h_both[r * nn + i * n + j] = h_both[r * nn + j * n + i] = b;
        }
      }
    });
    return PA_OK;
  });
}

extern "C" int pa_msa_boot_distances_host(const uint32_t *h_match, const uint32_t *h_both, uint32_t n, uint32_t n_reps, double missing, double *h_D,
                                          uint32_t n_threads) {
  const uint64_t nn = (uint64_t)n * n, cells = nn * n_reps;
  if (cells && (!h_match || !h_both || !h_D)) { pa_set_error("pa_msa_boot_distances_host: null argument"); return PA_E_INVALID; }
  if (!(missing >= 0.0 && missing <= 1.79769313486231570815e308)) {
    pa_set_error("pa_msa_boot_distances_host: the distance of a pair without columns must be finite and not negative");
    return PA_E_INVALID;
  }
  if (cells == 0) return PA_OK;
  return pa_host_guard("pa_msa_boot_distances_host", [&]() -> int {
    const uint64_t rows = (uint64_t)n * n_reps;
    HostPool::get().run(pa_host_threads(cells, 1u << 16, n_threads), [&](uint32_t id, uint32_t n_workers) {
      for (uint64_t row = rows * id / n_workers; row < rows * (id + 1) / n_workers; ++row) {
        const uint64_t base = row / n * nn;
        const uint32_t i = (uint32_t)(row % n);
        for (uint32_t j = 0; j < n; ++j) {
          const uint64_t at = base + (uint64_t)i * n + j;
          h_D[at] = boot::distance(i, j, h_match[at], h_both[at], h_both[base + (uint64_t)i * n + i], h_both[base + (uint64_t)j * n + j], missing);
        }
      }
    });
    return PA_OK;
  });
}
