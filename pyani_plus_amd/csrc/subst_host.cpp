// subst_host.cpp -- phylo-run on the host: the code table, the logarithm as an entry point of its own, and the twins
// pa_msa_subst_counts_host and pa_subst_distances_host of subst.hip (what the kernels are compared with, bit for bit,
// and what phylo-run uses on a machine without a GPU).  include/pyani_hip.h and DESIGN.md section 7m have the contract;
// subst_rule.h has the code, the logarithm and the distance, the same functions the kernels call, compiled here too
// with contraction off (strict_fp.h and the Makefile).
//
// The counts work from the rows as bytes.  A thread takes a pair (i <= j), writes the pair's three masks once -- 0xff
// where the column counts for V, for S and for T -- and then adds, per replicate, the weights under each mask (without
// weights: the masks' own bits).  The sums are integers, so no order shows.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pa_host.h"

#include "msa_boot_rule.h"
#include "subst_rule.h"

namespace {

// the sum of w[c] over the columns where mask[c] is 0xff; w == nullptr: every column once
inline uint32_t column_sum(const uint8_t *w, const uint8_t *mask, uint64_t n) {
  uint32_t total = 0;
  for (uint64_t c0 = 0; c0 < n; c0 += 1u << 16) {  // a block's sum of bytes fits 32 bits with room: the compiler keeps narrow lanes
    const uint64_t c1 = std::min<uint64_t>(n, c0 + (1u << 16));
    uint32_t part = 0;
    if (w)
      for (uint64_t c = c0; c < c1; ++c) part += (uint32_t)(w[c] & mask[c]);
    else
      for (uint64_t c = c0; c < c1; ++c) part += (uint32_t)(mask[c] & 1u);
    total += part;
  }
  return total;
}

bool valid_missing(double missing) { return missing >= 0.0 && missing <= 1.79769313486231570815e308; }

}  // namespace

extern "C" int pa_subst_code(uint8_t *h_code256) {
  if (!h_code256) { pa_set_error("pa_subst_code: null argument"); return PA_E_INVALID; }
  for (uint32_t b = 0; b < 256; ++b) h_code256[b] = subst::code_of(b);
  return PA_OK;
}

extern "C" int pa_subst_log_host(const double *h_x, uint64_t n, double *h_out) {
  if (n && (!h_x || !h_out)) { pa_set_error("pa_subst_log_host: null argument"); return PA_E_INVALID; }
  for (uint64_t i = 0; i < n; ++i) h_out[i] = subst::log_strict(h_x[i]);
  return PA_OK;
}

extern "C" int pa_msa_subst_counts_host(const uint8_t *h_rows, uint64_t row_stride, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights,
                                        uint32_t n_reps, uint32_t *h_valid, uint32_t *h_ts, uint32_t *h_tv, uint32_t n_threads) {
  if (n_rows && n_reps && (!h_valid || !h_ts || !h_tv || (n_cols && !h_rows))) {
    pa_set_error("pa_msa_subst_counts_host: null argument");
    return PA_E_INVALID;
  }
  if (!h_weights && n_reps > 1) { pa_set_error("pa_msa_subst_counts_host: %u replicates without weights; 1 without them", n_reps); return PA_E_INVALID; }
  if (n_cols >= (1ull << 32)) { pa_set_error("pa_msa_subst_counts_host: %llu columns (at most 2^32 - 1)", (unsigned long long)n_cols); return PA_E_INVALID; }
  if (n_rows > 65535) { pa_set_error("pa_msa_subst_counts_host: %u rows; at most 65535", n_rows); return PA_E_INVALID; }
  if (row_stride < n_cols) {
    pa_set_error("pa_msa_subst_counts_host: row stride %llu below the %llu columns", (unsigned long long)row_stride, (unsigned long long)n_cols);
    return PA_E_INVALID;
  }
  if (n_rows == 0 || n_reps == 0) return PA_OK;
  uint32_t max_weight = 0;
  if (h_weights)
    if (const int s = boot::check_weights("pa_msa_subst_counts_host", h_weights, n_cols, n_reps, &max_weight)) return s;
  return pa_host_guard("pa_msa_subst_counts_host", [&]() -> int {
    const uint64_t n = n_rows, nn = n * n, pairs = n * (n + 1) / 2;
    uint8_t code[256];
    for (uint32_t b = 0; b < 256; ++b) code[b] = subst::code_of(b);
    const uint32_t nt = pa_host_threads(pairs * std::max<uint64_t>(n_cols, 1) * n_reps, 1u << 20, n_threads);
    ChunkQueue queue(0, pairs, 1);  // one pair at a time
    HostPool::get().run(nt, [&](uint32_t, uint32_t) {
      std::vector<uint8_t> mv(n_cols), ms(n_cols), mt(n_cols);
      uint64_t i = 0, row_start = 0;  // pairs before row i: the pairs (i', j >= i') of the rows above
      for (uint64_t p, p_end; queue.take(p, p_end);) {
        while (p >= row_start + (n - i)) { row_start += n - i; ++i; }  // p only grows for a thread
        const uint64_t j = i + (p - row_start);
        const uint8_t *q = h_rows + i * row_stride, *s = h_rows + j * row_stride;
        for (uint64_t c = 0; c < n_cols; ++c) {
          const uint8_t a = code[q[c]], b = code[s[c]], x = a ^ b;
          const bool both = (a & b & 4u) != 0;
          mv[c] = both ? 0xff : 0;
          mt[c] = both && (x & 2u) ? 0xff : 0;
          ms[c] = both && !(x & 2u) && (x & 1u) ? 0xff : 0;
        }
        for (uint64_t r = 0; r < n_reps; ++r) {
          const uint8_t *w = h_weights ? h_weights + r * n_cols : nullptr;
          const uint64_t ij = r * nn + i * n + j, ji = r * nn + j * n + i;
          h_valid[ij] = h_valid[ji] = column_sum(w, mv.data(), n_cols);
          h_ts[ij] = h_ts[ji] = column_sum(w, ms.data(), n_cols);
          h_tv[ij] = h_tv[ji] = column_sum(w, mt.data(), n_cols);
        }
      }
    });
    return PA_OK;
  });
}

extern "C" int pa_subst_distances_host(const uint32_t *h_valid, const uint32_t *h_ts, const uint32_t *h_tv, uint32_t n, uint32_t n_reps, int model,
                                       double missing, double *h_D, uint64_t *h_undefined, uint32_t n_threads) {
  const uint64_t nn = (uint64_t)n * n, cells = nn * n_reps;
  if (n_reps && (!h_undefined || (n && (!h_valid || !h_ts || !h_tv || !h_D)))) { pa_set_error("pa_subst_distances_host: null argument"); return PA_E_INVALID; }
  if (!subst::known_model(model)) { pa_set_error("pa_subst_distances_host: unknown model %d (0: p, 1: jc69, 2: k80)", model); return PA_E_INVALID; }
  if (!valid_missing(missing)) {
    pa_set_error("pa_subst_distances_host: the distance of a pair without columns must be finite and not negative");
    return PA_E_INVALID;
  }
  for (uint64_t m = 0; m < 2ull * n_reps; ++m) h_undefined[m] = 0;
  if (cells == 0) return PA_OK;
  return pa_host_guard("pa_subst_distances_host", [&]() -> int {
    const uint64_t rows = (uint64_t)n * n_reps;
    std::vector<std::atomic<uint64_t>> undefined(2ull * n_reps);
    for (auto &u : undefined) u.store(0, std::memory_order_relaxed);
    pa_for_each(0, rows, 64, pa_host_threads(cells, 1u << 14, n_threads), [&](uint64_t row) {
      const uint64_t mat = row / n, base = mat * nn;
      const uint32_t i = (uint32_t)(row % n);
      uint64_t none = 0, saturated = 0;
      for (uint32_t j = 0; j < n; ++j) {
        const uint64_t at = base + (uint64_t)i * n + j;
        int why;
        h_D[at] = subst::distance(i, j, h_valid[at], h_ts[at], h_tv[at], model, missing, &why);
        if (i < j) {
          none += why == subst::kNoColumns;
          saturated += why == subst::kSaturated;
        }
      }
      if (none) undefined[2 * mat].fetch_add(none, std::memory_order_relaxed);
      if (saturated) undefined[2 * mat + 1].fetch_add(saturated, std::memory_order_relaxed);
    });
    for (uint64_t m = 0; m < 2ull * n_reps; ++m) h_undefined[m] = undefined[m].load(std::memory_order_relaxed);
    return PA_OK;
  });
}
