// nj_host.cpp -- neighbour joining on the host: what tree-run uses on a machine without a GPU and what nj.hip is compared
// with, bit for bit.  include/pyani_hip.h and DESIGN.md section 7h have the contract; nj_rule.h has its arithmetic, the
// same functions the kernels call, compiled here too with contraction off (strict_fp.h and the Makefile).
//
// The layout is the kernels': the live nodes in slots 0 .. m - 1 of a copy of D, a join puts u into the smaller of its
// two slots and moves the last slot into the larger.  The scan of the live pairs runs on host-pool threads, rows handed
// out a few at a time; each thread keeps its best pair under the total order of the contract and the threads' bests are
// compared under the same order, so the number of threads does not show in the result.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pa_host.h"

#include "distmat_rule.h"
#include "nj_rule.h"

namespace {

using nj::Cand;
using nj::kNone;

constexpr uint32_t kRowsPerTurn = 16;  // rows of the scan a thread takes at a time

}  // namespace

extern "C" int pa_nj_host(const double *h_D, uint32_t n, uint32_t *h_child, double *h_len, uint32_t *h_last, double *h_last_len,
                          uint32_t n_threads) {
  if (n < 1 || n > 65535) { pa_set_error("pa_nj_host: %u nodes; 1 to 65535", n); return PA_E_INVALID; }
  if (!h_D) { pa_set_error("pa_nj_host: null matrix"); return PA_E_INVALID; }
  if (n >= 2 && (!h_last || !h_last_len)) { pa_set_error("pa_nj_host: null argument for the last edge"); return PA_E_INVALID; }
  if (n >= 3 && (!h_child || !h_len)) { pa_set_error("pa_nj_host: null argument for the join table"); return PA_E_INVALID; }
  const uint64_t N = n;
  if (const int s = pa_check_distance_matrix_host("pa_nj_host", "D", h_D, n)) return s;
  if (n == 1) return PA_OK;
  return pa_host_guard("pa_nj_host", [&]() -> int {
    std::vector<double> D(h_D, h_D + N * N);  // the joins overwrite it: work on a copy
    std::vector<double> r(n);
    std::vector<uint32_t> id(n), slot_of(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
      double s = 0.0;
      for (uint32_t k = 0; k < n; ++k) s = s + D[i * N + k];
      r[i] = s;
      id[i] = i;
      slot_of[i] = i;
    }
    std::vector<Cand> bests;
    for (uint32_t t = 0; t + 2 < n; ++t) {
      const uint32_t m = n - t;
      const double m_minus_2 = (double)(m - 2);
      const uint32_t nt = pa_host_threads((uint64_t)m * (m - 1) / 2, 1u << 16, n_threads);
      bests.assign(nt, Cand{0.0, kNone, kNone});
      ChunkQueue rows(0, m - 1, kRowsPerTurn);  // m >= 3 here; the last row has no pair of its own
      HostPool::get().run(nt, [&](uint32_t worker, uint32_t) {
        Cand best{0.0, kNone, kNone};
        for (uint64_t a0, a1; rows.take(a0, a1);) {
          for (uint32_t a = (uint32_t)a0; a < a1; ++a) {
            const double *row = D.data() + a * N;
            const double r_a = r[a];
            const uint32_t id_a = id[a];
            for (uint32_t b = a + 1; b < m; ++b) {
              const bool a_first = id_a < id[b];
              const Cand c{nj::score(m_minus_2, row[b], a_first ? r_a : r[b], a_first ? r[b] : r_a), a_first ? id_a : id[b], a_first ? id[b] : id_a};
              if (nj::better(c, best)) best = c;
            }
          }
        }
        bests[worker] = best;
      });
      Cand best = bests[0];
      for (uint32_t w = 1; w < nt; ++w)
        if (nj::better(bests[w], best)) best = bests[w];
      if (best.lo == kNone) { pa_set_error("pa_nj_host: no live pair at join %u", t); return PA_E_INVALID; }  // never, with m >= 3
      const uint32_t A = slot_of[best.lo], B = slot_of[best.hi], P = std::min(A, B), R = std::max(A, B), L = m - 1, u = n + t;
      const double d = D[A * N + B], r_lo = r[A], r_hi = r[B];
      const double len_lo = nj::length_lo(m_minus_2, d, r_lo, r_hi);
      h_child[2 * (size_t)t] = best.lo;
      h_child[2 * (size_t)t + 1] = best.hi;
      h_len[2 * (size_t)t] = len_lo;
      h_len[2 * (size_t)t + 1] = d - len_lo;
      const double r_u = nj::row_sum_joined((double)m, d, r_lo, r_hi);
      for (uint32_t k = 0; k < m; ++k) {  // u's row and column in slot P, the row sums
        if (k == A || k == B) continue;
        const double d_lo = D[A * N + k], d_hi = D[B * N + k];
        const double d_u = nj::joined_distance(d_lo, d_hi, d);
        r[k] = nj::row_sum_after(r[k], d_lo, d_hi, d_u);
        D[P * N + k] = d_u;
        D[k * N + P] = d_u;
      }
      r[P] = r_u;
      id[P] = u;
      slot_of[u] = P;
      if (R != L) {  // the last slot's node moves into slot R
        for (uint32_t k = 0; k < L; ++k) {
          if (k == R) continue;
          const double v = D[L * N + k];
          D[R * N + k] = v;
          D[k * N + R] = v;
        }
        r[R] = r[L];
        id[R] = id[L];
        slot_of[id[R]] = R;
      }
    }
    h_last[0] = std::min(id[0], id[1]);
    h_last[1] = std::max(id[0], id[1]);
    *h_last_len = D[1];
    return PA_OK;
  });
}
