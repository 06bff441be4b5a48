// pcoa_host.cpp -- ordinate-run on the host: the twins of the tall product and of the centring (what pcoa.hip is compared
// with, bit for bit, and what ordinate-run uses on a machine without a GPU), and the eigen-solver, which lives here
// alone: pa_symm_top_eigs (pcoa.hip) and pa_symm_top_eigs_host both call pcoa::top_eigs and hand it their product.
// include/pyani_hip.h and DESIGN.md section 7i have the contract; pcoa_rule.h has its constants and formulas, the same
// functions the kernels call, compiled here too with contraction off (strict_fp.h and the Makefile).
//
// The twins hand out rows to host-pool threads; a row's sums are made by one thread in the contract's order, so the
// number of threads does not show in the result.  The solver's p-wide algebra runs on the calling thread.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pa_host.h"

#include "distmat_rule.h"
#include "pcoa_rule.h"
#include "pcoa_solver.h"

namespace {

using pcoa::kChunk;
using pcoa::kSumStart;

constexpr uint32_t kRowsPerTurn = 16;   // rows a thread takes at a time
constexpr uint32_t kPhase1Cap = 200;    // iterations of the unshifted phase, at most
constexpr int kJacobiSweeps = 100;      // cyclic Jacobi converges quadratically: a dozen sweeps in practice
constexpr double kDependent = 1e-8;     // a column that keeps less than this share of its norm is replaced, not normalised
constexpr int kDotLanes = 8;            // partial sums of the solver's dot products

// ---- the solver's vector operations: each a fixed order of single operations, whatever the caller
// x . y with kDotLanes accumulators: element i goes to accumulator i % kDotLanes, the accumulators are added pairwise
double dot(const double *x, const double *y, uint32_t n) {
  double acc[kDotLanes];
  for (int l = 0; l < kDotLanes; ++l) acc[l] = 0.0;
  uint32_t i = 0;
  for (; i + kDotLanes <= n; i += kDotLanes)
    for (int l = 0; l < kDotLanes; ++l) acc[l] = pcoa::mul_add(acc[l], x[i + l], y[i + l]);
  for (int l = 0; i < n; ++i, ++l) acc[l] = pcoa::mul_add(acc[l], x[i], y[i]);
  return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}
static_assert(kDotLanes == 8, "dot adds its eight accumulators by name");

// y += a x
void axpy(double a, const double *x, double *y, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) y[i] = pcoa::mul_add(y[i], a, x[i]);
}

// The eigen-decomposition of the symmetric p x p matrix a (row-major, destroyed) by cyclic Jacobi: a = v diag(w) v^T,
// the eigenvectors in the columns of v.  A rotation is skipped where the off-diagonal cell no longer changes either
// diagonal cell it touches.
void jacobi(std::vector<double> &a, uint32_t p, std::vector<double> &w, std::vector<double> &v) {
  v.assign((size_t)p * p, 0.0);
  for (uint32_t i = 0; i < p; ++i) v[(size_t)i * p + i] = 1.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0;
    for (uint32_t i = 0; i < p; ++i)
      for (uint32_t j = i + 1; j < p; ++j) off = off + std::fabs(a[(size_t)i * p + j]);
    if (off == 0.0) break;
    for (uint32_t x = 0; x < p; ++x) {
      for (uint32_t y = x + 1; y < p; ++y) {
        const double axy = a[(size_t)x * p + y];
        if (axy == 0.0) continue;
        const double axx = a[(size_t)x * p + x], ayy = a[(size_t)y * p + y];
        const double g = 100.0 * std::fabs(axy);
        if (std::fabs(axx) + g == std::fabs(axx) && std::fabs(ayy) + g == std::fabs(ayy)) {
          a[(size_t)x * p + y] = a[(size_t)y * p + x] = 0.0;
          continue;
        }
        const double h = ayy - axx;
        double t;
        if (std::fabs(h) + g == std::fabs(h)) {
          t = axy / h;
        } else {
          const double theta = 0.5 * h / axy;
          t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
          if (theta < 0.0) t = -t;
        }
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        a[(size_t)x * p + x] = axx - t * axy;
        a[(size_t)y * p + y] = ayy + t * axy;
        a[(size_t)x * p + y] = a[(size_t)y * p + x] = 0.0;
        for (uint32_t r = 0; r < p; ++r) {
          if (r != x && r != y) {
            const double arx = a[(size_t)r * p + x], ary = a[(size_t)r * p + y];
            const double nx = c * arx - s * ary, ny = s * arx + c * ary;
            a[(size_t)r * p + x] = a[(size_t)x * p + r] = nx;
            a[(size_t)r * p + y] = a[(size_t)y * p + r] = ny;
          }
          const double vrx = v[(size_t)r * p + x], vry = v[(size_t)r * p + y];
          v[(size_t)r * p + x] = c * vrx - s * vry;
          v[(size_t)r * p + y] = s * vrx + c * vry;
        }
      }
    }
  }
  w.resize(p);
  for (uint32_t i = 0; i < p; ++i) w[i] = a[(size_t)i * p + i];
}

// The columns of `cols` (p of them, n long each, one after the other) orthonormalised in place by twice-applied
// modified Gram-Schmidt.  A column that vanishes against the ones before it (it keeps at most kDependent of its norm)
// is replaced: by fresh start values first, by the unit vectors in turn after three of those.
struct Orthonormaliser {
  uint32_t n, p;
  uint64_t fresh = 0;  // start values handed out so far, after the start block's n p
  void fill_fresh(double *v) {
    for (uint32_t i = 0; i < n; ++i) v[i] = pcoa::start_value((uint64_t)n * p + fresh + i);
    fresh += n;
  }
  // v against the first c columns, twice; returns the norm that is left
  double project(const double *cols, uint32_t c, double *v) const {
    for (int pass = 0; pass < 2; ++pass)
      for (uint32_t d = 0; d < c; ++d) {
        const double *q = cols + (size_t)d * n;
        axpy(-dot(q, v, n), q, v, n);
      }
    return std::sqrt(dot(v, v, n));
  }
  void run(double *cols) {
    for (uint32_t c = 0; c < p; ++c) {
      double *v = cols + (size_t)c * n;
      const double before = std::sqrt(dot(v, v, n));
      double left = project(cols, c, v);
      uint32_t unit = 0;
      for (int tries = 0; !(left > kDependent * before) || !std::isfinite(left); ++tries) {
        double start = 1.0;
        if (tries < 3) {
          fill_fresh(v);
          start = std::sqrt(dot(v, v, n));
        } else {
          if (unit >= n) break;  // never: c < p <= n orthonormal columns leave some unit vector a share of 1 / sqrt(n)
          for (uint32_t i = 0; i < n; ++i) v[i] = i == unit ? 1.0 : 0.0;
          ++unit;
        }
        left = project(cols, c, v);
        if (left > kDependent * start && std::isfinite(left)) break;
        left = 0.0;  // this candidate vanished too: the next one
      }
      const double inv = 1.0 / left;
      for (uint32_t i = 0; i < n; ++i) v[i] = v[i] * inv;
    }
  }
};

void to_rows(const std::vector<double> &cols, uint32_t n, uint32_t p, std::vector<double> &rows) {
  for (uint32_t c = 0; c < p; ++c)
    for (uint32_t i = 0; i < n; ++i) rows[(size_t)i * p + c] = cols[(size_t)c * n + i];
}
void to_cols(const std::vector<double> &rows, uint32_t n, uint32_t p, std::vector<double> &cols) {
  for (uint32_t c = 0; c < p; ++c)
    for (uint32_t i = 0; i < n; ++i) cols[(size_t)c * n + i] = rows[(size_t)i * p + c];
}

}  // namespace

int pcoa::top_eigs(const char *what, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2, const Product &product,
                   double *h_values, double *h_vectors, double *h_residuals, double *h_info) {
  if (n < 1 || n > 65535) { pa_set_error("%s: %u rows; 1 to 65535", what, n); return PA_E_INVALID; }
  if (k < 1 || k > n || k > PA_EIGS_MAX_K) {
    pa_set_error("%s: %u eigenpairs of a matrix of %u rows; 1 to min(n, %d)", what, k, n, PA_EIGS_MAX_K);
    return PA_E_INVALID;
  }
  if (!(tol > 0.0) || !std::isfinite(tol)) { pa_set_error("%s: a tolerance of %g; it must be finite and above 0", what, tol); return PA_E_INVALID; }
  if (max_iter < 1) { pa_set_error("%s: max_iter 0; at least 1", what); return PA_E_INVALID; }
  if (!std::isfinite(fro2) || fro2 < 0.0) { pa_set_error("%s: a squared Frobenius norm of %g; it must be finite and not negative", what, fro2); return PA_E_INVALID; }
  if (!h_values || !h_vectors || !h_residuals || !h_info) { pa_set_error("%s: null output", what); return PA_E_INVALID; }
  return pa_host_guard(what, [&]() -> int {
    // the block: twice the pairs asked for, eight more at least, as wide as the product allows at most
    const uint32_t p = std::min({n, std::max(2 * k, k + 8), (uint32_t)PA_MUL_TALL_MAX_P});
    static_assert(PA_EIGS_MAX_K + 8 <= PA_MUL_TALL_MAX_P, "the widest block still has eight columns beyond the pairs asked for");
    const size_t np = (size_t)n * p;
    std::vector<double> Q(np), Y(np), rows_q(np), rows_y(np), X((size_t)n * k), R(n);
    std::vector<double> H((size_t)p * p), Hs((size_t)p * p), theta, S, lambda(p), resid(k);
    std::vector<uint32_t> order(p);
    for (uint32_t c = 0; c < p; ++c)
      for (uint32_t i = 0; i < n; ++i) Q[(size_t)c * n + i] = pcoa::start_value((uint64_t)i * p + c);
    Orthonormaliser orth{n, p};
    orth.run(Q.data());
    double sigma = 0.0, worst = 0.0, bound = 0.0;
    uint32_t phase = 1, phase1_iterations = 0;
    bool refresh = false;
    for (uint32_t it = 1; it <= max_iter; ++it) {
      to_rows(Q, n, p, rows_q);
      const int status = product(rows_q.data(), p, rows_y.data());
      if (status != PA_OK) return status;
      to_cols(rows_y, n, p, Y);
      if (sigma != 0.0) axpy(sigma, Q.data(), Y.data(), (uint32_t)np);  // Y += sigma Q
      for (uint32_t a = 0; a < p; ++a)
        for (uint32_t b = 0; b < p; ++b) H[(size_t)a * p + b] = dot(Q.data() + (size_t)a * n, Y.data() + (size_t)b * n, n);
      for (uint32_t a = 0; a < p; ++a)
        for (uint32_t b = 0; b < p; ++b) Hs[(size_t)a * p + b] = 0.5 * (H[(size_t)a * p + b] + H[(size_t)b * p + a]);
      jacobi(Hs, p, theta, S);
      for (uint32_t c = 0; c < p; ++c) {
        order[c] = c;
        if (!std::isfinite(theta[c])) { pa_set_error("%s: a Ritz value is not finite at iteration %u: the matrix is not finite", what, it); return PA_E_INVALID; }
      }
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return theta[a] > theta[b]; });
      double scale = 0.0;
      for (uint32_t c = 0; c < p; ++c) {
        lambda[c] = theta[order[c]] - sigma;
        scale = std::max(scale, std::fabs(lambda[c]));
      }
      // the first k Ritz vectors X = Q S and their residuals R = Y S - X theta
      bound = tol * scale;
      worst = 0.0;
      bool all_converged = true;
      for (uint32_t c = 0; c < k; ++c) {
        double *x = X.data() + (size_t)c * n;
        std::fill(x, x + n, 0.0);
        std::fill(R.begin(), R.end(), 0.0);
        for (uint32_t d = 0; d < p; ++d) {
          const double s = S[(size_t)d * p + order[c]];
          axpy(s, Q.data() + (size_t)d * n, x, n);
          axpy(s, Y.data() + (size_t)d * n, R.data(), n);
        }
        axpy(-theta[order[c]], x, R.data(), n);
        resid[c] = std::sqrt(dot(R.data(), R.data(), n));
        worst = std::max(worst, resid[c]);
        all_converged = all_converged && resid[c] <= bound;
      }
      bool done = false;
      if (phase == 1) {
        phase1_iterations = it;
        if (all_converged || it == kPhase1Cap) {
          double sum = 0.0;
          for (uint32_t c = 0; c < k; ++c)
            if (resid[c] <= bound) sum = sum + lambda[c] * lambda[c];
          const double rho = std::sqrt(std::max(fro2 - sum, 0.0));
          if (all_converged && lambda[k - 1] > rho) {
            done = true;  // certified: no eigenvalue left out exceeds rho
          } else {
            phase = 2;
            sigma = rho;
            refresh = all_converged;
          }
        }
      } else {
        done = all_converged;
      }
      if (done) {
        for (uint32_t c = 0; c < k; ++c) {
          const double *x = X.data() + (size_t)c * n;
          uint32_t at = 0;
          for (uint32_t i = 1; i < n; ++i)
            if (std::fabs(x[i]) > std::fabs(x[at])) at = i;
          const double sign = x[at] < 0.0 ? -1.0 : 1.0;
          for (uint32_t i = 0; i < n; ++i) h_vectors[(size_t)i * k + c] = sign * x[i];
          h_values[c] = lambda[c];
          h_residuals[c] = resid[c];
        }
        h_info[0] = (double)phase1_iterations;
        h_info[1] = (double)it;
        h_info[2] = sigma;
        return PA_OK;
      }
      if (refresh) {
        // Every pair converged and yet something larger may be left out: the block spans an invariant subspace, which
        // no product leads out of, shifted or not.  Phase 2 keeps the k Ritz vectors and starts the other columns afresh.
        std::copy(X.begin(), X.end(), Q.begin());
        for (uint32_t c = k; c < p; ++c) orth.fill_fresh(Q.data() + (size_t)c * n);
        refresh = false;
      } else {
        Q.swap(Y);
      }
      orth.run(Q.data());
    }
    pa_set_error("%s: no convergence in %u iterations (%u of them in phase 1, shift %g): the worst residual of the first %u pairs is %g, the bound %g",
                 what, max_iter, phase1_iterations, sigma, k, worst, bound);
    return PA_E_NOCONVERGE;
  });
}

extern "C" int pa_mul_tall_f64_host(const double *h_A, uint32_t n, const double *h_Q, uint32_t p, double *h_Y, uint32_t n_threads) {
  if (n < 1 || n > 65535) { pa_set_error("pa_mul_tall_f64_host: %u rows; 1 to 65535", n); return PA_E_INVALID; }
  if (p < 1 || p > PA_MUL_TALL_MAX_P) { pa_set_error("pa_mul_tall_f64_host: %u columns; 1 to %d", p, PA_MUL_TALL_MAX_P); return PA_E_INVALID; }
  if (!h_A || !h_Q || !h_Y) { pa_set_error("pa_mul_tall_f64_host: null argument"); return PA_E_INVALID; }
  return pa_host_guard("pa_mul_tall_f64_host", [&]() -> int {
    pa_for_each(0, n, kRowsPerTurn, pa_host_threads((uint64_t)n * n * p, 1u << 16, n_threads), [&](uint32_t i) {
      const double *row = h_A + (size_t)i * n;
      double y[PA_MUL_TALL_MAX_P], s[PA_MUL_TALL_MAX_P];
      for (uint32_t c = 0; c < p; ++c) y[c] = kSumStart;
      for (uint32_t j0 = 0; j0 < n; j0 += kChunk) {
        const uint32_t j1 = std::min<uint32_t>(j0 + kChunk, n);
        for (uint32_t c = 0; c < p; ++c) s[c] = kSumStart;
        for (uint32_t j = j0; j < j1; ++j) {
          const double a = row[j];
          const double *q = h_Q + (size_t)j * p;
          for (uint32_t c = 0; c < p; ++c) s[c] = pcoa::mul_add(s[c], a, q[c]);
        }
        for (uint32_t c = 0; c < p; ++c) y[c] = y[c] + s[c];
      }
      memcpy(h_Y + (size_t)i * p, y, (size_t)p * 8);
    });
    return PA_OK;
  });
}

extern "C" int pa_gower_center_host(const double *h_D, uint32_t n, double *h_B, double *h_trace, double *h_fro2, uint32_t n_threads) {
  if (n < 1 || n > 65535) { pa_set_error("pa_gower_center_host: %u rows; 1 to 65535", n); return PA_E_INVALID; }
  if (!h_D || !h_B || !h_trace || !h_fro2) { pa_set_error("pa_gower_center_host: null argument"); return PA_E_INVALID; }
  const uint64_t N = n;
  if (const int s = pa_check_distance_matrix_host("pa_gower_center_host", "D", h_D, n)) return s;
  return pa_host_guard("pa_gower_center_host", [&]() -> int {
    std::vector<double> r(n), row_sq(n);
    const double count = (double)n;
    pa_for_each(0, n, kRowsPerTurn, pa_host_threads(N * N, 1u << 16, n_threads), [&](uint32_t i) {
      double s = kSumStart;
      for (uint64_t j = 0; j < N; ++j) s = s + pcoa::squared(h_D[i * N + j]);
      r[i] = s / count;
    });
    double g = kSumStart;
    for (uint32_t i = 0; i < n; ++i) g = g + r[i];
    g = g / count;
    pa_for_each(0, n, kRowsPerTurn, pa_host_threads(N * N, 1u << 16, n_threads), [&](uint32_t i) {
      double s = kSumStart;
      for (uint64_t j = 0; j < N; ++j) {
        const double b = pcoa::centred(pcoa::squared(h_D[i * N + j]), r[i], r[j], g);
        h_B[i * N + j] = b;
        s = s + b * b;
      }
      row_sq[i] = s;
    });
    double trace = kSumStart, fro2 = kSumStart;
    for (uint64_t i = 0; i < N; ++i) {
      trace = trace + h_B[i * N + i];
      fro2 = fro2 + row_sq[i];
    }
    *h_trace = trace;
    *h_fro2 = fro2;
    return PA_OK;
  });
}

extern "C" int pa_symm_top_eigs_host(const double *h_B, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2, double *h_values,
                                     double *h_vectors, double *h_residuals, double *h_info, uint32_t n_threads) {
  if (!h_B) { pa_set_error("pa_symm_top_eigs_host: null matrix"); return PA_E_INVALID; }
  return pcoa::top_eigs("pa_symm_top_eigs_host", n, k, tol, max_iter, fro2,
                        [&](const double *h_Q, uint32_t p, double *h_Y) { return pa_mul_tall_f64_host(h_B, n, h_Q, p, h_Y, n_threads); },
                        h_values, h_vectors, h_residuals, h_info);
}
