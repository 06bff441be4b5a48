// linkage_host.cpp -- host side of plot-run's clustering: the row distances on the CPU (what a machine without a GPU
// uses and what rowdist.hip is compared with) and the average-linkage clustering of a condensed distance vector with
// the dendrogram's leaf order.
//
// Together they restate what seaborn's clustermap computes with its defaults (pyani_plus/plot_run.py:114-147):
// scipy.cluster.hierarchy.linkage(rows, method="average", metric="euclidean") and the `leaves` of
// dendrogram(..., no_plot=True), bit for bit, ties included.  DESIGN.md section 7c has the contract.
//
// The distances: one accumulator per pair, columns in ascending order, s = s + (a - b) * (a - b) with the square
// rounded before the addition, then the correctly rounded sqrt.  A compiler that is allowed to use FMA instructions
// (-march=native, or a target that always has them) contracts s + d * d by default and changes the last bit:
// strict_fp.h and -ffp-contract=off from the Makefile forbid it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

#include "pa_host.h"

#include "pairs_f64_host.h"

namespace {

inline uint64_t condensed_index(uint64_t n, uint64_t i, uint64_t j) {
  if (i > j) std::swap(i, j);
  return n * i - i * (i + 1) / 2 + (j - i - 1);
}

}  // namespace

extern "C" {

int pa_rowdist_euclid_host(const double *h_x, uint32_t n, uint32_t m, double *h_out, uint32_t n_threads) {
  if (n > (1u << 16)) { pa_set_error("pa_rowdist_euclid_host: %u rows; at most 65536", n); return PA_E_INVALID; }
  if (n < 2) return PA_OK;
  if (!h_out || (m && !h_x)) { pa_set_error("pa_rowdist_euclid_host: null argument"); return PA_E_INVALID; }
  return pa_host_guard("pa_rowdist_euclid_host", [&]() -> int {
    const uint64_t steps = (uint64_t)n * (n - 1) / 2 * std::max<uint32_t>(m, 1);
    const uint32_t nt = pa_host_threads(steps, 1u << 20, n_threads);
    // rows are handed out one at a time (row i has n - 1 - i pairs, the last row none; n >= 2 here)
    pa_for_each(0, n - 1, 1, nt, [&](uint32_t i) {
      double *out = h_out + condensed_index(n, i, i + 1);
      pairs_f64::pair_row_accumulate<pairs_f64::EuclidTerm>(h_x + (uint64_t)i * m, h_x + (uint64_t)(i + 1) * m, n - 1 - i, m,
                                                            [out](uint32_t u, double s) { out[u] = std::sqrt(s); });
    });
    return PA_OK;
  });
}

int pa_linkage_average(uint32_t n, const double *h_condensed, double *h_Z, uint32_t *h_leaves) {
  if (n == 0) return PA_OK;
  if (!h_leaves) { pa_set_error("pa_linkage_average: null argument"); return PA_E_INVALID; }
  if (n == 1) { h_leaves[0] = 0; return PA_OK; }  // scipy raises on one observation; a one-genome run still plots
  if (n > (1u << 16)) { pa_set_error("pa_linkage_average: %u observations; at most 65536", n); return PA_E_INVALID; }
  if (!h_condensed || !h_Z) { pa_set_error("pa_linkage_average: null argument"); return PA_E_INVALID; }
  // a NaN or infinite distance never wins the strict < of the search below, which would leave a chain without a neighbour
  for (uint64_t k = 0, count = (uint64_t)n * (n - 1) / 2; k < count; ++k)
    if (!std::isfinite(h_condensed[k])) {
      pa_set_error("pa_linkage_average: distance %llu of %llu is not finite", (unsigned long long)k, (unsigned long long)count);
      return PA_E_INVALID;
    }
  return pa_host_guard("pa_linkage_average", [&]() -> int {
    const uint64_t N = n;
    std::vector<double> D(h_condensed, h_condensed + N * (N - 1) / 2);  // the merges overwrite it: work on a copy
    std::vector<uint32_t> size(n, 1u), chain(n);
    struct Merge { uint32_t x, y; double dist; };
    std::vector<Merge> merges(n - 1);
    uint32_t chain_len = 0;
    // nearest-neighbour chain (scipy/cluster/_hierarchy.pyx nn_chain): follow nearest neighbours until two clusters are
    // each other's nearest, merge them, go on from what is left of the chain
    for (uint32_t k = 0; k + 1 < n; ++k) {
      if (chain_len == 0) {
        uint32_t i = 0;
        while (size[i] == 0) ++i;  // the lowest live index
        chain[0] = i;
        chain_len = 1;
      }
      uint32_t x = 0, y = 0;
      double current_min = 0.0;
      for (;;) {
        x = chain[chain_len - 1];
        // the previous element of the chain is preferred among equals: the search starts from its distance and only a
        // strictly smaller one replaces it
        if (chain_len > 1) {
          y = chain[chain_len - 2];
          current_min = D[condensed_index(N, x, y)];
        } else {
          current_min = std::numeric_limits<double>::infinity();
        }
        // D[idx(x, i)]: for i < x the stride between consecutive i shrinks by one each step, for i > x it is 1
        for (uint32_t i = 0; i < x; ++i) {
          if (size[i] == 0) continue;
          const double dist = D[N * i - (uint64_t)i * (i + 1) / 2 + (x - i - 1)];
          if (dist < current_min) { current_min = dist; y = i; }
        }
        const double *row = D.data() + (N * x - (uint64_t)x * (x + 1) / 2);  // row[i - x - 1] = D[idx(x, i)], i > x
        for (uint32_t i = x + 1; i < n; ++i) {
          if (size[i] == 0) continue;
          const double dist = row[i - x - 1];
          if (dist < current_min) { current_min = dist; y = i; }
        }
        if (chain_len == 1 && std::isinf(current_min)) {  // finite inputs, but an average of distances near 1e308 overflowed
          pa_set_error("pa_linkage_average: a merged distance is not finite");
          return PA_E_INVALID;
        }
        if (chain_len > 1 && y == chain[chain_len - 2]) break;
        chain[chain_len++] = y;
      }
      chain_len -= 2;
      if (x > y) std::swap(x, y);
      const uint32_t nx = size[x], ny = size[y];
      merges[k] = {x, y, current_min};
      size[x] = 0;        // x is dropped
      size[y] = nx + ny;  // y becomes the union
      const double fx = (double)nx, fy = (double)ny, fsum = (double)(nx + ny);
      for (uint32_t i = 0; i < n; ++i) {
        if (size[i] == 0 || i == y) continue;
        const uint64_t iy = condensed_index(N, i, y);
        D[iy] = (fx * D[condensed_index(N, i, x)] + fy * D[iy]) / fsum;
      }
    }
    // numpy.argsort(kind="mergesort"): stable
    std::vector<uint32_t> order(n - 1);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&merges](uint32_t a, uint32_t b) { return merges[a].dist < merges[b].dist; });
    // label(): merge r, in sorted order, is cluster n + r; its two sides are named by their current roots, smaller first
    std::vector<uint32_t> parent(2 * (size_t)n - 1), members(2 * (size_t)n - 1, 1u);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&parent](uint32_t v) {
      uint32_t root = v;
      while (parent[root] != root) root = parent[root];
      while (parent[v] != root) { const uint32_t up = parent[v]; parent[v] = root; v = up; }
      return root;
    };
    std::vector<uint32_t> left(n - 1), right(n - 1);
    for (uint32_t r = 0; r + 1 < n; ++r) {
      const Merge &mg = merges[order[r]];
      uint32_t a = find(mg.x), b = find(mg.y);
      if (a > b) std::swap(a, b);
      const uint32_t id = n + r;
      parent[a] = id;
      parent[b] = id;
      members[id] = members[a] + members[b];
      left[r] = a;
      right[r] = b;
      h_Z[4 * (size_t)r + 0] = (double)a;
      h_Z[4 * (size_t)r + 1] = (double)b;
      h_Z[4 * (size_t)r + 2] = mg.dist;
      h_Z[4 * (size_t)r + 3] = (double)members[id];
    }
    // dendrogram(no_plot=True)["leaves"]: pre-order from the last merge, first child before the second
    std::vector<uint32_t> stack;
    stack.push_back(2 * n - 2);
    uint32_t at = 0;
    while (!stack.empty()) {
      const uint32_t v = stack.back();
      stack.pop_back();
      if (v < n) { h_leaves[at++] = v; continue; }
      stack.push_back(right[v - n]);
      stack.push_back(left[v - n]);
    }
    return PA_OK;
  });
}

}  // extern "C"
