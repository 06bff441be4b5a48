// classify_host.cpp -- host side of classify: the edge list on the CPU (what a machine without a GPU uses and what
// classify.hip is compared with), the score matrix of tANI mode, and the clique pass over the sorted edges.
//
// The reference removes the lowest edge of a networkx graph, recomputes the connected components, and recurses into
// them when there are several (pyani_plus/classify.py:135-189): about quadratic in the number of edges.  The same rows
// follow from one pass over the edges in removal order, walked backwards: adding edges from the highest score down,
// every component the recursion ever visits appears exactly once as a union-find component, at the moment just before
// the edge that joins it to another one -- the edge whose removal separates it in the reference, hence its min_score.
// It is a clique iff it holds n (n - 1) / 2 edges.  DESIGN.md section 7b has the argument and the tie rule.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <numeric>
#include <utility>
#include <vector>

#include "pa_host.h"

#include "pair_rule.h"

struct pa_cliques {
  std::vector<uint32_t> n_nodes;
  std::vector<double> max_cov, min_score, max_score;
  std::vector<uint8_t> present;
  std::vector<uint64_t> member_off;
  std::vector<uint32_t> members;
};

namespace {

using pair_rule::agg2;  // with a = M[j,i], b = M[i,j], i < j
using pair_rule::agg_ok;

// a node of the component tree: the leaves are the genomes, an inner node is the union of its two children
struct Node {
  uint32_t child[2] = {0, 0};  // inner nodes only
  uint32_t first = 0;          // smallest member
  uint32_t n = 1;
  uint64_t edges = 0;
  double min_cov = 0, min_sc = 0;  // over its edges, when edges > 0
  double formed_by = 0;            // min_score
  bool recorded = false, has_formed_by = false, listed = false;
};

}  // namespace

extern "C" {

int pa_classify_edges_host(const double *h_score, const double *h_cov, uint32_t n, int agg_score, int agg_cov, double cov_min,
                           uint64_t cap_edges, uint32_t *h_i, uint32_t *h_j, double *h_edge_score, double *h_edge_cov,
                           uint64_t *n_edges) {
  if (!n_edges || (n >= 2 && (!h_score || !h_cov))) { pa_set_error("pa_classify_edges_host: null argument"); return PA_E_INVALID; }
  if (!agg_ok(agg_score) || !agg_ok(agg_cov)) {
    pa_set_error("pa_classify_edges_host: aggregators %d, %d (PA_AGG_MIN, PA_AGG_MAX or PA_AGG_MEAN)", agg_score, agg_cov);
    return PA_E_INVALID;
  }
  if (n > (1u << 16)) { pa_set_error("pa_classify_edges_host: %u genomes; the edge list is indexed with 32 bits, at most 65536 genomes", n); return PA_E_INVALID; }
  if (cov_min != cov_min) { pa_set_error("pa_classify_edges_host: cov_min is NaN"); return PA_E_INVALID; }
  *n_edges = 0;
  try {
    std::vector<uint32_t> vi, vj;
    std::vector<double> vs, vc;
    // A strip of kStrip rows at a time: the column strip M[j, i0 .. i0 + kStrip) is transposed into t_*[r][j] first
    // (kStrip contiguous doubles per row j), so that the pair loop reads both directions along j.
    constexpr uint32_t kStrip = 64;
    std::vector<double> t_score((size_t)kStrip * n), t_cov((size_t)kStrip * n);
    for (uint32_t i0 = 0; i0 < n; i0 += kStrip) {
      const uint32_t rows = std::min(kStrip, n - i0);
      for (uint32_t j = i0 + 1; j < n; ++j)
        for (uint32_t r = 0; r < rows; ++r) {
          t_score[(size_t)r * n + j] = h_score[(uint64_t)j * n + i0 + r];
          t_cov[(size_t)r * n + j] = h_cov[(uint64_t)j * n + i0 + r];
        }
      for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t i = i0 + r;
        for (uint32_t j = i + 1; j < n; ++j) {
          const double c = agg2(agg_cov, t_cov[(size_t)r * n + j], h_cov[(uint64_t)i * n + j]);
          const double s = agg2(agg_score, t_score[(size_t)r * n + j], h_score[(uint64_t)i * n + j]);
          if (c == c && s == s && c > cov_min) { vi.push_back(i); vj.push_back(j); vs.push_back(s); vc.push_back(c); }
        }
      }
    }
    const uint64_t E = vi.size();
    *n_edges = E;
    if (E > cap_edges) {
      pa_set_error("pa_classify_edges_host: %llu edges, caller gave room for %llu", (unsigned long long)E, (unsigned long long)cap_edges);
      return PA_E_CAPACITY;
    }
    if (E == 0) return PA_OK;
    if (!h_i || !h_j || !h_edge_score || !h_edge_cov) { pa_set_error("pa_classify_edges_host: null output"); return PA_E_INVALID; }
    // the list is in (i, j) order and the sort is stable: equal scores (-0.0 == 0.0) stay in (i, j) order
    // (the score travels with the position: a sort of positions alone looks every score up at random)
    std::vector<std::pair<double, uint32_t>> order(E);
    for (uint64_t e = 0; e < E; ++e) order[e] = {vs[e], (uint32_t)e};
    std::stable_sort(order.begin(), order.end(),
                     [](const std::pair<double, uint32_t> &a, const std::pair<double, uint32_t> &b) { return a.first < b.first; });
    for (uint64_t p = 0; p < E; ++p) {
      const uint32_t e = order[p].second;
      h_i[p] = vi[e]; h_j[p] = vj[e]; h_edge_score[p] = vs[e]; h_edge_cov[p] = vc[e];
    }
  } catch (const std::bad_alloc &) {
    pa_set_error("pa_classify_edges_host: out of memory");
    return PA_E_NOMEM;
  }
  return PA_OK;
}

int pa_classify_tani_host(const double *h_hadamard, uint64_t n_cells, double *h_score) {
  if (n_cells && (!h_hadamard || !h_score)) { pa_set_error("pa_classify_tani_host: null argument"); return PA_E_INVALID; }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (uint64_t k = 0; k < n_cells; ++k) {
    const double h = h_hadamard[k];
    // map(lambda x: -log(x) if x else nan, na_action="ignore"), then tani * -1 where it is not NaN
    h_score[k] = (h != h || h == 0.0) ? nan : (-std::log(h)) * -1.0;
  }
  return PA_OK;
}

int pa_classify_cliques(uint32_t n, uint64_t n_edges, const uint32_t *h_i, const uint32_t *h_j, const double *h_edge_score,
                        const double *h_edge_cov, pa_cliques **out) {
  if (!out || (n_edges && (!h_i || !h_j || !h_edge_score || !h_edge_cov))) { pa_set_error("pa_classify_cliques: null argument"); return PA_E_INVALID; }
  *out = nullptr;
  for (uint64_t e = 0; e < n_edges; ++e) {
    if (h_i[e] >= n || h_j[e] >= n || h_i[e] == h_j[e]) {
      pa_set_error("pa_classify_cliques: edge %llu joins %u and %u of %u nodes", (unsigned long long)e, h_i[e], h_j[e], n);
      return PA_E_INVALID;
    }
    if (e && h_edge_score[e] < h_edge_score[e - 1]) {
      pa_set_error("pa_classify_cliques: edge %llu has a lower score than the edge before it", (unsigned long long)e);
      return PA_E_INVALID;
    }
  }
  try {
    std::unique_ptr<pa_cliques> cl(new pa_cliques);
    std::vector<Node> nodes;
    nodes.reserve(2 * (size_t)n);
    nodes.resize(n);
    for (uint32_t p = 0; p < n; ++p) nodes[p].first = p;
    std::vector<uint32_t> parent(n), node_of(n);  // union-find over the genomes; node_of[root] = its tree node
    std::iota(parent.begin(), parent.end(), 0u);
    std::iota(node_of.begin(), node_of.end(), 0u);
    auto find = [&parent](uint32_t x) {
      while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
      return x;
    };
    auto is_clique = [](const Node &nd) { return nd.edges == (uint64_t)nd.n * (nd.n - 1) / 2; };
    auto add_edge = [](Node &nd, double s, double c) {
      if (nd.edges == 0 || c < nd.min_cov) nd.min_cov = c;
      if (nd.edges == 0 || s < nd.min_sc) nd.min_sc = s;
      ++nd.edges;
    };
    for (uint64_t e = n_edges; e-- > 0;) {
      const double s = h_edge_score[e], c = h_edge_cov[e];
      uint32_t a = find(h_i[e]), b = find(h_j[e]);
      if (a != b) {
        const uint32_t na = node_of[a], nb = node_of[b];
        for (uint32_t k : {na, nb}) {
          nodes[k].recorded = is_clique(nodes[k]);
          nodes[k].formed_by = s;
          nodes[k].has_formed_by = true;
        }
        Node u;
        const bool a_first = nodes[na].first < nodes[nb].first;
        u.child[0] = a_first ? na : nb;
        u.child[1] = a_first ? nb : na;
        u.first = std::min(nodes[na].first, nodes[nb].first);
        u.n = nodes[na].n + nodes[nb].n;
        for (uint32_t k : {na, nb})
          if (nodes[k].edges) {
            if (u.edges == 0 || nodes[k].min_cov < u.min_cov) u.min_cov = nodes[k].min_cov;
            if (u.edges == 0 || nodes[k].min_sc < u.min_sc) u.min_sc = nodes[k].min_sc;
            u.edges += nodes[k].edges;
          }
        if (nodes[na].n < nodes[nb].n) std::swap(a, b);
        parent[b] = a;
        node_of[a] = (uint32_t)nodes.size();
        nodes.push_back(u);
      }
      add_edge(nodes[node_of[a]], s, c);
    }
    std::vector<uint32_t> roots;
    for (uint32_t p = 0; p < n; ++p)
      if (find(p) == p) roots.push_back(node_of[p]);
    std::sort(roots.begin(), roots.end(), [&nodes](uint32_t x, uint32_t y) { return nodes[x].first < nodes[y].first; });
    const bool several = roots.size() > 1;
    for (uint32_t r : roots) {
      nodes[r].recorded = is_clique(nodes[r]);
      nodes[r].has_formed_by = several && n_edges > 0;
      nodes[r].formed_by = n_edges ? h_edge_score[0] : 0.0;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<uint32_t> stack, walk;
    cl->member_off.push_back(0);
    auto emit = [&](uint32_t k) {
      Node &nd = nodes[k];
      if (!nd.recorded || nd.listed) return;
      nd.listed = true;
      const bool has_edges = nd.n > 1;  // a recorded node is a clique: edges > 0 iff n > 1
      cl->n_nodes.push_back(nd.n);
      cl->max_cov.push_back(has_edges ? nd.min_cov : nan);
      cl->min_score.push_back(nd.has_formed_by ? nd.formed_by : nan);
      cl->max_score.push_back(has_edges ? nd.min_sc : nan);
      cl->present.push_back((uint8_t)((has_edges ? 1 : 0) | (nd.has_formed_by ? 2 : 0) | (has_edges ? 4 : 0)));
      const size_t at = cl->members.size();
      walk.assign(1, k);
      while (!walk.empty()) {
        const uint32_t w = walk.back();
        walk.pop_back();
        if (w < n) cl->members.push_back(w);
        else { walk.push_back(nodes[w].child[1]); walk.push_back(nodes[w].child[0]); }
      }
      std::sort(cl->members.begin() + (std::ptrdiff_t)at, cl->members.end());
      cl->member_off.push_back(cl->members.size());
    };
    if (several)
      for (uint32_t r : roots) emit(r);
    for (auto it = roots.rbegin(); it != roots.rend(); ++it) stack.push_back(*it);
    while (!stack.empty()) {
      const uint32_t k = stack.back();
      stack.pop_back();
      emit(k);
      if (k >= n) { stack.push_back(nodes[k].child[1]); stack.push_back(nodes[k].child[0]); }
    }
    *out = cl.release();
  } catch (const std::bad_alloc &) {
    pa_set_error("pa_classify_cliques: out of memory");
    return PA_E_NOMEM;
  }
  return PA_OK;
}

int pa_cliques_info(const pa_cliques *cl, uint64_t *n_rows, uint64_t *n_members) {
  if (!cl) { pa_set_error("pa_cliques_info: null handle"); return PA_E_INVALID; }
  if (n_rows) *n_rows = cl->n_nodes.size();
  if (n_members) *n_members = cl->members.size();
  return PA_OK;
}

int pa_cliques_copy(const pa_cliques *cl, uint32_t *n_nodes, double *max_cov, double *min_score, double *max_score, uint8_t *present,
                    uint64_t *member_off, uint32_t *members) {
  if (!cl) { pa_set_error("pa_cliques_copy: null handle"); return PA_E_INVALID; }
  if (n_nodes) std::copy(cl->n_nodes.begin(), cl->n_nodes.end(), n_nodes);
  if (max_cov) std::copy(cl->max_cov.begin(), cl->max_cov.end(), max_cov);
  if (min_score) std::copy(cl->min_score.begin(), cl->min_score.end(), min_score);
  if (max_score) std::copy(cl->max_score.begin(), cl->max_score.end(), max_score);
  if (present) std::copy(cl->present.begin(), cl->present.end(), present);
  if (member_off) std::copy(cl->member_off.begin(), cl->member_off.end(), member_off);
  if (members) std::copy(cl->members.begin(), cl->members.end(), members);
  return PA_OK;
}

void pa_cliques_free(pa_cliques *cl) { delete cl; }

}  // extern "C"
