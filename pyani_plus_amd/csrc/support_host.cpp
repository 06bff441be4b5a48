// support_host.cpp -- bootstrap-run: how many replicate trees have each edge of the reference tree (pa_tree_support).
// include/pyani_hip.h and DESIGN.md section 7l have the contract; tests/bootstrap_cases.py restates it with sets.
//
// Day's algorithm (W. H. E. Day 1985), exact and O(n) per tree.  A join table is an unrooted tree: node n + t is joined
// to its two children, and the two nodes no join takes are joined by the last edge.  Every tree is walked from leaf 0.
// The walk of the reference tree numbers the other leaves in the order it meets them, so that the leaves below any of
// its nodes are an interval [lo, hi] of those numbers; a node below which there are 2 to n - 2 leaves is a clade, and it
// is kept in row lo of a table when it is the last child of its parent and in row hi otherwise, which gives no row two
// clades.  Below a node of a replicate tree the numbers have a minimum, a maximum and a count: the leaves are an
// interval iff max - min + 1 == count, and the clade is the reference's iff row min or row max holds that interval.
// Sets are compared through exact integers: nothing is hashed.
#include <cstdint>
#include <vector>

#include "pa_host.h"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// A join table walked from leaf 0: nodes in pre-order, each node's parent on the way back to leaf 0
struct Walk {
  std::vector<uint32_t> adj;     // three neighbours per node (a leaf has one)
  std::vector<uint32_t> parent;  // towards leaf 0; kNone for leaf 0
  std::vector<uint32_t> order;   // pre-order from leaf 0
  std::vector<uint32_t> stack;
};

// false where the table is no tree over n leaves: a child out of range or taken twice
bool walk_from_leaf0(uint32_t n, const uint32_t *child, Walk &w, uint32_t *bad_join) {
  const uint32_t nodes = 2 * n - 2;
  w.adj.assign((size_t)nodes * 3, kNone);
  auto link = [&](uint32_t a, uint32_t b) {
    for (uint32_t *slot = &w.adj[(size_t)a * 3], *end = slot + 3; slot < end; ++slot)
      if (*slot == kNone) { *slot = b; return true; }
    return false;
  };
  std::vector<uint32_t> &taken = w.parent;  // borrowed: the join that takes a node
  taken.assign(nodes, kNone);
  for (uint32_t t = 0; t + 2 < n; ++t)
    for (int k = 0; k < 2; ++k) {
      const uint32_t v = child[2 * t + k];
      if (v >= n + t || taken[v] != kNone) { *bad_join = t; return false; }
      taken[v] = t;
      link(v, n + t);
      link(n + t, v);
    }
  // the last edge: the two nodes that no join takes, the last node made among them
  uint32_t a = kNone;
  for (uint32_t v = 0; v + 1 < nodes; ++v)
    if (taken[v] == kNone) a = v;
  link(a, nodes - 1);
  link(nodes - 1, a);
  w.parent.assign(nodes, kNone);
  w.order.clear();
  w.stack.assign(1, 0u);
  std::vector<uint32_t> &parent = w.parent;
  while (!w.stack.empty()) {
    const uint32_t v = w.stack.back();
    w.stack.pop_back();
    w.order.push_back(v);
    for (int k = 2; k >= 0; --k) {  // pushed last to first: met first to last
      const uint32_t u = w.adj[(size_t)v * 3 + k];
      if (u != kNone && u != parent[v]) { parent[u] = v; w.stack.push_back(u); }
    }
  }
  return true;
}

struct Below {
  uint32_t lo, hi, count;
};

// per node: the smallest and largest number and the count of the leaves below it (leaf 0 has no number and counts nothing)
void fold(uint32_t n, const Walk &w, const std::vector<uint32_t> &number, std::vector<Below> &below) {
  below.assign(w.parent.size(), Below{kNone, 0u, 0u});
  for (size_t at = w.order.size(); at-- > 1;) {
    const uint32_t v = w.order[at];
    if (v < n) below[v] = Below{number[v], number[v], 1u};
    Below &up = below[w.parent[v]];
    const Below &b = below[v];
    up.lo = b.lo < up.lo ? b.lo : up.lo;
    up.hi = b.hi > up.hi ? b.hi : up.hi;
    up.count += b.count;
  }
}

int tree_support(uint32_t n, const uint32_t *ref_child, uint32_t n_reps, const uint32_t *rep_child, uint32_t *support) {
  const uint32_t nodes = 2 * n - 2, joins = n - 2;
  Walk ref;
  uint32_t bad = 0;
  if (!walk_from_leaf0(n, ref_child, ref, &bad)) {
    pa_set_error("pa_tree_support: join %u of the reference tree takes a node that is not there or is taken already", bad);
    return PA_E_INVALID;
  }
  // the reference's leaf numbers and its table of clades
  std::vector<uint32_t> number(n, kNone);
  uint32_t next = 0;
  for (const uint32_t v : ref.order)
    if (v < n && v != 0) number[v] = next++;
  std::vector<Below> below;
  fold(n, ref, number, below);
  struct Row {
    uint32_t lo, hi, node;
  };
  std::vector<Row> table(n, Row{kNone, kNone, kNone});
  auto is_clade = [n](const Below &b) { return b.count >= 2 && b.count + 2 <= n; };
  for (const uint32_t v : ref.order) {
    if (v < n || !is_clade(below[v])) continue;
    const bool last_child = below[ref.parent[v]].hi == below[v].hi;
    Row &row = table[last_child ? below[v].lo : below[v].hi];
    row = Row{below[v].lo, below[v].hi, v};
  }
  std::vector<uint32_t> found(nodes, 0);  // per reference node that is a clade: the replicates that have it
  // the replicates: independent of one another, so host-pool threads take them in turn and count into their own arrays
  const uint32_t nt = pa_host_threads((uint64_t)n_reps * n, 1u << 14, 0);
  std::vector<std::vector<uint32_t>> counts(nt, std::vector<uint32_t>(nodes, 0));
  std::vector<uint64_t> bad_rep(nt, ~0ull), bad_at(nt, 0);
  HostPool::get().run(nt, [&](uint32_t id, uint32_t n_workers) {
    Walk w;
    std::vector<Below> b;
    for (uint64_t r = id; r < n_reps; r += n_workers) {
      uint32_t bad_join = 0;
      if (!walk_from_leaf0(n, rep_child + r * 2 * joins, w, &bad_join)) {
        if (bad_rep[id] == ~0ull) { bad_rep[id] = r; bad_at[id] = bad_join; }
        continue;
      }
      fold(n, w, number, b);
      for (const uint32_t v : w.order) {
        if (v < n || !is_clade(b[v]) || b[v].hi - b[v].lo + 1 != b[v].count) continue;
        for (const uint32_t at : {b[v].lo, b[v].hi}) {
          const Row &row = table[at];
          if (row.lo == b[v].lo && row.hi == b[v].hi) { ++counts[id][row.node]; break; }
        }
      }
    }
  });
  uint64_t first_bad = ~0ull, first_at = 0;
  for (uint32_t id = 0; id < nt; ++id)
    if (bad_rep[id] < first_bad) { first_bad = bad_rep[id]; first_at = bad_at[id]; }
  if (first_bad != ~0ull) {
    pa_set_error("pa_tree_support: join %llu of replicate %llu takes a node that is not there or is taken already", (unsigned long long)first_at,
                 (unsigned long long)first_bad);
    return PA_E_INVALID;
  }
  for (const auto &part : counts)
    for (uint32_t v = 0; v < nodes; ++v) found[v] += part[v];
  // node n + t stands for the edge above it in the join table: to the node that takes it, or the last edge for the last
  // node made.  Seen from leaf 0, the lower end of that edge has the edge's clade below it.
  std::vector<uint32_t> above(nodes, kNone);
  for (uint32_t t = 0; t < joins; ++t) above[ref_child[2 * t]] = above[ref_child[2 * t + 1]] = n + t;
  for (uint32_t v = 0; v + 1 < nodes; ++v)
    if (above[v] == kNone) { above[nodes - 1] = v; above[v] = nodes - 1; break; }  // the last edge, from either end
  for (uint32_t t = 0; t < joins; ++t) {
    const uint32_t v = n + t, up = above[v];
    const uint32_t lower = ref.parent[v] == up ? v : up;
    support[t] = is_clade(below[lower]) ? found[lower] : n_reps;  // a trivial split is in every tree
  }
  return PA_OK;
}

}  // namespace

extern "C" int pa_tree_support(uint32_t n, const uint32_t *h_ref_child, uint32_t n_reps, const uint32_t *h_rep_child, uint32_t *h_support) {
  if (!h_ref_child || !h_support || (n_reps && !h_rep_child)) { pa_set_error("pa_tree_support: null argument"); return PA_E_INVALID; }
  if (n < 4 || n > 65535) { pa_set_error("pa_tree_support: %u leaves; 4 to 65535 (fewer have no internal edge)", n); return PA_E_INVALID; }
  return pa_host_guard("pa_tree_support", [&] { return tree_support(n, h_ref_child, n_reps, h_rep_child, h_support); });
}
