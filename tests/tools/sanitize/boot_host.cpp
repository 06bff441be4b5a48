// The host side of bootstrap-run (pa_tree_support, pa_msa_boot_counts_host, pa_msa_boot_distances_host) on random
// inputs in exact-size heap buffers, under AddressSanitizer / UBSan (host build only).  The support is checked against
// the clades as 64-bit leaf sets, the counts against the plain double loop.
//   usage: boot_host [trials]
#include <cstdarg>
#include <cstdio>
void pa_set_error(const char *fmt, ...) {}
#include "../../../pyani_plus_amd/csrc/msa_boot_host.cpp"
#include "../../../pyani_plus_amd/csrc/support_host.cpp"
#include <random>
#include <set>

// a random join table over n leaves: any two live nodes are joined, n - 2 times
static void random_table(std::mt19937_64 &rng, uint32_t n, uint32_t *child) {
  std::vector<uint32_t> live(n);
  for (uint32_t i = 0; i < n; ++i) live[i] = i;
  for (uint32_t t = 0; t + 2 < n; ++t) {
    const size_t a = rng() % live.size();
    uint32_t x = live[a];
    live.erase(live.begin() + a);
    const size_t b = rng() % live.size();
    uint32_t y = live[b];
    live.erase(live.begin() + b);
    child[2 * t] = x < y ? x : y;
    child[2 * t + 1] = x < y ? y : x;
    live.push_back(n + t);
  }
}
// per join, the leaves on the side of the edge above node n + t that is away from leaf 0
static std::vector<uint64_t> clades(uint32_t n, const uint32_t *child) {
  std::vector<uint64_t> below(2 * n - 2), out(n - 2);
  const uint64_t all = n == 64 ? ~0ull : (1ull << n) - 1;
  for (uint32_t i = 0; i < n; ++i) below[i] = 1ull << i;
  for (uint32_t t = 0; t + 2 < n; ++t) {
    below[n + t] = below[child[2 * t]] | below[child[2 * t + 1]];
    out[t] = below[n + t] & 1 ? all & ~below[n + t] : below[n + t];
  }
  return out;
}
static bool trivial(uint64_t clade, uint32_t n) {
  const int k = __builtin_popcountll(clade);
  return k < 2 || k + 2 > (int)n;
}

int main(int argc, char **argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 300;
  std::mt19937_64 rng(11);
  size_t trees = 0, cells = 0;
  for (int trial = 0; trial < trials; ++trial) {
    // ---- support
    const uint32_t n = 4 + (uint32_t)(rng() % 61), reps = (uint32_t)(rng() % 9);
    uint32_t *ref = new uint32_t[2 * (n - 2)], *rep = new uint32_t[(size_t)reps * 2 * (n - 2) ? (size_t)reps * 2 * (n - 2) : 1], *got = new uint32_t[n - 2];
    random_table(rng, n, ref);
    for (uint32_t r = 0; r < reps; ++r) {
      if (rng() % 3 == 0) memcpy(rep + (size_t)r * 2 * (n - 2), ref, sizeof(uint32_t) * 2 * (n - 2));  // some replicates are the reference
      else random_table(rng, n, rep + (size_t)r * 2 * (n - 2));
    }
    if (pa_tree_support(n, ref, reps, rep, got) != PA_OK) { printf("support failed at trial %d\n", trial); return 1; }
    const std::vector<uint64_t> want = clades(n, ref);
    for (uint32_t t = 0; t + 2 < n; ++t) {
      uint32_t count = 0;
      for (uint32_t r = 0; r < reps; ++r) {
        const std::vector<uint64_t> have = clades(n, rep + (size_t)r * 2 * (n - 2));
        count += std::set<uint64_t>(have.begin(), have.end()).count(want[t]) ? 1 : 0;
      }
      if (trivial(want[t], n)) count = reps;
      if (got[t] != count) { printf("SUPPORT MISMATCH at trial %d, join %u: %u, expected %u\n", trial, t, got[t], count); return 1; }
    }
    trees += reps + 1;
    delete[] ref; delete[] rep; delete[] got;
    // ---- counts and distances
    const uint32_t rows = (uint32_t)(rng() % 7), n_reps = (uint32_t)(rng() % 4);
    const uint64_t cols = rng() % 200, stride = cols + rng() % 3;
    uint8_t *text = new uint8_t[(size_t)rows * stride ? (size_t)rows * stride : 1], *w = new uint8_t[(size_t)n_reps * cols ? (size_t)n_reps * cols : 1];
    for (size_t i = 0; i < (size_t)rows * stride; ++i) text[i] = "ACGT-"[rng() % 5];
    for (uint32_t r = 0; r < n_reps; ++r) {
      memset(w + (size_t)r * cols, 0, cols);
      for (uint64_t t = 0; t < cols; ++t) {
        uint64_t c = rng() % cols;
        while (w[(size_t)r * cols + c] == 255) c = (c + 1) % cols;
        ++w[(size_t)r * cols + c];
      }
    }
    const size_t nn = (size_t)rows * rows, total = nn * n_reps;
    uint32_t *m = new uint32_t[total ? total : 1], *b = new uint32_t[total ? total : 1];
    double *d = new double[total ? total : 1];
    if (pa_msa_boot_counts_host(text, stride, rows, cols, w, n_reps, m, b, 1 + (uint32_t)(rng() % 4)) != PA_OK) { printf("counts failed at trial %d\n", trial); return 1; }
    if (pa_msa_boot_distances_host(m, b, rows, n_reps, 0.5, d, 1 + (uint32_t)(rng() % 4)) != PA_OK) { printf("distances failed at trial %d\n", trial); return 1; }
    for (uint32_t r = 0; r < n_reps; ++r)
      for (uint32_t i = 0; i < rows; ++i)
        for (uint32_t j = 0; j < rows; ++j) {
          uint32_t wm = 0, wb = 0;
          for (uint64_t c = 0; c < cols; ++c) {
            const uint8_t q = text[i * stride + c], s = text[j * stride + c];
            wm += q == s && q != '-' ? w[(size_t)r * cols + c] : 0;
            wb += q != '-' && s != '-' ? w[(size_t)r * cols + c] : 0;
          }
          const size_t at = r * nn + (size_t)i * rows + j;
          if (m[at] != wm || b[at] != wb) { printf("COUNT MISMATCH at trial %d\n", trial); return 1; }
          if (!(d[at] >= 0.0 && d[at] <= 1.0) || (i == j && d[at] != 0.0)) { printf("DISTANCE OUT OF RANGE at trial %d\n", trial); return 1; }
          ++cells;
        }
    delete[] text; delete[] w; delete[] m; delete[] b; delete[] d;
  }
  printf("%zu trees and %zu cells checked\n", trees, cells);
  return 0;
}
