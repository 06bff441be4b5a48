// The host twins of plot-run's distributions (select, moments, Gaussian kernel density, wide uniform-bin histogram) on
// random inputs in exact-size heap buffers, under AddressSanitizer / UBSan (host build only).  The select is checked
// against a sort, the histogram against a search of the edges, the density against a second statement of its sum.
//   usage: dist_host [trials]
#include <cstdarg>
#include <cstdio>
void pa_set_error(const char *fmt, ...) {}
#include "../../../pyani_plus_amd/csrc/dist_host.cpp"
#include "../../../pyani_plus_amd/csrc/hist_host.cpp"
#include <random>
int main(int argc, char **argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> unit(0.0, 1.0);
  const double nan = std::nan("");
  size_t checked = 0;
  for (int t = 0; t < trials; ++t) {
    const uint64_t n = rng() % 400;
    double *v = new double[n ? n : 1];
    std::vector<double> valid;
    for (uint64_t i = 0; i < n; ++i) {
      v[i] = rng() % 5 ? (rng() % 3 ? unit(rng) * 4 - 2 : (double)(rng() % 4) * 0.25) : nan;
      if (v[i] == v[i]) valid.push_back(v[i]);
    }
    std::sort(valid.begin(), valid.end());
    // ---- select: up to 8 ranks, one of them sometimes out of range
    const uint32_t n_ranks = (uint32_t)(rng() % 9);
    uint64_t *ranks = new uint64_t[n_ranks ? n_ranks : 1];
    double *picked = new double[n_ranks ? n_ranks : 1];
    bool in_range = true;
    for (uint32_t r = 0; r < n_ranks; ++r) {
      ranks[r] = rng() % (valid.size() + 1 + (rng() % 16 == 0));
      in_range = in_range && ranks[r] < valid.size();
    }
    const int status = pa_select_f64_host(v, n, ranks, n_ranks, picked);
    if ((status == PA_OK) != in_range) { printf("MISMATCH select status at trial %d\n", t); return 1; }
    for (uint32_t r = 0; status == PA_OK && r < n_ranks; ++r, ++checked)
      if (picked[r] != valid[ranks[r]]) { printf("MISMATCH select at trial %d\n", t); return 1; }
    // ---- moments and density
    double mom[2] = {nan, nan};
    if (pa_moments_f64_host(v, n, mom) != PA_OK) return 1;
    if (valid.empty() != (mom[0] != mom[0])) { printf("MISMATCH moments at trial %d\n", t); return 1; }
    const uint32_t n_grid = 1 + (uint32_t)(rng() % 40);
    double *grid = new double[n_grid], *density = new double[n_grid];
    for (uint32_t j = 0; j < n_grid; ++j) grid[j] = -2.5 + 5.0 * j / n_grid;
    const double bw = 0.01 + unit(rng);
    const int kde = pa_kde_gauss_f64_host(v, n, grid, n_grid, bw, density);
    if ((kde == PA_OK) != !valid.empty()) { printf("MISMATCH density status at trial %d\n", t); return 1; }
    for (uint32_t j = 0; kde == PA_OK && j < n_grid; ++j, ++checked) {
      double sum = 0.0;
      for (double x : valid) sum += exp(-0.5 * ((grid[j] - x) / bw) * ((grid[j] - x) / bw));
      sum /= (double)valid.size() * bw * sqrt(2.0 * M_PI);
      if (!(fabs(density[j] - sum) <= 1e-12 * sum + 1e-300)) { printf("MISMATCH density at trial %d\n", t); return 1; }
    }
    // ---- wide histogram: the counts buffer has exactly `bins` elements
    const uint32_t bins = 1 + (uint32_t)(rng() % (t % 50 == 0 ? 70000 : 3000));
    double *edges = new double[bins + 1];
    uint64_t *counts = new uint64_t[bins], *want = new uint64_t[bins]();
    const double lo = -1.5, hi = 1.75;
    for (uint32_t b = 0; b <= bins; ++b) edges[b] = b == bins ? hi : lo + (hi - lo) * b / bins;
    if (pa_hist_uniform_f64_wide_host(v, n, edges, bins, counts) != PA_OK) { printf("histogram failed at trial %d\n", t); return 1; }
    for (double x : valid) {
      if (x < lo || x > hi) continue;
      uint32_t b = (uint32_t)(std::upper_bound(edges, edges + bins + 1, x) - edges);  // the first edge above x
      ++want[b > bins ? bins - 1 : b - 1];
    }
    for (uint32_t b = 0; b < bins; ++b, ++checked)
      if (counts[b] != want[b]) { printf("MISMATCH histogram at trial %d, bin %u of %u\n", t, b, bins); return 1; }
    delete[] v; delete[] ranks; delete[] picked; delete[] grid; delete[] density; delete[] edges; delete[] counts; delete[] want;
  }
  // the argument checks
  double two[2] = {1.0, 1.0}, out[1];
  uint64_t one_count[1], nine[9] = {0};
  if (pa_select_f64_host(two, 2, nine, 9, out) != PA_E_INVALID || pa_hist_uniform_f64_wide_host(two, 2, two, 1, one_count) != PA_E_INVALID ||
      pa_hist_uniform_f64_wide_host(two, 2, two, 0, one_count) != PA_E_INVALID || pa_kde_gauss_f64_host(two, 2, two, 1, 0.0, out) != PA_E_INVALID) {
    printf("MISMATCH argument checks\n");
    return 1;
  }
  printf("%d trials, %zu values checked\n", trials, checked);
  return 0;
}
