// The host twin of plot-run's scatter figures (the 2-D binning) on random points in exact-size heap buffers, under
// AddressSanitizer / UBSan (host build only).  Counts and last indices are checked against a search of the edges.
//   usage: scatter_host [trials]
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
void pa_set_error(const char *fmt, ...) {}
#include "../../../pyani_plus_amd/csrc/scatter_host.cpp"
#include "../../../pyani_plus_amd/csrc/hist_host.cpp"
#include <random>
static uint32_t search(const double *e, uint32_t bins, double v) {  // the last edge <= v, the last bin for the last edge
  uint32_t b = 0;
  while (b + 1 < bins && e[b + 1] <= v) ++b;
  return b;
}
int main(int argc, char **argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> unit(0.0, 1.0);
  const double nan = std::nan("");
  size_t points = 0;
  for (int t = 0; t < trials; ++t) {
    const uint32_t bx = t % 50 == 0 ? 1024 : 1 + (uint32_t)(rng() % 70), by = t % 50 == 1 ? 1024 : 1 + (uint32_t)(rng() % 70);
    const uint64_t n = rng() % 400, cells = (uint64_t)bx * by;
    double *xe = new double[bx + 1], *ye = new double[by + 1];
    const double x0 = unit(rng) - 0.5, xs = 0.1 + unit(rng), y0 = unit(rng) - 0.5, ys = 0.1 + unit(rng);
    for (uint32_t b = 0; b <= bx; ++b) xe[b] = b == bx ? x0 + xs : x0 + xs * ((double)b / bx);
    for (uint32_t b = 0; b <= by; ++b) ye[b] = b == by ? y0 + ys : y0 + ys * ((double)b / by);
    double *x = new double[n ? n : 1], *y = new double[n ? n : 1];
    for (uint64_t i = 0; i < n; ++i) {  // inside, outside, on an edge, NaN
      const unsigned kx = rng() % 8, ky = rng() % 8;
      x[i] = kx == 0 ? nan : kx == 1 ? xe[rng() % (bx + 1)] : x0 - 0.1 * xs + 1.2 * xs * unit(rng);
      y[i] = ky == 0 ? nan : ky == 1 ? ye[rng() % (by + 1)] : y0 - 0.1 * ys + 1.2 * ys * unit(rng);
    }
    uint64_t *counts = new uint64_t[cells], *last = new uint64_t[cells], *want_c = new uint64_t[cells](), *want_l = new uint64_t[cells];
    for (uint64_t c = 0; c < cells; ++c) want_l[c] = PA_BIN2D_NONE;
    if (pa_bin2d_f64_host(x, y, n, xe, bx, ye, by, counts, last) != PA_OK) { printf("bin2d failed at trial %d\n", t); return 1; }
    for (uint64_t i = 0; i < n; ++i) {
      if (!(x[i] >= xe[0] && x[i] <= xe[bx] && y[i] >= ye[0] && y[i] <= ye[by])) continue;
      const uint64_t c = (uint64_t)search(xe, bx, x[i]) * by + search(ye, by, y[i]);
      ++want_c[c];
      want_l[c] = i;
    }
    for (uint64_t c = 0; c < cells; ++c)
      if (counts[c] != want_c[c] || last[c] != want_l[c]) { printf("BIN2D MISMATCH at trial %d cell %llu\n", t, (unsigned long long)c); return 1; }
    // refused before anything is read: too many points for arrays of one, bins out of range
    if (pa_bin2d_f64_host(x, y, 0xFFFFFFFFULL, xe, bx, ye, by, counts, last) != PA_E_INVALID) { printf("n = 2^32 - 1 accepted\n"); return 1; }
    if (pa_bin2d_f64_host(x, y, n, xe, 0, ye, by, counts, last) != PA_E_INVALID || pa_bin2d_f64_host(x, y, n, xe, bx, ye, 1025, counts, last) != PA_E_INVALID) { printf("bins accepted\n"); return 1; }
    points += n;
    delete[] xe; delete[] ye; delete[] x; delete[] y; delete[] counts; delete[] last; delete[] want_c; delete[] want_l;
  }
  printf("%d trials, %zu points\n", trials, points);
  return 0;
}
