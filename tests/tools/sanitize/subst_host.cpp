// The host side of phylo-run (pa_subst_code, pa_subst_log_host, pa_msa_subst_counts_host, pa_subst_distances_host) on
// random inputs in exact-size heap buffers, under AddressSanitizer / UBSan (host build only).  The counts are checked
// against the plain loop over the pairs and the columns, the undefined pairs against a count of the `missing` cells.
//   usage: subst_host [trials]
#include <cstdarg>
#include <cstdio>
void pa_set_error(const char *fmt, ...) {}
#include "../../../pyani_plus_amd/csrc/msa_boot_host.cpp"
#include "../../../pyani_plus_amd/csrc/subst_host.cpp"
#include <cmath>
#include <random>

int main(int argc, char **argv) {
  const int trials = argc > 1 ? atoi(argv[1]) : 300;
  std::mt19937_64 rng(12);
  uint8_t code[256];
  if (pa_subst_code(code) != PA_OK) return 1;
  size_t cells = 0;
  for (int trial = 0; trial < trials; ++trial) {
    const uint32_t rows = (uint32_t)(rng() % 7), n_reps = (uint32_t)(rng() % 4);
    const bool weighted = n_reps != 1 || rng() % 2;
    const uint64_t cols = rng() % 200, stride = cols + rng() % 3;
    uint8_t *text = new uint8_t[(size_t)rows * stride ? (size_t)rows * stride : 1], *w = new uint8_t[(size_t)n_reps * cols ? (size_t)n_reps * cols : 1];
    for (size_t i = 0; i < (size_t)rows * stride; ++i) text[i] = "ACGTacgtUuNRY-"[rng() % 14];
    for (uint32_t r = 0; r < n_reps; ++r) {
      memset(w + (size_t)r * cols, 0, cols);
      for (uint64_t t = 0; t < cols; ++t) {
        uint64_t c = rng() % cols;
        while (w[(size_t)r * cols + c] == 255) c = (c + 1) % cols;
        ++w[(size_t)r * cols + c];
      }
    }
    const size_t nn = (size_t)rows * rows, total = nn * n_reps;
    uint32_t *v = new uint32_t[total ? total : 1], *s = new uint32_t[total ? total : 1], *t = new uint32_t[total ? total : 1];
    double *d = new double[total ? total : 1];
    uint64_t *undefined = new uint64_t[2 * n_reps ? 2 * n_reps : 1];
    if (pa_msa_subst_counts_host(text, stride, rows, cols, weighted ? w : nullptr, n_reps, v, s, t, 1 + (uint32_t)(rng() % 4)) != PA_OK) { printf("counts failed at trial %d\n", trial); return 1; }
    for (uint32_t r = 0; r < n_reps; ++r)
      for (uint32_t i = 0; i < rows; ++i)
        for (uint32_t j = 0; j < rows; ++j) {
          uint32_t wv = 0, ws = 0, wt = 0;
          for (uint64_t c = 0; c < cols; ++c) {
            const uint8_t a = code[text[i * stride + c]], b = code[text[j * stride + c]];
            const uint32_t weight = weighted ? w[(size_t)r * cols + c] : 1;
            if (a < 4 || b < 4) continue;
            wv += weight;
            if ((a ^ b) & 2) wt += weight;
            else if (a != b) ws += weight;
          }
          const size_t at = r * nn + (size_t)i * rows + j;
          if (v[at] != wv || s[at] != ws || t[at] != wt) { printf("COUNT MISMATCH at trial %d\n", trial); return 1; }
          ++cells;
        }
    for (int model = PA_SUBST_MODEL_P; model <= PA_SUBST_MODEL_K80; ++model) {
      if (pa_subst_distances_host(v, s, t, rows, n_reps, model, 9.0, d, undefined, 1 + (uint32_t)(rng() % 4)) != PA_OK) { printf("distances failed at trial %d\n", trial); return 1; }
      for (uint32_t r = 0; r < n_reps; ++r) {
        uint64_t missing = 0;
        for (uint32_t i = 0; i < rows; ++i)
          for (uint32_t j = 0; j < rows; ++j) {
            const double x = d[r * nn + (size_t)i * rows + j];
            if (!(x >= 0.0) || !std::isfinite(x) || std::signbit(x) || (i == j && x != 0.0)) { printf("DISTANCE OUT OF RANGE at trial %d\n", trial); return 1; }
            missing += i < j && x == 9.0;
          }
        if (undefined[2 * r] + undefined[2 * r + 1] != missing) { printf("UNDEFINED MISMATCH at trial %d\n", trial); return 1; }
      }
    }
    delete[] text; delete[] w; delete[] v; delete[] s; delete[] t; delete[] d; delete[] undefined;
  }
  double x[6] = {1.0, 0.5, 1e-310, 0.0, -1.0, 3.0}, y[6];
  if (pa_subst_log_host(x, 6, y) != PA_OK || y[0] != 0.0 || std::fabs(y[1] - std::log(0.5)) > 1e-15 || std::fabs(y[2] - std::log(1e-310)) > 1e-12) { printf("LOGARITHM\n"); return 1; }
  printf("%zu cells checked\n", cells);
  return 0;
}
