// Host program of tests/test_murmur_word_tables.py: every second product k_j that the k-mer hash kernel can form from its
// tables, through the formulas the kernel itself uses (pyani_plus_amd/csrc/murmur_words.h).
//   argv[1]: output file.  For every word j = 0..3 and every byte count n = 1..8 of that word (k = 8j + n), the 65 536
//   values k_j of the group pairs (lo + 256 * hi), as little-endian uint64: 4 x 8 x 65 536 values.
#include <cstdio>
#include <vector>

#include "murmur_words.h"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "wb");
  if (!f) return 3;
  std::vector<uint64_t> out(65536);
  for (int j = 0; j < 4; ++j) {
    for (int n = 1; n <= 8; ++n) {
      const int k = 8 * j + n;
      pa_dev::WordLoEntry lo[256];
      uint32_t hi[256];
      for (uint32_t g = 0; g < 256; ++g) {
        lo[g] = pa_dev::word_lo_entry(j, k, g);
        hi[g] = pa_dev::word_hi_entry(j, k, g);
      }
      for (uint32_t h = 0; h < 256; ++h)
        for (uint32_t l = 0; l < 256; ++l) out[l + 256 * h] = pa_dev::second_product_of(j, lo[l].t_lo, lo[l].t_hi, lo[l].a_hi, hi[h]);
      if (std::fwrite(out.data(), sizeof(uint64_t), out.size(), f) != out.size()) return 4;
    }
  }
  return std::fclose(f) == 0 ? 0 : 5;
}
