// The launcher's arithmetic (pa_launch_geom.h: ceil_div, stride_blocks, launch_verdict, dispatch_value) under AddressSanitizer / UBSan:
// a stand-alone CPU program, no HIP runtime.
//   usage: launch_geom
#include <cstdio>
#include <vector>

#include "../../../pyani_plus_amd/csrc/pa_launch_geom.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int main() {
  // limits as an MI355X reports them, and a second, odd set: the verdict reads them, it holds no constants of its own
  const LaunchLimits sets[2] = {{{2147483647ull, 65536ull, 65536ull}, {1024, 1024, 1024}, 1024}, {{1000, 7, 3}, {96, 5, 2}, 128}};
  for (const LaunchLimits &lim : sets) {
    for (int d = 0; d < 3; ++d) {
      // block counts 0, 1, the limit and the limit + 1 in dimension d, the other two at 1
      const uint64_t counts[4] = {0, 1, lim.grid[d], lim.grid[d] + 1};
      const LaunchVerdict want[4] = {LaunchVerdict::kEmptyGrid, LaunchVerdict::kGo, LaunchVerdict::kGo, LaunchVerdict::kOutsideLimits};
      for (int i = 0; i < 4; ++i) {
        uint64_t g[3] = {1, 1, 1};
        g[d] = counts[i];
        CHECK(launch_verdict(LaunchDim(g[0], g[1], g[2]), 64, lim) == want[i]);
      }
      // an empty grid is nothing to do even where another dimension is beyond its limit
      uint64_t g[3] = {lim.grid[0] + 1, lim.grid[1] + 1, lim.grid[2] + 1};
      g[d] = 0;
      CHECK(launch_verdict(LaunchDim(g[0], g[1], g[2]), 64, lim) == LaunchVerdict::kEmptyGrid);
      // the same four sizes for the block
      const uint64_t threads[4] = {0, 1, lim.block[d], lim.block[d] + 1};
      for (int i = 0; i < 4; ++i) {
        uint64_t b[3] = {1, 1, 1};
        b[d] = threads[i];
        CHECK(launch_verdict(1, LaunchDim(b[0], b[1], b[2]), lim) == (i == 1 || i == 2 ? LaunchVerdict::kGo : LaunchVerdict::kOutsideLimits));
      }
    }
    // every dimension within its own limit, the product of the block's beyond the threads of a block
    CHECK(launch_verdict(1, LaunchDim(lim.block[0], 2, 1), lim) == LaunchVerdict::kOutsideLimits);
    CHECK(launch_verdict(1, LaunchDim(lim.threads_per_block / 2, 2, 1), lim) == LaunchVerdict::kGo);
    CHECK(launch_verdict(LaunchDim(lim.grid[0], lim.grid[1], lim.grid[2]), LaunchDim(lim.threads_per_block / 2, 2, 1), lim) == LaunchVerdict::kGo);
  }
  // a 64-bit block count that 32 bits would have cut to a small, valid one: 2^32 + 5 blocks of 256
  const uint64_t n = ((1ull << 32) + 5) * 256 - 17;
  CHECK(ceil_div(n, 256) == (1ull << 32) + 5);
  CHECK((uint32_t)ceil_div(n, 256) == 5u);
  CHECK(launch_verdict(ceil_div(n, 256), 256, sets[0]) == LaunchVerdict::kOutsideLimits);
  CHECK(launch_verdict(LaunchDim(1, 1ull << 32, 1), 256, sets[0]) == LaunchVerdict::kOutsideLimits);
  CHECK(launch_verdict(LaunchDim(1, 1, (1ull << 32) + 1), 256, sets[0]) == LaunchVerdict::kOutsideLimits);
  // ceil_div at its edges: no a + b - 1 that wraps
  CHECK(ceil_div(0, 256) == 0 && ceil_div(1, 256) == 1 && ceil_div(256, 256) == 1 && ceil_div(257, 256) == 2);
  CHECK(ceil_div(~0ull, 1) == ~0ull && ceil_div(~0ull, 2) == (1ull << 63) && ceil_div(~0ull, ~0ull) == 1 && ceil_div(~0ull - 1, ~0ull) == 1);
  // the grid of a grid-stride pass: a workgroup per 256 elements up to 1024 of them, then it stays
  CHECK(stride_blocks(0) == 0 && stride_blocks(1) == 1 && stride_blocks(256) == 1 && stride_blocks(257) == 2);
  CHECK(stride_blocks(1024 * 256 - 1) == 1024 && stride_blocks(1024 * 256) == 1024 && stride_blocks(1024 * 256 + 1) == 1024);
  CHECK(stride_blocks(1023 * 256) == 1023 && stride_blocks(1023 * 256 + 1) == 1024 && stride_blocks((1ull << 40) - 1) == 1024 && stride_blocks(~0ull) == 1024);

  // the value dispatch: each listed value reaches its own case once and no other, a value off the list reports a miss
  static_assert(std::is_same<value_list<1, 4>, std::integer_sequence<int, 1, 2, 3, 4>>::value, "consecutive values");
  static_assert(std::is_same<value_list<256, 5, 64>, std::integer_sequence<int, 256, 320, 384, 448, 512>>::value, "values with a step");
  auto exercise = [](auto list, int lo, int hi, int step) {
    for (int v = lo - 2 * step; v <= hi + 2 * step; ++v) {
      std::vector<int> reached;
      const bool hit = dispatch_value(v, list, [&](auto constant) { reached.push_back(decltype(constant)::value); });
      const bool listed = v >= lo && v <= hi && (v - lo) % step == 0;
      CHECK(hit == listed);
      CHECK(listed ? (reached.size() == 1 && reached[0] == v) : reached.empty());
    }
  };
  exercise(value_list<1, 16>{}, 1, 16, 1);        // threads per bit row
  exercise(value_list<8, 9>{}, 8, 16, 1);         // fragment ANI's k
  exercise(value_list<256, 5, 64>{}, 256, 512, 64);  // the mapping kernel's stretch capacity
  exercise(value_list<2, 7>{}, 2, 8, 1);          // planes of the MSA pair kernel
  exercise(value_list<1, 64>{}, 1, 64, 1);        // the k-mer hash's k
  int calls = 0;
  CHECK(!dispatch_value((int64_t)(1ull << 32) + 8, value_list<8, 9>{}, [&](auto) { ++calls; }) && calls == 0);  // no match by the low 32 bits
  CHECK(!dispatch_value(-1, value_list<1, 16>{}, [&](auto) { ++calls; }) && calls == 0);

  if (failures) return 1;
  printf("launch geometry and value dispatch agree\n");
  return 0;
}
