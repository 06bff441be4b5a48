// pa_launch_geom.h -- the arithmetic of a kernel launch and the run-time value dispatch: pure functions of sizes and
// limits, no HIP runtime, so that a host compiler (and tests/tools/sanitize/launch_geom_main.cpp) can reach them.
#pragma once

#include <cstdint>
#include <type_traits>
#include <utility>

// ceil(a / b) in 64 bits, without the overflow of a + b - 1
constexpr uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// A grid in blocks or a block in threads.  64-bit, so that a count that does not fit the device is refused by
// launch_verdict instead of being cut off on the way; a plain count converts to the 1-D form.
struct LaunchDim {
  uint64_t x, y, z;
  constexpr LaunchDim(uint64_t x_, uint64_t y_ = 1, uint64_t z_ = 1) : x(x_), y(y_), z(z_) {}
};
// hipDeviceProp_t's maxGridSize, maxThreadsDim and maxThreadsPerBlock
struct LaunchLimits {
  uint64_t grid[3], block[3], threads_per_block;
};
enum class LaunchVerdict { kGo, kEmptyGrid, kOutsideLimits };
// An empty grid (a dimension of 0) is nothing to do; anything else must fit the device: every grid dimension, every
// block dimension (at least 1 each) and the block's threads.
constexpr LaunchVerdict launch_verdict(LaunchDim grid, LaunchDim block, const LaunchLimits &lim) {
  if (grid.x == 0 || grid.y == 0 || grid.z == 0) return LaunchVerdict::kEmptyGrid;
  const uint64_t g[3] = {grid.x, grid.y, grid.z}, b[3] = {block.x, block.y, block.z};
  uint64_t threads = 1;
  for (int d = 0; d < 3; ++d) {
    if (g[d] > lim.grid[d] || b[d] == 0 || b[d] > lim.block[d]) return LaunchVerdict::kOutsideLimits;
    threads *= b[d];  // each factor is within its limit (a few thousand): no overflow
  }
  return threads <= lim.threads_per_block ? LaunchVerdict::kGo : LaunchVerdict::kOutsideLimits;
}

// The grid of a grid-stride pass of 256-lane workgroups over n elements: ceil(n / 256) workgroups, at most 1024 (four
// for each of the 256 CUs); workgroup b takes the elements 256 b + lane, then every 256 * grid further on.
constexpr uint32_t kStrideThreads = 256, kStrideMaxBlocks = 1024;
constexpr uint32_t stride_blocks(uint64_t n) {
  const uint64_t want = ceil_div(n, kStrideThreads);
  return (uint32_t)(want < kStrideMaxBlocks ? want : kStrideMaxBlocks);
}

// ---- run-time value to template argument --------------------------------------------------------------------------
// Calls fn(std::integral_constant<int, V>{}) for the V of the list that equals v; false if none does, for the caller
// to set its own error or take its own default.
template <int... Vs, class Fn>
bool dispatch_value(int64_t v, std::integer_sequence<int, Vs...>, Fn &&fn) {
  return ((v == Vs && (fn(std::integral_constant<int, Vs>{}), true)) || ...);
}
// the list First, First + Step, ... of Count values
template <int First, int Step, int... I>
constexpr auto value_list_from(std::integer_sequence<int, I...>) { return std::integer_sequence<int, First + Step * I...>{}; }
template <int First, int Count, int Step = 1>
using value_list = decltype(value_list_from<First, Step>(std::make_integer_sequence<int, Count>{}));
