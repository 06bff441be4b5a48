// distmat.hip -- the check of a distance matrix on the device (gfx950, wave64), for every entry point that takes one:
// pa_nj, pa_gower_center, pa_mantel.  distmat_rule.h has the rule of a cell, distmat_host.cpp the host twin and the
// message.  One launch per matrix, one read-back for all of them.
#include "pa_internal.h"

#include "distmat_rule.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxMatrices = kDistBad.words / 4;  // two 64-bit words each

// bad[0] counts the cells that break the rule, bad[1] is the first of them in row-major order
__global__ __launch_bounds__(kThreads) void distmat_validate_kernel(const double *__restrict__ D, uint32_t n, unsigned long long *__restrict__ bad) {
  const uint64_t cells = (uint64_t)n * n;
  uint64_t count = 0, first = ~0ull;
  for (uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x; at < cells; at += (uint64_t)gridDim.x * kThreads) {
    const uint32_t i = (uint32_t)(at / n), j = (uint32_t)(at % n);
    if (distmat::bad_cell(D[at], D[(uint64_t)j * n + i], i == j)) {
      ++count;
      if (at < first) first = at;
    }
  }
  if (count) {  // integer atomics: the count and the minimum do not depend on the order
    atomicAdd(&bad[0], (unsigned long long)count);
    atomicMin(&bad[1], (unsigned long long)first);
  }
}

}  // namespace

int pa_check_distance_matrices(pa_ctx *c, const char *who, const char *const *names, const double *const *d_M, int count, uint32_t n) {
  PA_REQUIRE(count >= 1 && count <= kMaxMatrices, "%s: %d matrices to check; 1 to %d", who, count, kMaxMatrices);
  unsigned long long *d_bad = c->slot<unsigned long long>(kDistBad);
  const uint64_t cells = (uint64_t)n * n;
  for (int m = 0; m < count; ++m) {
    PA_HIP(hipMemsetAsync(d_bad + 2 * m, 0, 8, c->stream));
    PA_HIP(hipMemsetAsync(d_bad + 2 * m + 1, 0xFF, 8, c->stream));
    PA_TRY(PA_LAUNCH(c, distmat_validate_kernel, std::min<uint64_t>((cells + kThreads - 1) / kThreads, 1u << 16), kThreads, 0, d_M[m], n, d_bad + 2 * m));
  }
  unsigned long long bad[2 * kMaxMatrices] = {};
  PA_TRY(pa_read_back(c, (const unsigned long long *)d_bad, bad, 2u * (uint32_t)count));
  for (int m = 0; m < count; ++m)
    if (bad[2 * m]) return distmat::refuse(who, names[m], n, bad[2 * m], bad[2 * m + 1]);
  return PA_OK;
}
