// pcoa.hip -- ordinate-run on the device (gfx950, wave64): the tall product Y = A Q, the centring of a distance matrix,
// and the entry point of the eigen-solver that does its products here.
//
// ordinate-run turns a finished run's distances into principal coordinates: the top k eigenpairs of the doubly centred
// matrix B of the squared distances.  Block subspace iteration needs only repeated products of the n x n matrix with a
// thin n x p block (p <= 32): n^2 p multiply-adds that read the n^2 8-byte cells once.  That product is the hot path and
// it is below; the p-wide algebra around it is host code (pcoa_host.cpp, pcoa::top_eigs), the same code for the host
// twin, so that the two differ by the product alone.  The definitions are this project's own (the reference has no
// ordination): include/pyani_hip.h and DESIGN.md section 7i have the contract, tests/pcoa_cases.py restates it
// independently, pcoa_host.cpp has the twins with the same bits, pcoa_rule.h the constants and formulas of both.
//
// The product.  The order of a sum is the contract's: within a chunk of kChunk columns ascending j into one accumulator,
// then the chunks' sums in ascending order.  mul_tall_kernel runs on a grid of (kRowTile-row tile) x (chunk) and writes
// each output's chunk sum; mul_tall_sum_kernel adds them.  Inside a chunk a lane owns its outputs -- rows lane % 64 and
// lane % 64 + 64 of the tile and PC consecutive columns of Q, the same for every lane of a wave -- and walks j upwards,
// so no sum is split between lanes and the tiling does not show in a result.
//   A   is read once, kSub columns of the tile's rows at a time: every wave reads whole 256-byte row segments into
//       registers while the sub-block before is being consumed, then stores them to LDS with a pitch of kSub + 1
//       doubles, so that a wave's 64 rows of one column fall into distinct banks;
//   Q   the chunk's rows of it go through LDS the same way, padded with zeros to kWaves * PC columns; a wave reads one
//       address at a time (a broadcast), once for both of a lane's rows: one row per lane, which reads Q from LDS
//       twice as often per cell of A, was measured slower at N = 10 000 (profiles/pcoa/README.md);
//   LDS 128 * 33 * 8 + 32 * 32 * 8 = 42 KB at most; 124 VGPRs at p = 11 (four waves a SIMD), 222 at p = 32 (two).
// The memory system bounds it: 8 bytes per cell of A against PC multiplications and additions.  No floating-point atomics.
//
// The centring.  Six launches: the check (distmat.hip, pa_nj's too), the rows' means of the squares (a lane per row,
// walking its column instead: D is bitwise symmetric and a column is read coalesced), the mean of the means (one lane:
// the order is the contract's), B and its diagonal, the rows' sums of B^2 (B is bitwise symmetric too), and one lane
// for the trace and the squared Frobenius norm.
#include "pa_internal.h"

#include "pcoa_rule.h"
#include "pcoa_solver.h"

namespace {

using pcoa::kChunk;
using pcoa::kSumStart;

constexpr int kThreads = 256;  // lanes per workgroup of the product and of the cell-wise kernels
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;  // column groups of the product: a wave's lanes share their columns of Q
constexpr int kRowsPerLane = 2;           // rows of the tile a lane owns: lane % 64 and 64 further on
constexpr int kRowTile = kWave * kRowsPerLane;  // rows per workgroup of the product
constexpr int kSub = 32;                  // columns of A staged in LDS at a time
constexpr int kPitch = kSub + 1;          // doubles between two rows of the staged tile
constexpr int kStage = kRowTile * kSub / kThreads;  // cells of A a lane stages per sub-block
constexpr int kMaxPC = (PA_MUL_TALL_MAX_P + kWaves - 1) / kWaves;
constexpr int kBatch = 8;        // loads of a lane in flight before the first is used (the column walks)
constexpr int kSumThreads = 64;  // the column walks: one lane per row, small workgroups so that more of them stream
static_assert(kChunk % kSub == 0, "a chunk is whole sub-blocks but for the matrix's last columns");
static_assert(kRowTile * kSub % kThreads == 0 && kThreads % kSub == 0, "the staging covers the sub-block with whole row segments");

// One (row tile, chunk): out[(chunk * n + i) * p + c] = the chunk's sum of A[i, j] * Q[j, c], ascending j.
template <int PC>
__global__ __launch_bounds__(kThreads) void mul_tall_kernel(const double *__restrict__ A, uint32_t n, const double *__restrict__ Q, uint32_t p,
                                                          double *__restrict__ out) {
  constexpr int kCols = kWaves * PC;  // columns of the staged Q, those at and past p zero
  constexpr int kStageQ = (kSub * kCols + kThreads - 1) / kThreads;  // cells of Q a lane stages per sub-block
  __shared__ double s_a[kRowTile * kPitch];
  __shared__ double s_q[kSub * kCols];
  const uint32_t row0 = blockIdx.x * kRowTile, chunk = blockIdx.y;
  const uint32_t j_begin = chunk * kChunk, j_end = j_begin + kChunk < n ? j_begin + kChunk : n;
  const uint32_t lane_row = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  // staging: cell t of this lane is row threadIdx.x / kSub + t * (kThreads / kSub), column threadIdx.x % kSub of the
  // sub-block; rows past the matrix repeat its last row (their lanes write nothing), columns past the chunk are not read
  const uint32_t st_col = threadIdx.x % kSub, st_row = threadIdx.x / kSub;
  double pre_a[kStage], pre_q[kStageQ];
  auto fetch = [&](uint32_t j0) {
#pragma unroll
    for (int t = 0; t < kStage; ++t) {
      const uint32_t i = row0 + st_row + t * (kThreads / kSub), j = j0 + st_col;
      pre_a[t] = j < j_end ? A[(uint64_t)(i < n ? i : n - 1) * n + j] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < kStageQ; ++t) {
      const uint32_t e = threadIdx.x + t * kThreads, j = j0 + e / kCols, c = e % kCols;
      pre_q[t] = e < (uint32_t)(kSub * kCols) && j < j_end && c < p ? Q[(uint64_t)j * p + c] : 0.0;
    }
  };
  double acc[kRowsPerLane][PC];
#pragma unroll
  for (int r = 0; r < kRowsPerLane; ++r)
#pragma unroll
    for (int t = 0; t < PC; ++t) acc[r][t] = kSumStart;
  const double *my_a = s_a + lane_row * kPitch, *my_q = s_q + wave * PC;
  auto consume = [&](uint32_t j) {
    double q[PC];
#pragma unroll
    for (int t = 0; t < PC; ++t) q[t] = my_q[j * kCols + t];
#pragma unroll
    for (int r = 0; r < kRowsPerLane; ++r) {
      const double a = my_a[r * kWave * kPitch + j];
#pragma unroll
      for (int t = 0; t < PC; ++t) acc[r][t] = pcoa::mul_add(acc[r][t], a, q[t]);
    }
  };
  fetch(j_begin);
  for (uint32_t j0 = j_begin; j0 < j_end; j0 += kSub) {
    __syncthreads();  // the sub-block before has been consumed
#pragma unroll
    for (int t = 0; t < kStage; ++t) s_a[(st_row + t * (kThreads / kSub)) * kPitch + st_col] = pre_a[t];
#pragma unroll
    for (int t = 0; t < kStageQ; ++t)
      if (threadIdx.x + t * kThreads < (uint32_t)(kSub * kCols)) s_q[threadIdx.x + t * kThreads] = pre_q[t];
    __syncthreads();
    if (j0 + kSub < j_end) fetch(j0 + kSub);
    const uint32_t cols = j_end - j0;
    if (cols >= (uint32_t)kSub) {
#pragma unroll 16
      for (uint32_t j = 0; j < (uint32_t)kSub; ++j) consume(j);
    } else {
      for (uint32_t j = 0; j < cols; ++j) consume(j);
    }
  }
#pragma unroll
  for (int r = 0; r < kRowsPerLane; ++r) {
    const uint32_t i = row0 + lane_row + r * kWave;
    if (i >= n) continue;
#pragma unroll
    for (int t = 0; t < PC; ++t) {
      const uint32_t c = wave * PC + t;
      if (c < p) out[((uint64_t)chunk * n + i) * p + c] = acc[r][t];
    }
  }
}

// Y[i, c] = the chunks' sums in ascending order
__global__ __launch_bounds__(kThreads) void mul_tall_sum_kernel(const double *__restrict__ partial, uint64_t cells, uint32_t chunks,
                                                              double *__restrict__ Y) {
  const uint64_t at = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (at >= cells) return;
  double y = kSumStart;
  for (uint32_t b = 0; b < chunks; ++b) y = y + partial[(uint64_t)b * cells + at];
  Y[at] = y;
}

uint32_t chunks_of(uint32_t n) { return (n + kChunk - 1) / kChunk; }

template <int PC>
int launch_mul_tall(pa_ctx *c, const double *d_A, uint32_t n, const double *d_Q, uint32_t p, double *d_out) {
  return PA_LAUNCH(c, mul_tall_kernel<PC>, LaunchDim((n + kRowTile - 1) / kRowTile, chunks_of(n)), kThreads, 0, d_A, n, d_Q, p, d_out);
}

// The product with the partial sums' place given: chunks_of(n) * n * p doubles (not touched for a single chunk)
int mul_tall(pa_ctx *c, const double *d_A, uint32_t n, const double *d_Q, uint32_t p, double *d_Y, double *d_partial) {
  const uint32_t chunks = chunks_of(n);
  double *out = chunks == 1 ? d_Y : d_partial;  // one chunk: its sums are the result
  switch ((p + kWaves - 1) / kWaves) {
    case 1: PA_TRY(launch_mul_tall<1>(c, d_A, n, d_Q, p, out)); break;
    case 2: PA_TRY(launch_mul_tall<2>(c, d_A, n, d_Q, p, out)); break;
    case 3: PA_TRY(launch_mul_tall<3>(c, d_A, n, d_Q, p, out)); break;
    case 4: PA_TRY(launch_mul_tall<4>(c, d_A, n, d_Q, p, out)); break;
    case 5: PA_TRY(launch_mul_tall<5>(c, d_A, n, d_Q, p, out)); break;
    case 6: PA_TRY(launch_mul_tall<6>(c, d_A, n, d_Q, p, out)); break;
    case 7: PA_TRY(launch_mul_tall<7>(c, d_A, n, d_Q, p, out)); break;
    default: PA_TRY(launch_mul_tall<kMaxPC>(c, d_A, n, d_Q, p, out)); break;
  }
  static_assert(kMaxPC == 8, "one case per number of columns a lane may own");
  if (chunks == 1) return PA_OK;
  const uint64_t cells = (uint64_t)n * p;
  return PA_LAUNCH(c, mul_tall_sum_kernel, (cells + kThreads - 1) / kThreads, kThreads, 0, (const double *)d_partial, cells, chunks, d_Y);
}

uint64_t partial_doubles(uint32_t n, uint32_t p) { return chunks_of(n) > 1 ? (uint64_t)chunks_of(n) * n * p : 0; }

// ---- the centring
// out[i] = (M[i, 0]^2 + ... + M[i, n - 1]^2) / divisor for a bitwise symmetric M, by walking k upwards: M[k, i] is
// M[i, k] bit for bit and is read coalesced across i
__global__ __launch_bounds__(kSumThreads) void gower_row_squares_kernel(const double *__restrict__ M, uint32_t n, double divisor,
                                                                       double *__restrict__ out) {
  const uint32_t i = blockIdx.x * kSumThreads + threadIdx.x;
  if (i >= n) return;
  double s = kSumStart;
  for (uint32_t k0 = 0; k0 < n; k0 += kBatch) {  // kBatch loads in flight, then the additions in order
    double v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) v[j] = k0 + j < n ? M[(uint64_t)(k0 + j) * n + i] : 0.0;
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
      if (k0 + j < n) s = s + pcoa::squared(v[j]);
  }
  out[i] = s / divisor;
}

// One lane, because the order of these sums is the contract's: out[0] = (x[0] + ... + x[n - 1]) / divisor and, with y,
// out[1] = y[0] + ... + y[n - 1]
__global__ void gower_sums_kernel(const double *__restrict__ x, const double *__restrict__ y, uint32_t n, double divisor, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = kSumStart, t = kSumStart;
  for (uint32_t i = 0; i < n; ++i) {
    s = s + x[i];
    if (y) t = t + y[i];
  }
  out[0] = s / divisor;
  if (y) out[1] = t;
}

// Row blockIdx.y of B, and its diagonal cell once more in diag
__global__ __launch_bounds__(kThreads) void gower_center_kernel(const double *__restrict__ D, uint32_t n, const double *__restrict__ r,
                                                              const double *__restrict__ g, double *__restrict__ B, double *__restrict__ diag) {
  const uint32_t i = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint64_t at = (uint64_t)i * n + j;
  const double b = pcoa::centred(pcoa::squared(D[at]), r[i], r[j], *g);
  B[at] = b;
  if (i == j) diag[i] = b;
}

}  // namespace

extern "C" int pa_mul_tall_f64(pa_ctx *c, const double *d_A, uint32_t n, const double *d_Q, uint32_t p, double *d_Y) {
  PA_REQUIRE(c != nullptr, "pa_mul_tall_f64: null context");
  PA_REQUIRE(n >= 1 && n <= 65535, "pa_mul_tall_f64: %u rows; 1 to 65535", n);
  PA_REQUIRE(p >= 1 && p <= PA_MUL_TALL_MAX_P, "pa_mul_tall_f64: %u columns; 1 to %d", p, PA_MUL_TALL_MAX_P);
  PA_REQUIRE(d_A != nullptr && d_Q != nullptr && d_Y != nullptr, "pa_mul_tall_f64: null argument");
  PA_HIP(hipSetDevice(c->device));
  double *d_partial;
  PA_TRY(pa_carve(c->pcoa_work, "pcoa_work", [&](Carve &k) { d_partial = k.take<double>(partial_doubles(n, p)); }));
  return mul_tall(c, d_A, n, d_Q, p, d_Y, d_partial);
}

extern "C" int pa_gower_center(pa_ctx *c, const double *d_D, uint32_t n, double *d_B, double *h_trace, double *h_fro2) {
  PA_REQUIRE(c != nullptr, "pa_gower_center: null context");
  PA_REQUIRE(n >= 1 && n <= 65535, "pa_gower_center: %u rows; 1 to 65535", n);
  PA_REQUIRE(d_D != nullptr && d_B != nullptr && h_trace != nullptr && h_fro2 != nullptr, "pa_gower_center: null argument");
  PA_HIP(hipSetDevice(c->device));
  PA_TRY(pa_check_distance_matrix(c, "pa_gower_center", d_D, n));  // one read-back
  // workspace: r, the rows' sums of B^2, B's diagonal, then g, the trace and the squared norm
  double *r, *row_sq, *diag, *g, *totals;
  PA_TRY(pa_carve(c->pcoa_work, "pcoa_work", [&](Carve &k) {
    r = k.take<double>(n); row_sq = k.take<double>(n); diag = k.take<double>(n); g = k.take<double>(1); totals = k.take<double>(2);
  }));
  const uint32_t sum_blocks = (n + kSumThreads - 1) / kSumThreads;
  PA_TRY(PA_LAUNCH(c, gower_row_squares_kernel, sum_blocks, kSumThreads, 0, d_D, n, (double)n, r));
  PA_TRY(PA_LAUNCH(c, gower_sums_kernel, 1, kWave, 0, (const double *)r, (const double *)nullptr, n, (double)n, g));
  PA_TRY(PA_LAUNCH(c, gower_center_kernel, LaunchDim((n + kThreads - 1) / kThreads, n), kThreads, 0, d_D, n, (const double *)r, (const double *)g, d_B, diag));
  PA_TRY(PA_LAUNCH(c, gower_row_squares_kernel, sum_blocks, kSumThreads, 0, (const double *)d_B, n, 1.0, row_sq));
  PA_TRY(PA_LAUNCH(c, gower_sums_kernel, 1, kWave, 0, (const double *)diag, (const double *)row_sq, n, 1.0, totals));
  double out[2] = {0.0, 0.0};
  PA_TRY(pa_read_back(c, (const double *)totals, out, 2));
  *h_trace = out[0];
  *h_fro2 = out[1];
  return PA_OK;
}

extern "C" int pa_symm_top_eigs(pa_ctx *c, const double *d_B, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2,
                                double *h_values, double *h_vectors, double *h_residuals, double *h_info) {
  PA_REQUIRE(c != nullptr, "pa_symm_top_eigs: null context");
  PA_REQUIRE(d_B != nullptr, "pa_symm_top_eigs: null matrix");
  PA_HIP(hipSetDevice(c->device));
  // the product of one iteration: the block goes up, the two launches, the block comes down
  auto product = [c, d_B, n](const double *h_Q, uint32_t p, double *h_Y) -> int {
    const uint64_t block = (uint64_t)n * p;
    double *d_Q, *d_Y, *d_partial;
    PA_TRY(pa_carve(c->pcoa_work, "pcoa_work", [&](Carve &k) {
      d_Q = k.take<double>(block); d_Y = k.take<double>(block); d_partial = k.take<double>(partial_doubles(n, p));
    }));
    PA_HIP(hipMemcpyAsync(d_Q, h_Q, block * 8, hipMemcpyHostToDevice, c->stream));
    PA_TRY(mul_tall(c, d_B, n, d_Q, p, d_Y, d_partial));
    return pa_copy_to_host(c, h_Y, d_Y, block * 8);
  };
  return pcoa::top_eigs("pa_symm_top_eigs", n, k, tol, max_iter, fro2, product, h_values, h_vectors, h_residuals, h_info);
}
