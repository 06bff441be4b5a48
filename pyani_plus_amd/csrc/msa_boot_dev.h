// msa_boot_dev.h -- the bit-sliced column weights of a batch of bootstrap replicates, stated once for msa_boot.hip (the
// two weighted counts of bootstrap-run) and subst.hip (the three of phylo-run): the kernel that slices the uploaded
// bytes into planes, the workspace of a launch and the upload of a batch.  The unnamed namespace keeps the kernel's
// symbol what it was when msa_boot.hip alone had it.
#pragma once

#include "msa_tile_dev.h"

namespace {
using namespace msa_tile;

constexpr uint32_t kBatch = PA_MSA_BOOT_BATCH;
static_assert(kBatch <= 65535, "the batch is the grid's z axis");
static_assert(kChunk * kMaxBits <= kThreads, "one lane stages one weight word");

// wplanes[(rep * n_words + w) * 8 + beta]: the 8 planes of a word side by side, zero from the batch's nb on.
// weights: n_reps rows of `stride` bytes (a multiple of 32, 16-byte aligned, zero at and past n_cols).
__global__ __launch_bounds__(kThreads) void boot_weight_planes_kernel(const uint8_t *__restrict__ weights, uint64_t stride, uint32_t n_words,
                                                                      uint32_t n_reps, uint32_t *__restrict__ wplanes) {
  const uint64_t total = (uint64_t)n_reps * n_words;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kThreads) {
    const uint32_t rep = (uint32_t)(i / n_words), w = (uint32_t)(i % n_words);
    const uint4 *p16 = reinterpret_cast<const uint4 *>(weights + (uint64_t)rep * stride + (uint64_t)w * 32u);
    const uint4 v0 = p16[0], v1 = p16[1];
    const uint32_t words[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t out[kMaxBits] = {0};
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const uint32_t v = (words[j >> 2] >> (8 * (j & 3))) & 0xffu;
#pragma unroll
      for (uint32_t beta = 0; beta < kMaxBits; ++beta) out[beta] |= ((v >> beta) & 1u) << j;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(wplanes + i * kMaxBits);
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
  }
}

// The weight words [wc, wc + kChunk) of replicate blockIdx.z's planes `wp` into sw, beside the tile's rows (between the
// two barriers of a stage); words at or past w_hi as zero
__device__ inline void stage_weight_words(uint32_t (&sw)[kChunk][kMaxBits], const uint32_t *__restrict__ wp, uint32_t wc, uint32_t w_hi, uint32_t tid) {
  if (tid < kChunk * kMaxBits) {
    const uint32_t w = wc + tid / kMaxBits;
    (&sw[0][0])[tid] = w < w_hi ? wp[(uint64_t)w * kMaxBits + tid % kMaxBits] : 0u;
  }
}

// the workspace of a launch over up to kBatch replicates (pa_ctx::boot_work)
struct Work {
  uint8_t *weights;   // kBatch rows of `stride` bytes
  uint32_t *wplanes;  // kBatch x n_words x 8
  static uint64_t stride(uint64_t n_words) { return n_words * 32u; }
  void layout(Carve &k, uint64_t n_words) {
    weights = k.take<uint8_t>((uint64_t)kBatch * stride(n_words), 32);  // each row a multiple of 32 further on
    wplanes = k.take<uint32_t>((uint64_t)kBatch * n_words * kMaxBits);
  }
};

// Rows [r0, r0 + count) of h_weights (rows of n_cols bytes) up into w.weights and sliced into w.wplanes, on the
// context's stream, which still reads h_weights when this returns
inline int upload_weight_planes(pa_ctx *c, const Work &w, const uint8_t *h_weights, uint32_t r0, uint32_t count, uint64_t n_cols, uint32_t n_words) {
  const uint64_t stride = Work::stride(n_words);
  PA_HIP(hipMemsetAsync(w.weights, 0, (uint64_t)count * stride, c->stream));
  PA_HIP(hipMemcpy2DAsync(w.weights, stride, h_weights + (uint64_t)r0 * n_cols, n_cols, n_cols, count, hipMemcpyHostToDevice, c->stream));
  return PA_LAUNCH(c, boot_weight_planes_kernel, stride_blocks((uint64_t)count * n_words), kThreads, 0, (const uint8_t *)w.weights, stride, n_words, count,
                   w.wplanes);
}

}  // namespace
