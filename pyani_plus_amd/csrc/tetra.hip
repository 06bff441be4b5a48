// tetra.hip -- the two device steps of the TETRA-hip method (gfx950, wave64): the di-, tri- and tetranucleotide counts of
// every genome of an arena, and the correlations between the genomes' unit rows of tetranucleotide Z-scores.
//
// Replaces nothing in the reference: pyani-plus has no TETRA method.  The definition in include/pyani_hip.h and
// DESIGN.md section 7g is this project's own contract (after Teeling et al. 2004); no bit parity with pyani or JSpecies
// is claimed.  The Z-scores between the two kernels are 256 values per genome and are computed on the host
// (tetra_host.cpp).
//
// ---- tetra_counts_kernel --------------------------------------------------------------------------------------------
// One pass over the packed arena.  A workgroup takes a chunk of kChunkBlocks 64-position blocks of ONE genome (the host
// hands it the chunk table: genome g owns chunks [chunk_off[g], chunk_off[g + 1])); a lane takes one block per iteration,
// one 16-byte packed load, plus the three bases before it from the previous word.  The lane owns the window family of
// every start s = 64 t - 3 .. 64 t + 60, that is the 4-window that ENDS in its block: the look-back form, because then the
// arena's dirty bitmap says exactly what the lane needs -- bit t is set when block t or the 32 positions before it hold
// an invalid position -- and a block whose bit is clear counts its 64 tetranucleotides without reading the mask
// (kmer_hash.hip's clean-block path).  The first block of a genome has no look-back, the last one also owns the starts
// 64 t + 61 and 64 t + 62 whose longer windows would leave the genome: both take the masked path.
//
// Only ONE histogram update is made per start: the longest of the windows of length 4, 3, 2 from that start that is
// valid.  With hist4, extra3 and extra2 the counts of those updates,
//     F4[w] = hist4[w],  F3[abc] = sum_d hist4[abcd] + extra3[abc],  F2[ab] = sum_c F3[abc] + extra2[ab]:
// every valid 3-window is either the prefix of a valid 4-window from the same start or was counted in extra3, and
// likewise for 2-windows.  That is a third of the LDS atomics of counting the three spectra directly; the direct form is
// the kernel's kDirect instance, kept for the measurement that chose between them (PA_TETRA_DIRECT=1 in the tools build,
// tools/tetra_bench.py).
//
// The updates are no-return 32-bit LDS atomics (ds_add_u32) into kCopies private histograms per workgroup, the copy
// chosen by the lane, so that a homopolymer -- 64 lanes, one bin -- spreads over kCopies addresses.  The LDS bins are
// indexed as the bases lie in the packed word (first base in the low bits); the flush reverses the digits to the
// contract's index (first base most significant) and adds each non-zero bin to the genome's row with one 64-bit
// vector global atomic.  Integer sums: the result does not depend on the order, two runs give the same counts.
//
// ---- tetra_corr_kernel ----------------------------------------------------------------------------------------------
// The tile skeleton of pairs_f64_tile.h (which has the layout) with a product as its term and the 256 columns known at
// compile time: 64 x 64 pairs per 256-thread workgroup, 4 x 4 pairs per lane.  Bit
// contract: one accumulator per pair, acc = acc + U_a[k] * U_b[k] for k = 0 .. 255 ascending, the product rounded before
// the addition (contraction is off for this file, and the Makefile passes -ffp-contract=off), no split over k, no
// atomics; r = min(1, max(-1, acc)), NaN kept; the diagonal (same genome index) is exactly 1.0 unless NaN.  The f64 matrix
// rate of this device is no higher than its vector rate, so this is a register-tiled vector kernel: the order of the
// additions stays defined.
#include "pa_internal.h"

#include "pairs_f64_tile.h"

namespace {

// ---- counts ---------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kBlocksPerLane = 16;                           // iterations of a workgroup over its chunk
constexpr uint32_t kChunkBlocks = kThreads * kBlocksPerLane;  // 64-position blocks per workgroup: 262 144 positions
constexpr int kCopies = 16;                                  // private histograms per workgroup
constexpr int kBins = PA_TETRA_BINS;                         // 256 + 64 + 16
constexpr int kCopyStride = kBins + 1;                       // odd: the copies start in different banks
constexpr int kOff3 = 256, kOff2 = 320;                      // where extra3 / extra2 start in a copy

// the k 2-bit digits of x in reverse order: packed order (first base lowest) <-> the contract's (first base highest)
__host__ __device__ constexpr uint32_t rev_digits(uint32_t x, int k) {
  uint32_t r = 0;
  for (int i = 0; i < k; ++i) r |= ((x >> (2 * i)) & 3u) << (2 * (k - 1 - i));
  return r;
}

// largest g with chunk_off[g] <= chunk   (n + 1 ascending entries, chunk < chunk_off[n]; empty genomes repeat an entry)
__device__ __forceinline__ uint32_t find_chunk_genome(const uint32_t *__restrict__ chunk_off, uint32_t n, uint32_t chunk) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

template <bool kDirect>
__global__ __launch_bounds__(kThreads) void tetra_counts_kernel(const uint4 *__restrict__ packed, const uint2 *__restrict__ mask,
                                                                const uint64_t *__restrict__ dirty, const uint32_t *__restrict__ genome_blk,
                                                                const uint32_t *__restrict__ chunk_off, uint32_t n_genomes,
                                                                unsigned long long *__restrict__ counts) {
  __shared__ uint32_t hist[kCopies * kCopyStride];
  __shared__ uint32_t f3[64];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < kCopies * kCopyStride; i += kThreads) hist[i] = 0u;
  const uint32_t chunk = blockIdx.x;
  const uint32_t g = find_chunk_genome(chunk_off, n_genomes, chunk);  // uniform in the workgroup
  const uint32_t g_first = genome_blk[g], g_end = genome_blk[g + 1];
  const uint32_t blk0 = g_first + (chunk - chunk_off[g]) * kChunkBlocks;
  uint32_t *const mine = hist + (tid % kCopies) * kCopyStride;
  __syncthreads();

#pragma unroll 1
  for (int it = 0; it < kBlocksPerLane; ++it) {
    const uint32_t t = blk0 + (uint32_t)it * kThreads + tid;
    if (t >= g_end) break;  // (the lanes past the genome's end are the last of the workgroup: nothing follows for them)
    const uint4 cur = packed[t];
    const bool first = t == g_first, last = t + 1 == g_end;
    // bases -16 .. -1; of a genome's first block they are another genome's and are masked out below
    const uint32_t pw = first ? 0u : reinterpret_cast<const uint32_t *>(packed)[4 * (uint64_t)t - 1];
    const uint32_t W[6] = {pw, cur.x, cur.y, cur.z, cur.w, 0u};
    const bool is_dirty = (dirty[t >> 6] >> (t & 63u)) & 1ull;
    if (!is_dirty && !first && !last) {
      // clean: the 64 starts -3 .. 60 all have a valid 4-window.  Start s is base s + 16 of W, bits 2 (s + 16) ..+7
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        constexpr int kLead = 13;  // start -3 is base 13 of W
        const int base = i + kLead, d = base >> 4, sh = 2 * (base & 15);
        const uint32_t w = (sh <= 24 ? W[d] >> sh : __builtin_amdgcn_alignbit(W[d + 1], W[d], sh)) & 0xffu;
        atomicAdd(&mine[w], 1u);
        if constexpr (kDirect) {
          atomicAdd(&mine[kOff3 + (w & 0x3fu)], 1u);
          atomicAdd(&mine[kOff2 + (w & 0xfu)], 1u);
        }
      }
      continue;
    }
    // masked path.  inv: bit i <-> position i - 3 of the block is invalid, i = 0 .. 69; 64 .. 66 (positions 61 .. 63)
    // come from the mask, 67 .. 69 stand for the positions after the block: the windows that reach them are the next
    // block's, or -- in the genome's last block -- leave the genome
    const uint2 m = mask[t];
    const uint64_t m64 = ((uint64_t)m.y << 32) | m.x;
    const uint32_t back = first ? 7u : (mask[t - 1].y >> 29);
    const uint64_t inv_lo = (m64 << 3) | back;
    const uint32_t inv_hi = (uint32_t)(m64 >> 61) | 0x38u;
    // bad_k: bit i <-> the window of k positions from start i - 3 holds an invalid position
    auto shr = [&](int s, uint64_t &lo, uint32_t &hi) {
      lo = (inv_lo >> s) | ((uint64_t)inv_hi << (64 - s));
      hi = inv_hi >> s;
    };
    uint64_t s1_lo, s2_lo, s3_lo;
    uint32_t s1_hi, s2_hi, s3_hi;
    shr(1, s1_lo, s1_hi);
    shr(2, s2_lo, s2_hi);
    shr(3, s3_lo, s3_hi);
    const uint64_t bad2_lo = inv_lo | s1_lo, bad3_lo = bad2_lo | s2_lo, bad4_lo = bad3_lo | s3_lo;
    const uint32_t bad2_hi = inv_hi | s1_hi, bad3_hi = bad2_hi | s2_hi;
    // starts 0 .. 63 (positions -3 .. 60), and in the genome's last block 64 and 65 (positions 61, 62: no 4-window)
    const int n_starts = last ? 66 : 64;
#pragma unroll 1
    for (int i = 0; i < n_starts; ++i) {
      const bool hi_part = i >= 64;
      const uint32_t b2 = hi_part ? (bad2_hi >> (i - 64)) & 1u : (uint32_t)(bad2_lo >> i) & 1u;
      if (b2) continue;  // not even two valid positions
      const uint32_t b3 = hi_part ? (bad3_hi >> (i - 64)) & 1u : (uint32_t)(bad3_lo >> i) & 1u;
      const uint32_t b4 = hi_part ? 1u : (uint32_t)(bad4_lo >> i) & 1u;
      const int base = i + 13, d = base >> 4, sh = 2 * (base & 15);  // d <= 4: W[d + 1] exists
      const uint32_t w = __builtin_amdgcn_alignbit(W[d + 1], W[d], sh) & 0xffu;  // a shift of 0 returns the low operand
      if constexpr (kDirect) {
        if (!b4) atomicAdd(&mine[w], 1u);
        if (!b3) atomicAdd(&mine[kOff3 + (w & 0x3fu)], 1u);
        atomicAdd(&mine[kOff2 + (w & 0xfu)], 1u);
      } else {
        if (!b4) atomicAdd(&mine[w], 1u);
        else if (!b3) atomicAdd(&mine[kOff3 + (w & 0x3fu)], 1u);
        else atomicAdd(&mine[kOff2 + (w & 0xfu)], 1u);
      }
    }
  }
  __syncthreads();
  // the copies into copy 0
  for (uint32_t b = tid; b < (uint32_t)kBins; b += kThreads) {
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < kCopies; ++c) s += hist[c * kCopyStride + b];
    hist[b] = s;  // bin b of copy 0 is read by this lane alone in this loop
  }
  __syncthreads();
  // F3 in packed order: the 4-words with prefix j are j | d << 6 (kDirect: counted, nothing to derive)
  if (tid < 64) f3[tid] = hist[kOff3 + tid] + (kDirect ? 0u : hist[tid] + hist[tid | 64u] + hist[tid | 128u] + hist[tid | 192u]);
  __syncthreads();
  unsigned long long *const row = counts + (uint64_t)g * kBins;
  {
    const uint32_t v = hist[tid];  // kThreads == 256 tetranucleotides
    if (v) atomicAdd(&row[rev_digits(tid, 4)], (unsigned long long)v);
  }
  if (tid < 64) {
    const uint32_t v = f3[tid];
    if (v) atomicAdd(&row[kOff3 + rev_digits(tid, 3)], (unsigned long long)v);
  } else if (tid < 80) {
    const uint32_t j = tid - 64;
    const uint32_t v = hist[kOff2 + j] + (kDirect ? 0u : f3[j] + f3[j | 16u] + f3[j | 32u] + f3[j | 48u]);
    if (v) atomicAdd(&row[kOff2 + rev_digits(j, 2)], (unsigned long long)v);
  }
}
static_assert(kThreads == 256, "the flush takes one tetranucleotide per lane");
static_assert(kBins == 336, "256 tetra-, 64 tri- and 16 dinucleotides");

// ---- correlations -----------------------------------------------------------------------------------------------------
constexpr int kTile = 64;              // rows of queries and of subjects per workgroup: the launch grid's step
constexpr int kCols = PA_TETRA_WORDS;  // 256 columns per row
static_assert(kTile == pairs_f64::kTile && kThreads == pairs_f64::kThreads, "the correlation kernel is launched with the skeleton's tile and workgroup");

struct DotTerm {
  static __device__ __forceinline__ double add(double acc, double a, double b) {
    const double p = a * b;  // rounded here: contraction is off for this file
    return acc + p;
  }
};

__device__ __forceinline__ double finish_r(double acc, bool same) {
  if (acc != acc) return acc;  // a degenerate genome: NaN (min and max would drop it)
  if (same) return 1.0;
  return acc > 1.0 ? 1.0 : (acc < -1.0 ? -1.0 : acc);
}

// out is [q1 - q0][s1 - s0].  symmetric (q0 == s0, q1 == s1): the tiles below the diagonal return at once and the tiles
// above it write their mirror image too -- the same bits, as a * b is b * a term by term
__global__ __launch_bounds__(kThreads, 4) void tetra_corr_kernel(const double *__restrict__ u, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1,
                                                              int symmetric, double *__restrict__ out) {
  const uint32_t tj = blockIdx.x, ti = blockIdx.y;
  if (symmetric && tj < ti) return;
  const uint32_t i0 = q0 + ti * kTile, j0 = s0 + tj * kTile;
  const uint32_t ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  double acc[4][4];
  pairs_f64::pair_tile_accumulate<kCols, DotTerm>(u, kCols, i0, q1, j0, s1, ty, tx, acc);

  const uint64_t ns = s1 - s0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const uint32_t i = i0 + 4 * ty + a;
    if (i >= q1) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t j = j0 + 4 * tx + b;
      if (j >= s1) continue;
      const double r = finish_r(acc[a][b], i == j);
      out[(uint64_t)(i - q0) * ns + (j - s0)] = r;
      if (symmetric && tj > ti) out[(uint64_t)(j - q0) * ns + (i - s0)] = r;  // square: j is a row and i a column as well
    }
  }
}

}  // namespace

extern "C" int pa_tetra_counts(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty, uint64_t arena_bases,
                               const uint64_t *h_genome_start, uint32_t n_genomes, uint64_t *d_counts) {
  PA_REQUIRE(c != nullptr && h_genome_start != nullptr, "pa_tetra_counts: null argument");
  PA_REQUIRE((arena_bases % PA_ALIGN_BASES) == 0, "pa_tetra_counts: arena_bases %llu is not a multiple of %u", (unsigned long long)arena_bases,
             PA_ALIGN_BASES);
  PA_REQUIRE(h_genome_start[n_genomes] == arena_bases, "pa_tetra_counts: genome_start[n] must equal arena_bases");
  const uint64_t n_blocks = arena_bases / PA_ALIGN_BASES;
  PA_REQUIRE(n_blocks < (1ULL << 32), "pa_tetra_counts: arena too large: %llu blocks of 64 bases", (unsigned long long)n_blocks);
  if (n_genomes == 0) return PA_OK;
  PA_REQUIRE(d_counts != nullptr && (arena_bases == 0 || (d_packed != nullptr && d_mask != nullptr)), "pa_tetra_counts: null argument");
  // genome g: blocks [tab[g], tab[g + 1]) and chunks [tab[n + 1 + g], tab[n + 1 + g + 1])
  std::vector<uint32_t> tab(2 * ((size_t)n_genomes + 1));
  uint32_t *const blk = tab.data(), *const chunk_off = tab.data() + n_genomes + 1;
  uint64_t n_chunks = 0;
  for (uint32_t g = 0; g <= n_genomes; ++g) {
    const uint64_t s = h_genome_start[g];
    PA_REQUIRE((s % PA_ALIGN_BASES) == 0 && (g == 0 || s >= h_genome_start[g - 1]) && s <= arena_bases,
               "pa_tetra_counts: genome_start[%u]=%llu must be an ascending multiple of %u inside the arena", g, (unsigned long long)s,
               PA_ALIGN_BASES);
    blk[g] = (uint32_t)(s / PA_ALIGN_BASES);
    chunk_off[g] = (uint32_t)n_chunks;
    if (g < n_genomes) n_chunks += ceil_div((h_genome_start[g + 1] - s) / PA_ALIGN_BASES, kChunkBlocks);
  }
  PA_HIP(hipSetDevice(c->device));
  PA_HIP(hipMemsetAsync(d_counts, 0, (uint64_t)n_genomes * kBins * sizeof(uint64_t), c->stream));
  if (n_chunks == 0) return PA_OK;
  const uint64_t *dirty = nullptr;
  PA_TRY(pa_dirty_or_build(c, d_mask, n_blocks, d_dirty, &dirty));
  PA_TRY(c->tetra_tab.reserve(tab.size() * sizeof(uint32_t)));
  PA_HIP(hipMemcpyAsync(c->tetra_tab.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  const uint32_t *d_tab = c->tetra_tab.as<uint32_t>();
  const char *direct = PA_TOOL_ENV("PA_TETRA_DIRECT");  // the measurement's other form, read per call
  auto launch = [&](auto kernel, const char *name) {
    return pa_launch(c, name, kernel, false, n_chunks, kThreads, 0, nullptr, reinterpret_cast<const uint4 *>(d_packed),
                     reinterpret_cast<const uint2 *>(d_mask), dirty, d_tab, d_tab + n_genomes + 1, n_genomes,
                     reinterpret_cast<unsigned long long *>(d_counts));
  };
  const int status = direct && direct[0] == '1' ? launch(tetra_counts_kernel<true>, "tetra_counts_kernel<direct>")
                                                : launch(tetra_counts_kernel<false>, "tetra_counts_kernel");
  PA_HIP(hipStreamSynchronize(c->stream));  // the upload reads `tab`
  return status;
}

extern "C" int pa_tetra_corr(pa_ctx *c, const double *d_U, uint32_t n, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, int symmetric,
                             double *d_out) {
  PA_REQUIRE(c != nullptr, "pa_tetra_corr: null context");
  PA_REQUIRE(q0 <= q1 && q1 <= n && s0 <= s1 && s1 <= n, "pa_tetra_corr: ranges [%u, %u) x [%u, %u) outside the %u genomes", q0, q1, s0, s1, n);
  PA_REQUIRE(!symmetric || (q0 == s0 && q1 == s1), "pa_tetra_corr: symmetric needs the same query and subject range, not [%u, %u) x [%u, %u)", q0,
             q1, s0, s1);
  if (q0 == q1 || s0 == s1) return PA_OK;
  PA_REQUIRE(d_U != nullptr && d_out != nullptr, "pa_tetra_corr: null argument");
  PA_HIP(hipSetDevice(c->device));
  return PA_LAUNCH(c, tetra_corr_kernel, LaunchDim(ceil_div(s1 - s0, kTile), ceil_div(q1 - q0, kTile)), kThreads, 0, d_U, q0, q1, s0, s1,
                   symmetric ? 1 : 0, d_out);
}
