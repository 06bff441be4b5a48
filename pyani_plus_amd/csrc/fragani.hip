// fragani.hip -- fastANI-style fragment-mapping ANI on gfx950 (BASELINE configs[3]).
//
// Replaces one `fastANI --ql queries -r subject --fragLen F -k K --minFraction M` process per
// subject column (pyani_plus/private_cli.py:1044-1063) by an all-vs-all device pipeline.  The
// algorithm is the restatement pinned in oracle/fragani_oracle.c (published fastANI / Mashmap
// method; it reproduces the reference's 25 fixture rows and test pins exactly); every number this
// file produces (minimizers, per-fragment shared counts, kept fragments, the float sums of the
// identities) equals the oracle's.
//
//   1. minimizer_kernel   both-strand 32-bit murmur of every K-mer (first multiply by LDS table,
//                         as in kmer_hash.hip), winnowing minimum over w positions from an LDS tile,
//                         ordered compaction -> minimizers (hash, window id, contig) per contig
//   2. radix sort by hash -> dense hash ids, postings, "same hash earlier in this contig" links
//   3. query_sketch_kernel a fragment's sketch is a SLICE of its genome's minimizers (window ids
//                         inside the fragment + the one still active at the first window at which the
//                         fragment, sketched alone as fastANI does it, selects any): sort, de-duplicate
//                         in LDS, no re-hashing
//   4. seed hits           every posting of every sketch hash -> (rank of the hash in the sketch, ref contig, window id),
//                         bucketed by reference genome (one fragment per workgroup, the listed pairs' hits
//                         staged in LDS and written as whole slices); one wave per (fragment, reference
//                         genome) segment then orders its hits in registers, applies the L1 run test and
//                         slides the fragment over every candidate range: the winnowed-MinHash Jaccard
//                         of every window that could be the optimum (bit tables over query rank x
//                         reference position in LDS, no per-window sort; a tight bound from the hits' ranks
//                         and one hash comparison per stretch entry decides which windows that is); segments
//                         of at most eight hits take the hit-by-hit form (map_sparse_kernel); of equally
//                         good candidates the last
//   5. one best fragment per reference bin by atomicMax on (J, shared, s); per pair the kept
//      fragments and the float sum of their float identities in bin order (fastANI's arithmetic).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <optional>
#include <type_traits>
#include <vector>

#include "murmur_dev.h"
#include "pa_internal.h"
#include "wave_dev.h"

namespace {

using namespace pa_dev;

constexpr int kThreads = 256;
constexpr uint32_t kSkip = 0xffffffffu;
constexpr int kQMax = 512;       // largest fragment sketch handled
constexpr int kHitCapSmall = 256;  // segments up to this many hits run with the smaller LDS footprint
constexpr int kHitCap = 512;     // seed hits of one (fragment, reference genome) segment staged in LDS
constexpr double kPercIdentity = 80.0, kConfLevel = 0.9, kPvalCutoff = 1e-3, kRefSize = 5e6;
// Query genomes go through in batches of up to 2^17 fragments (13 batches for 1 000 genomes of 5 Mb: 1.46 s against
// 1.48 s with 2^16).  A batch whose seed hits do not fit 31-bit indices is halved and started again.
#ifndef PA_FRAGANI_BATCH_FRAGS
#define PA_FRAGANI_BATCH_FRAGS (1u << 17)
#endif
#ifndef PA_MAP_LDS_PAD
#define PA_MAP_LDS_PAD 0u  // (an experiment's switch: LDS asked for and not used, to see what a wave less per SIMD costs)
#endif

// ============================================================== host statistics (Mashmap)
double md2j(double d, int k) { return 1.0 / (2.0 * std::exp(k * d) - 1.0); }
double j2md(double j, int k) {
  if (j == 0) return 1.0;
  if (j == 1) return 0.0;
  return (-1.0 / k) * std::log(2.0 * j / (1.0 + j));
}
double binom_cdf(int x, int n, double p) {
  if (x < 0) return 0.0;
  if (x >= n) return 1.0;
  double sum = 0.0;
  const double lp = std::log(p), lq = std::log1p(-p);
  for (int i = 0; i <= x; ++i)
    sum += std::exp(std::lgamma(n + 1.0) - std::lgamma(i + 1.0) - std::lgamma(n - i + 1.0) + i * lp + (n - i) * lq);
  return sum > 1.0 ? 1.0 : sum;
}
int binom_quantile_upper(int n, double p, double q) {
  if (p <= 0.0) return 0;
  if (p >= 1.0) return n;
  for (int x = 0; x <= n; ++x)
    if (1.0 - binom_cdf(x, n, p) <= q) return x;
  return n;
}
double md_lower_bound(double d, int s, int k) {
  const int x = binom_quantile_upper(s, md2j(d, k), (1.0 - kConfLevel) / 2.0);
  return j2md((double)x / s, k);
}
bool upper_bound_passes(int shared, int s, int k) {
  const double d = j2md((double)shared / s, k);
  return 100.0 * (1.0 - md_lower_bound(d, s, k)) >= kPercIdentity;
}
int min_shared_for(int s, int k) {
  for (int x = 0; x <= s; ++x)
    if (upper_bound_passes(x, s, k)) return x;
  return s + 1;
}
int relaxed_min_hits(int s, int k) {
  int best = (int)std::ceil(1.0 * s * md2j(1.0 - kPercIdentity / 100.0, k));
  for (int i = best; i >= 0; --i) {
    if (upper_bound_passes(i, s, k)) best = i; else break;
  }
  return best;
}
// Winnowing window: the smallest sketch size of Mashmap's list 1, 2, 5, 10, 20, 30, ... whose random-match p-value
// over a 5 Mb reference is <= 1e-3, then w = 2*fragLen/sketch (24 for k=16, fragLen=3000: the window fastANI logs).
int window_size_for(int k, int frag_len) {
  auto passes = [&](int s) {
    const double px = 1.0 / (1.0 + std::pow(4.0, k) / frag_len);
    const double r = px * px / (px + px - px * px);
    const int x = relaxed_min_hits(s, k);
    const double comp = x == 0 ? 1.0 : 1.0 - binom_cdf(x - 1, s, r);
    return kRefSize * comp <= kPvalCutoff;
  };
  int s = 1;
  bool found = false;
  for (int cand : {1, 2, 5}) { s = cand; if ((found = passes(s))) break; }
  for (int cand = 10; cand < frag_len && !found; cand += 10) { s = cand; found = passes(s); }
  int w = (int)(2.0 * frag_len / s);
  if (w < 1) w = 1;
  if (w > frag_len) w = frag_len;
  return w;
}

// ============================================================== device helpers
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *__restrict__ v, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// first minimizer of contig c with window id >= x, through the per-contig bucket index
// (bucket b of a contig = window ids [b*256, b*256+256); bucket_first holds global minimizer indices and
// one closing entry per contig): two dependent loads plus a ~20-entry search instead of a 19-step
// binary search whose every probe misses the caches
constexpr uint32_t kBucketShift = 8;
__device__ __forceinline__ uint32_t wpos_lower_bound(const uint32_t *__restrict__ mini_wpos,
                                                     const uint32_t *__restrict__ bucket_first, uint32_t bucket_base,
                                                     uint32_t n_buckets, uint32_t x) {
  uint32_t b = x >> kBucketShift;
  if (b >= n_buckets) b = n_buckets;  // beyond the contig: the closing entry
  const uint32_t lo = bucket_first[bucket_base + b];
  const uint32_t hi = b < n_buckets ? bucket_first[bucket_base + b + 1] : lo;
  return lower_bound_u32(mini_wpos, lo, hi, x);
}

__device__ __forceinline__ uint32_t contig_of(const uint64_t *__restrict__ start, uint32_t n, uint64_t pos) {
  uint32_t lo = 0, hi = n;  // largest c with start[c] <= pos (start[0] == 0)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (start[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return pa_dev::wave_sum_dpp(v); }
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane) {
  (void)lane;
  return pa_dev::wave_incl_scan_dpp(v) - v;
}

// The kernels, in pipeline order (one translation unit: the files are included here, inside the anonymous namespace)
#include "fragani_rules.inc"   // the key of a seed hit; the rules of the mapping that its two kernels share
#include "fragani_index.inc"   // 1. minimizers, 2. dictionary of minimizer hashes, postings, frequency cut
#include "fragani_seed.inc"    // 3. fragment sketches, 4. seed hits bucketed by reference genome, segment lists
#include "fragani_map.inc"     // 4. (continued) map_segments_kernel: L1, the exact slide, bounds
#include "fragani_sparse.inc"  // 4b. map_sparse_kernel: segments of a handful of seed hits

// ============================================================== 5. per-pair reduction
// One wave per (query of the batch, reference genome): kept fragments and the sum of their identities.  fastANI holds the
// identities as floats and adds them up in a float, in (contig, bin) order; a float sum depends on its order, so the wave
// adds in exactly that order: 64 bins per load, then one addition per kept bin through a scalar loop over the wave.
__global__ __launch_bounds__(64) void reduce_pairs_kernel(const unsigned long long *__restrict__ table,
                                                          uint64_t table_stride,
                                                          const uint32_t *__restrict__ genome_bin_off,
                                                          uint32_t n_genomes, const float *__restrict__ ident_tab,
                                                          uint32_t *__restrict__ matched, double *__restrict__ ident_sum) {
  const uint32_t lane = threadIdx.x;
  const uint32_t q = blockIdx.x / n_genomes, r = blockIdx.x % n_genomes;
  const uint32_t b0 = genome_bin_off[r], b1 = genome_bin_off[r + 1];
  uint32_t cnt = 0;
  float sum = 0.0f;
  for (uint32_t base = b0; base < b1; base += 64) {
    const uint32_t bidx = base + lane;
    const unsigned long long v = bidx < b1 ? table[(uint64_t)q * table_stride + bidx] : 0ull;
    float id = 0.0f;
    if (v) {
      const uint32_t shared = (uint32_t)(v >> 16) & 0xffffu, s = (uint32_t)v & 0xffffu;
      id = ident_tab[(uint64_t)s * (kQMax + 1) + shared];
    }
    uint64_t kept = __ballot(v != 0ull);
    cnt += (uint32_t)__popcll(kept);
    while (kept) {
      const int l = __builtin_ctzll(kept);
      kept &= kept - 1;
      sum = __fadd_rn(sum, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, id), l)));
    }
  }
  if (lane == 0) {
    matched[(uint64_t)q * n_genomes + r] = cnt;
    ident_sum[(uint64_t)q * n_genomes + r] = (double)sum;
  }
}

// ============================================================== host driver
template <typename T>
int upload(pa_ctx *c, DevBuf &buf, const std::vector<T> &v) {
  PA_TRY(buf.reserve(v.size() * sizeof(T) + 16));
  if (!v.empty()) PA_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return PA_OK;
}

// The device buffers of the workspace, each named here and nowhere else: the members of FragWork, their share in its
// budget, their release after PA_E_NOMEM and in the destructor all follow from this list.  ONE(name): a buffer `name`;
// PAIR(name): two, `name[0]` and `name[1]`.
#define PA_FRAGWORK_BUFFERS(ONE, PAIR)                                                                                  \
  ONE(contig_start) ONE(contig_len) ONE(contig_genome) ONE(block_counts) ONE(block_offsets) ONE(mini_hash)             \
  ONE(mini_wpos) ONE(mini_contig) ONE(contig_mini_off) PAIR(keys) PAIR(vals) ONE(flags) ONE(mini_id) ONE(post_start)   \
  ONE(prev_same) ONE(frag_contig) ONE(frag_no) ONE(frag_genome_local) ONE(q_hash) ONE(q_pos) ONE(q_id) ONE(q_s)        \
  ONE(hit_count) ONE(hit_off) PAIR(hkeys) PAIR(hvals) ONE(seg_start) ONE(tab_min_hits) ONE(tab_min_shared)             \
  ONE(ident_tab) ONE(contig_bin_off) ONE(genome_bin_off) ONE(table) ONE(matched) ONE(ident_sum) ONE(scalars)           \
  ONE(run_g) ONE(seg_list) ONE(seg2_a0) ONE(seg2_nh) ONE(post_cw) ONE(seg_a0) ONE(seg_nh) ONE(genome_first_contig)     \
  ONE(contig_bucket_off) ONE(bucket_first) ONE(post_g) ONE(seg_rec) ONE(hash_cut) ONE(q_cut) ONE(post_cw2)             \
  ONE(post_g2) ONE(run_hist) ONE(long_runs) ONE(frag_d) ONE(uniq_hash) ONE(lookup_at) ONE(seg_f) ONE(seg2_f)           \
  ONE(amb_pos) ONE(amb_byte) ONE(seg_over) ONE(q_tab)

// The words of FragWork::scalars: the counters and cursors the kernels are handed, as ScalarSlots (pa_internal.h).  Every
// slot is zeroed by one hipMemsetAsync over exactly its own words (none covers two slots) and read back whole, both by
// the function named with it.
// run_minimizers: minimizer_kernel has the buffer to itself, all kMiniScalarBytes zeroed before every run: [0] ticket,
// [1] minimizers, [2] a wait ran out, [3] unused -- the four words read back -- and one ticket counter per XCD behind them
constexpr ScalarSlot kMiniScalars{0, kMiniScalarBytes / 4u}, kMiniResult{0, 4};
constexpr uint32_t kMiniTotalWord = 1, kMiniRanOutWord = 2;  // within kMiniResult
// From the dictionary on, the first 16 words (kBatchScalarBytes):
constexpr ScalarSlot kScanTotal{0, 2};       // every pa_exclusive_scan_u32: its 64-bit total (written, never zeroed)
constexpr ScalarSlot kSparseOver{3, 1};      // map_short_segments: segments map_sparse_kernel hands on to the general kernel
constexpr ScalarSlot kSegCounters{4, 4};     // bucket_pass: [1] segments that need a sort of their own, [2] the longest of them
constexpr ScalarSlot kSketchOverflow{8, 2};  // prepare_run, once per call: [0] fragment sketches cut at kQMax (read at the call's end)
constexpr ScalarSlot kBigCursor{10, 1};      // list_segments_bucketed: cursor of big_segments_kernel; kPreCursor's first word, done with before that
constexpr ScalarSlot kPreCursor{10, 2};      // map_short_segments: prefilter_segments_kernel's 64-bit word: [lo] general, [hi] sparse
constexpr ScalarSlot kMaxHits{12, 2};        // stage_batch: [0] most seed hits of one fragment, [1] the longest sketch (read by seed_batch)
constexpr ScalarSlot kSegCursor{14, 2};      // bucket_pass: one 64-bit word: [lo] short, [hi] long segments listed
constexpr uint32_t kBatchScalarBytes = 64;
static_assert(slots_apart(kBatchScalarBytes, {kScanTotal, kSparseOver, kSegCounters, kSketchOverflow, kPreCursor, kMaxHits, kSegCursor}) &&
                  slots_apart(kBatchScalarBytes, {kScanTotal, kSegCounters, kSketchOverflow, kBigCursor, kMaxHits, kSegCursor}) &&
                  kMiniResult.bytes() <= kMiniScalarBytes,
              "two slots of FragWork::scalars that are live at the same time overlap");

struct FragWork {
#define PA_ONE(name) DevBuf name;
#define PA_PAIR(name) DevBuf name[2];
  PA_FRAGWORK_BUFFERS(PA_ONE, PA_PAIR)
#undef PA_ONE
#undef PA_PAIR
  template <typename T = uint32_t>
  T *slot(ScalarSlot s) const { return reinterpret_cast<T *>(scalars.as<uint32_t>() + s.word); }
  // the arena's residues that are neither ACGT nor N (pa_fragani_set_ambiguous), and the arena they belong to
  const void *amb_for = nullptr;
  uint32_t amb_n = 0;
  std::vector<uint64_t> amb_host_pos;  // what the device arrays hold: a call that hands over the same list again changes nothing
  std::vector<uint8_t> amb_host_byte;
  AmbiguousList ambiguous(const void *d_packed) const {
    const bool mine = amb_n && amb_for == d_packed;
    return AmbiguousList{mine ? amb_pos.as<uint64_t>() : nullptr, mine ? amb_byte.as<uint8_t>() : nullptr, mine ? amb_n : 0u};
  }
  // the reference index (stages 1 and 2) of the last pa_fragani(_ex) call, for PA_FRAGANI_REUSE_INDEX
  bool index_valid = false;
  const void *index_packed = nullptr;
  uint64_t index_arena_bases = 0;
  uint32_t index_contigs = 0, index_genomes = 0, index_k = 0, index_frag_len = 0, index_m = 0, index_ids = 0;
  uint32_t index_ref0 = 0, index_ref1 = 0;  // the reference genomes whose minimizers the dictionary holds
  uint32_t index_lookup_bits = 10;          // log2 of the slots of the look-up table by hash value (such a dictionary only)
  uint32_t tables_k = 0;                    // the k the tables by sketch size (tab_min_hits, tab_min_shared, ident_tab) on the device were made for; 0: none
  uint64_t index_key_room = 0;              // keys of one half of the sort's key buffer (W.keys[0] holds both halves)
  int index_which = 0;
  // every buffer of the workspace shares one budget: what pa_fragani_workspace reports and pa_fragani_set_workspace_cap bounds
  DevBudget budget;
  template <class Fn>
  void each_buffer(Fn &&fn) {
#define PA_ONE(name) fn(name);
#define PA_PAIR(name) fn(name[0]); fn(name[1]);
    PA_FRAGWORK_BUFFERS(PA_ONE, PA_PAIR)
#undef PA_ONE
#undef PA_PAIR
  }
  FragWork() { each_buffer([this](DevBuf &b) { b.budget = &budget; }); }
  FragWork(const FragWork &) = delete;
  FragWork &operator=(const FragWork &) = delete;
  ~FragWork() { each_buffer([](DevBuf &b) { b.release(); }); }
};

// The workspace lives in the context like the sketch and pair workspaces do: buffers only grow, and a
// second call does not pay for returning tens of GB to the driver and asking for them again.
FragWork &frag_work(pa_ctx *c) {
  if (!c->frag_work) c->frag_work = new FragWork();
  return *static_cast<FragWork *>(c->frag_work);
}

// Mashmap's frequency cut (see posting_run_hist_kernel): thresholds per reference genome on the host, from the histograms
// of the run lengths; the runs at or above them leave the posting lists.  `heads`: 1 at the first posting of every hash,
// `ids_before`: the hashes before a posting's own (the scan of `heads`), `sorted_idx`: the postings' minimizers, `idx_spare`: m words; `scratch`: 2 m words,
// free at this point.
int cut_frequent_postings(pa_ctx *c, FragWork &W, const uint32_t *d_heads, const uint32_t *d_ids_before, uint32_t *d_sorted_idx,
                          uint32_t *d_idx_spare, uint32_t *scratch, uint32_t m,
                          uint32_t n_ids, const uint32_t *h_contig_genome, uint32_t n_contigs, uint32_t n_genomes) {
  uint32_t *scratch_a = scratch, *scratch_b = scratch + m;
  PA_TRY(W.hash_cut.reserve(((uint64_t)n_ids / 32 + 2) * 4));
  PA_HIP(hipMemsetAsync(W.hash_cut.p, 0, ((uint64_t)n_ids / 32 + 2) * 4, c->stream));
  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_NO_FREQ_CUT")) { if (atoi(v)) return PA_OK; }  // tools: the seeds as rounds 1-4 looked them up
  constexpr uint32_t kOverCap = 1u << 20;
  std::vector<uint32_t> threshold(n_genomes, 0xffffffffu);
  bool any = false;
  {
    const uint64_t hist_words = (uint64_t)n_genomes * kFreqBins + n_genomes + 1;  // histograms, duplicate counts, overflow cursor
    PA_TRY(W.run_hist.reserve(hist_words * 4));
    PA_TRY(W.long_runs.reserve((uint64_t)kOverCap * 8));
    uint32_t *d_hist = W.run_hist.as<uint32_t>(), *d_dups = d_hist + (uint64_t)n_genomes * kFreqBins, *d_over_n = d_dups + n_genomes;
    PA_HIP(hipMemsetAsync(d_hist, 0, hist_words * 4, c->stream));
    // the runs numbered: flags in scratch_a, runs before each posting in scratch_b, the runs' first postings in idx_spare
    // (m + 1 words: every buffer here was reserved with room to spare)
    const uint64_t gm0 = ceil_div(m, kThreads);
    PA_TRY(PA_LAUNCH(c, posting_run_flags_kernel, gm0, kThreads, 0, d_heads, W.post_g.as<uint16_t>(), m, scratch_a));
    PA_TRY(pa_exclusive_scan_u32(c, scratch_a, scratch_b, m, nullptr));
    PA_TRY(PA_LAUNCH(c, posting_run_starts_kernel, gm0, kThreads, 0, scratch_a, scratch_b, m, d_idx_spare));
    PA_TRY(PA_LAUNCH(c, posting_run_hist_kernel, gm0, kThreads, 0, scratch_a, scratch_b, d_idx_spare, W.post_g.as<uint16_t>(), m, d_hist, d_dups,
                     W.long_runs.as<uint2>(), kOverCap, d_over_n));
    std::vector<uint32_t> h((size_t)hist_words);
    PA_TRY(pa_copy_to_host(c, h.data(), d_hist, hist_words * 4));
    const uint32_t n_over = h[hist_words - 1];
    PA_REQUIRE(n_over <= kOverCap, "pa_fragani: %u (minimizer, genome) pairs with %u or more occurrences", n_over, kFreqBins - 1);
    std::vector<uint2> h_over(n_over);
    if (n_over) PA_TRY(pa_copy_to_host(c, h_over.data(), W.long_runs.p, (size_t)n_over * 8));
    // minimizers per genome: its contigs' shares of the minimizer array
    std::vector<uint32_t> cmo(n_contigs + 1);
    PA_TRY(pa_copy_to_host(c, cmo.data(), W.contig_mini_off.p, (size_t)(n_contigs + 1) * 4));
    std::vector<uint64_t> n_min(n_genomes, 0);
    for (uint32_t ci = 0; ci < n_contigs; ++ci) n_min[h_contig_genome[ci]] += cmo[ci + 1] - cmo[ci];
    std::vector<std::vector<uint32_t>> long_runs(n_genomes);
    for (const uint2 &e : h_over) long_runs[e.x].push_back(e.y);
    for (uint32_t g = 0; g < n_genomes; ++g) {
      const uint32_t *bars = h.data() + (uint64_t)g * kFreqBins;
      const uint64_t uniq = n_min[g] - h[(uint64_t)n_genomes * kFreqBins + g];
      const int64_t to_ignore = (int64_t)((float)uniq * 0.001f / 100);
      // the bars from the most frequent minimizers down: (count, distinct minimizers with that count)
      std::vector<std::pair<uint32_t, uint64_t>> top;
      std::sort(long_runs[g].begin(), long_runs[g].end(), std::greater<uint32_t>());
      for (uint32_t v : long_runs[g]) { if (!top.empty() && top.back().first == v) ++top.back().second; else top.push_back({v, 1}); }
      uint64_t repeated = long_runs[g].size();
      for (uint32_t cnt = kFreqBins - 2; cnt >= 2; --cnt) if (bars[cnt]) { top.push_back({cnt, bars[cnt]}); repeated += bars[cnt]; }
      if (uniq > repeated) top.push_back({1u, uniq - repeated});
      int64_t sum = 0;
      for (const auto &bar : top) {
        sum += (int64_t)bar.second;
        if (sum < to_ignore) threshold[g] = bar.first;
        else { if (sum == to_ignore) threshold[g] = bar.first; break; }
      }
      any = any || threshold[g] != 0xffffffffu;
    }
  }
  if (!any) return PA_OK;
  // take the runs out: flags, their prefix sums, the postings moved into the workspace's second pair of arrays (which then
  // change places with the first), the lists' bounds rewritten
  PA_TRY(upload(c, W.run_hist, threshold));  // (the histograms are on the host by now)
  PA_TRY(W.post_cw2.reserve((uint64_t)m * 8));
  PA_TRY(W.post_g2.reserve((uint64_t)m * 2 + 16));
  const uint64_t gm = ceil_div(m, kThreads);
  PA_TRY(PA_LAUNCH(c, posting_cut_flags_kernel, gm, kThreads, 0, d_heads, d_ids_before, scratch_b, d_idx_spare, W.post_g.as<uint16_t>(), m,
                   W.run_hist.as<uint32_t>(), scratch_a, W.hash_cut.as<uint32_t>()));
  PA_TRY(PA_LAUNCH(c, mark_cut_minimizers_kernel, gm, kThreads, 0, d_heads, d_ids_before, d_sorted_idx, m, W.hash_cut.as<uint32_t>(),
                   W.mini_id.as<uint32_t>()));
  uint64_t kept64 = 0;
  PA_TRY(pa_scan_total_u32(c, scratch_a, scratch_b, m, W.slot<uint64_t>(kScanTotal), &kept64));
  const uint32_t kept = (uint32_t)kept64;
  if (kept != m) {
    PA_TRY(PA_LAUNCH(c, posting_compact_kernel, gm, kThreads, 0, scratch_a, scratch_b, W.post_cw.as<uint64_t>(), W.post_g.as<uint16_t>(),
                     d_sorted_idx, m, W.post_cw2.as<uint64_t>(), W.post_g2.as<uint16_t>(), d_idx_spare));
    PA_TRY(PA_LAUNCH(c, posting_starts_kernel, ceil_div((uint64_t)n_ids + 1, kThreads), kThreads, 0, W.post_start.as<uint32_t>(), n_ids, scratch_b,
                     m, kept));
    std::swap(W.post_cw, W.post_cw2);
    std::swap(W.post_g, W.post_g2);
    // (the postings' minimizer indices -- what the path for more than 8 192 genomes reads -- go back where they are looked for)
    PA_HIP(hipMemcpyAsync(d_sorted_idx, d_idx_spare, (uint64_t)kept * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  return PA_OK;
}

template <int K>
int run_minimizers(pa_ctx *c, FragWork &W, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                   uint32_t n_contigs, int w, uint32_t *m_out, const std::function<void()> *meanwhile) {
  PA_REQUIRE(ceil_div(arena_bases, kOwn) < (1ULL << 32), "fragment ANI: an arena of %llu bases has too many tiles for the minimizer scan",
             (unsigned long long)arena_bases);
  const uint32_t blocks = (uint32_t)ceil_div(arena_bases, kOwn);
  PA_TRY(W.block_counts.reserve((uint64_t)blocks * 8));  // the look-back words of minimizer_kernel
  PA_TRY(W.scalars.reserve(kMiniScalars.bytes()));
  PA_TRY(W.block_offsets.reserve((uint64_t)blocks * 4 + 16));  // the contig of every tile's first position
  PA_TRY(PA_LAUNCH(c, tile_contig_kernel, ceil_div(blocks, kThreads), kThreads, 0, W.contig_start.as<uint64_t>(), n_contigs, blocks,
                   W.block_offsets.as<uint32_t>()));
  // expected density of winnowed minimizers is 2 / (w + 1); the arrays are sized a quarter above that and the run is
  // repeated with the exact size should a low-complexity data set need more
  uint64_t cap = (uint64_t)((double)arena_bases * 2.5 / (double)(w + 1)) + (1u << 20);
  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_MINIMIZER_ROOM")) cap = std::max<uint64_t>(1, strtoull(v, nullptr, 10));  // tests: force the repeat
  // tiles are drawn from one counter per XCD; from a single counter when a wait of the chained scan ran out under that
  // scheme (see the kernel) -- or when a tool asks for it
  uint32_t ticket_mode = 1;
  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_ONE_TICKET")) { if (atoi(v)) ticket_mode = 0; }
  for (int attempt = 0; attempt < 2; ++attempt) {
    PA_REQUIRE(cap < (1ULL << 31), "fragment ANI: room for %llu minimizers exceeds the 31-bit index space", (unsigned long long)cap);
    PA_TRY(W.mini_hash.reserve(cap * 4 + 16));
    PA_TRY(W.mini_wpos.reserve(cap * 4 + 16));
    PA_TRY(W.mini_contig.reserve(cap * 4 + 16));
    PA_HIP(hipMemsetAsync(W.block_counts.p, 0, (uint64_t)blocks * 8, c->stream));
    PA_HIP(hipMemsetAsync(W.slot(kMiniScalars), 0, kMiniScalars.bytes(), c->stream));
    PA_TRY(PA_LAUNCH(c, minimizer_kernel<K>, blocks, kMiniThreads, 0, d_packed, d_mask, arena_bases, W.contig_start.as<uint64_t>(),
                     W.contig_len.as<uint32_t>(), n_contigs, w, W.block_counts.as<unsigned long long>(), W.slot(kMiniScalars), (uint32_t)cap,
                     W.mini_hash.as<uint32_t>(), W.mini_wpos.as<uint32_t>(), W.mini_contig.as<uint32_t>(), blocks, W.ambiguous(d_packed), ticket_mode,
                     W.block_offsets.as<uint32_t>()));
    uint32_t h[kMiniResult.words];
    ReadBack rb(c);
    PA_TRY(rb.queue(W.slot(kMiniResult), h, kMiniResult.words));
    if (meanwhile && *meanwhile) {  // the caller's host-side bookkeeping, while the kernel runs (once)
      (*meanwhile)();
      meanwhile = nullptr;
    }
    PA_TRY(rb.wait());
    bool ran_out = h[kMiniRanOutWord] != 0;
    if (const char *v = PA_TOOL_ENV("PA_FRAGANI_TICKET_TIMEOUT")) { if (atoi(v) && ticket_mode != 0) ran_out = true; }  // tests: as if a wait had run out
    if (ran_out && ticket_mode != 0) {  // a wait ran out with the tiles drawn per XCD: once more, from one counter
      ticket_mode = 0;
      --attempt;
      continue;
    }
    PA_REQUIRE(h[kMiniRanOutWord] == 0, "fragment ANI: the minimizer scan gave up waiting for a tile (%u tiles)", blocks);
    const uint64_t m = h[kMiniTotalWord];
    if (m <= cap) {
      *m_out = (uint32_t)m;
      return PA_OK;
    }
    cap = m;
  }
  pa_set_error("fragment ANI: minimizer count changed between two runs over the same arena");
  return PA_E_HIP;
}

int dispatch_minimizers(pa_ctx *c, FragWork &W, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                        uint32_t n_contigs, uint32_t k, int w, uint32_t *m_out, const std::function<void()> *meanwhile = nullptr) {
  int status = PA_E_INVALID;
  if (!dispatch_value(k, value_list<8, 9>{}, [&](auto kk) { status = run_minimizers<kk()>(c, W, d_packed, d_mask, arena_bases, n_contigs, w, m_out, meanwhile); }))
    pa_set_error("fragment ANI: k=%u outside [8,16] (fastANI itself stops at 16)", k);
  return status;
}

int stage_contigs(pa_ctx *c, FragWork &W, const uint64_t *h_contig_start, const uint32_t *h_contig_len,
                  const uint32_t *h_contig_genome, uint32_t n_contigs, uint32_t n_genomes, uint64_t arena_bases) {
  PA_REQUIRE(n_contigs >= 1 && n_contigs < (1u << 20), "fragment ANI: %u contigs (supported: 1 .. 2^20-1)", n_contigs);
  std::vector<uint64_t> cs(h_contig_start, h_contig_start + n_contigs);
  std::vector<uint32_t> cl(h_contig_len, h_contig_len + n_contigs), cg(h_contig_genome, h_contig_genome + n_contigs);
  for (uint32_t i = 0; i < n_contigs; ++i) {
    PA_REQUIRE(cs[i] + cl[i] <= arena_bases && (i == 0 || cs[i] >= cs[i - 1] + cl[i - 1]) && cg[i] < n_genomes &&
                   (i == 0 || cg[i] >= cg[i - 1]) && cl[i] < (1u << 24),
               "fragment ANI: contig %u is out of order, outside the arena, or longer than 2^24", i);
  }
  cs[0] = 0;  // positions before the first contig (none in practice) resolve to contig 0
  PA_TRY(upload(c, W.contig_start, cs));
  PA_TRY(upload(c, W.contig_len, cl));
  PA_TRY(upload(c, W.contig_genome, cg));
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}

// ============================================================== the stages of one pa_fragani_ex call
// fragani_ex_impl (at the end) reads as the pipeline; every stage below is a plain function over the context, the
// workspace and these few structs.

// The call: its arguments as handed in and, from check_call, what follows from them alone.
struct FragCall {
  const uint32_t *d_packed, *d_mask;
  uint64_t arena_bases;
  const uint64_t *h_contig_start;
  const uint32_t *h_contig_len, *h_contig_genome;
  uint32_t n_contigs, n_genomes, k, frag_len, qry0, qry1, ref0, ref1, flags;
  uint32_t *h_total_frags, *h_matched;
  double *h_ident_sum;
  int w = 0;                            // winnowing window
  uint32_t count_windows = 0;           // windows of one fragment
  uint32_t out_cols = 0, out_col0 = 0;  // the row length of the two result matrices on the host, and the first column they hold
  bool reuse = false;
};

// Fragments and reference bins (layout_fragments)
struct FragLayout {
  std::vector<uint32_t> frag_contig, frag_no, genome_frag_off, contig_bin_off, genome_bin_off;
};

// What every batch of the call shares (prepare_run)
struct FragRun {
  int which = 0;            // W.vals[which]: the postings' minimizers; W.vals[1 - which]: spare
  bool restricted = false;  // the dictionary holds a range of the genomes: hashes are looked up by value
  uint64_t range_bins = 1;  // bins of the reference genomes asked for
  uint64_t hit_limit = 1ULL << 31;
  uint32_t ref_cap = 0;     // stretch capacity of the mapping kernel
  bool use_buckets = false, trace = false;
};

// One batch of query genomes [g0, g1): fragments [f0, f0 + nf)
struct FragBatch {
  uint32_t g0 = 0, g1 = 0, f0 = 0, nf = 0, nq = 0;
  uint32_t *q_hash = nullptr, *q_pos = nullptr, *q_id = nullptr;  // the fragments' sketches
  uint64_t n_hits = 0;
  uint32_t max_hits = 0, s_cap = 0;  // most seed hits of one fragment; the longest sketch, in steps of 64
  unsigned long long *table = nullptr;  // best fragment per (query genome, reference bin)
};

// The batch's seed hits and its (fragment, reference genome) segments, as either way of listing them leaves them:
// hits in hk[hw] / hv[hw]; segments [0, n_keep) of seg_a0 / seg_nh (/ seg_f) and, bucketed, n_large long ones from large_at.
struct SegLists {
  uint64_t *hk[2] = {nullptr, nullptr};
  uint32_t *hv[2] = {nullptr, nullptr};
  int hw = 0;
  bool presorted = true;
  uint32_t n_keep = 0, n_large = 0, large_at = 0;
};

int check_call(pa_ctx *c, FragCall &a) {
  PA_REQUIRE(c && a.d_packed && a.d_mask && a.h_total_frags && a.h_matched && a.h_ident_sum, "pa_fragani: null argument");
  PA_REQUIRE(a.ref0 <= a.ref1 && a.ref1 <= a.n_genomes, "pa_fragani: reference range [%u,%u) outside [0,%u)", a.ref0, a.ref1, a.n_genomes);
  PA_REQUIRE(a.qry0 <= a.qry1 && a.qry1 <= a.n_genomes, "pa_fragani: query range [%u,%u) outside [0,%u)", a.qry0, a.qry1, a.n_genomes);
  PA_REQUIRE(a.n_genomes <= 0xffffu, "pa_fragani: %u genomes (limit 65 535: a posting names its genome in 16 bits)", a.n_genomes);
  PA_REQUIRE((a.flags & ~(uint32_t)(PA_FRAGANI_REUSE_INDEX | PA_FRAGANI_COLUMNS_ONLY)) == 0, "pa_fragani: unknown flags 0x%x", a.flags);
  a.out_cols = (a.flags & PA_FRAGANI_COLUMNS_ONLY) ? a.ref1 - a.ref0 : a.n_genomes;
  a.out_col0 = (a.flags & PA_FRAGANI_COLUMNS_ONLY) ? a.ref0 : 0u;
  a.reuse = (a.flags & PA_FRAGANI_REUSE_INDEX) != 0;
  PA_REQUIRE(a.frag_len >= 100 && a.frag_len <= 0xffffu, "pa_fragani: fragLen %u outside [100, 65535]", a.frag_len);
  PA_HIP(hipSetDevice(c->device));
  a.w = window_size_for((int)a.k, (int)a.frag_len);
  PA_REQUIRE(a.w >= 1 && a.w <= 64, "pa_fragani: winnowing window %d outside [1,64] for k=%u fragLen=%u", a.w, a.k, a.frag_len);
  PA_REQUIRE((int)a.frag_len > a.w + (int)a.k, "pa_fragani: fragLen %u too short for window %d", a.frag_len, a.w);
  a.count_windows = a.frag_len - (uint32_t)(a.w - 1) - (a.k - 1);
  FragWork &W = frag_work(c);
  snprintf(W.budget.what, sizeof(W.budget.what), "pa_fragani: %u genomes (%llu residues of arena), queries [%u,%u), reference range [%u,%u), fragLen %u",
           a.n_genomes, (unsigned long long)a.arena_bases, a.qry0, a.qry1, a.ref0, a.ref1, a.frag_len);
  return PA_OK;
}

// PA_FRAGANI_REUSE_INDEX: the index the workspace holds is this call's.  `*no_fragments`: no contig holds a fragment, so
// every pair is 0 of 0, whatever index an earlier call left (or did not leave) behind -- the results are written here.
int check_reuse(const FragWork &W, const FragCall &a, bool *no_fragments) {
  uint64_t any_frags = 0;
  for (uint32_t ci = 0; ci < a.n_contigs; ++ci) any_frags += a.h_contig_len[ci] / a.frag_len;
  *no_fragments = any_frags == 0;
  if (*no_fragments) {
    for (uint32_t g = 0; g < a.n_genomes; ++g) a.h_total_frags[g] = 0;
    for (uint64_t i = (uint64_t)a.qry0 * a.out_cols; i < (uint64_t)a.qry1 * a.out_cols; ++i) { a.h_matched[i] = 0; a.h_ident_sum[i] = 0.0; }
    return PA_OK;
  }
  PA_REQUIRE(W.index_valid && W.index_packed == (const void *)a.d_packed && W.index_arena_bases == a.arena_bases &&
                 W.index_contigs == a.n_contigs && W.index_genomes == a.n_genomes && W.index_k == a.k && W.index_frag_len == a.frag_len &&
                 W.index_ref0 <= a.ref0 && a.ref1 <= W.index_ref1,
             "pa_fragani: PA_FRAGANI_REUSE_INDEX without a preceding call on the same arena, contigs, k and fragLen whose "
             "reference range holds this one");
  return PA_OK;
}

// Fragments and reference bins, and the caller's rows zeroed (host bookkeeping: some 10 ms for the 1.7 million fragments
// and the two result matrices of 1 000 genomes -- on a fresh index done while minimizer_kernel runs, not before or after
// it with the device idle)
void layout_fragments(const FragCall &a, FragLayout &L) {
  L.genome_frag_off.assign(a.n_genomes + 1, 0);
  L.contig_bin_off.assign(a.n_contigs + 1, 0);
  L.genome_bin_off.assign(a.n_genomes + 1, 0);
  for (uint32_t g = 0; g < a.n_genomes; ++g) a.h_total_frags[g] = 0;
  uint64_t all_frags = 0;
  for (uint32_t ci = 0; ci < a.n_contigs; ++ci) all_frags += a.h_contig_len[ci] / a.frag_len;
  L.frag_contig.resize(all_frags);
  L.frag_no.resize(all_frags);
  uint64_t at = 0;
  for (uint32_t ci = 0; ci < a.n_contigs; ++ci) {
    const uint32_t nf = a.h_contig_len[ci] / a.frag_len;
    for (uint32_t f = 0; f < nf; ++f) { L.frag_contig[at + f] = ci; L.frag_no[at + f] = f; }
    at += nf;
    a.h_total_frags[a.h_contig_genome[ci]] += nf;
    L.contig_bin_off[ci + 1] = L.contig_bin_off[ci] + a.h_contig_len[ci] / (a.frag_len - 20u) + 2;
  }
  for (uint32_t g = 0; g < a.n_genomes; ++g) L.genome_frag_off[g + 1] = L.genome_frag_off[g] + a.h_total_frags[g];
  uint32_t ci = 0;
  for (uint32_t g = 0; g < a.n_genomes; ++g) {
    L.genome_bin_off[g] = L.contig_bin_off[ci];
    while (ci < a.n_contigs && a.h_contig_genome[ci] == g) ++ci;
  }
  L.genome_bin_off[a.n_genomes] = L.contig_bin_off[a.n_contigs];
  memset(a.h_matched + (uint64_t)a.qry0 * a.out_cols, 0, (uint64_t)(a.qry1 - a.qry0) * a.out_cols * sizeof(uint32_t));
  for (uint64_t i = (uint64_t)a.qry0 * a.out_cols; i < (uint64_t)a.qry1 * a.out_cols; ++i) a.h_ident_sum[i] = 0.0;
}

// ---- 1. minimizers of every contig (the fragment layout made meanwhile), their offsets per contig, the per-contig
// bucket index over window ids
int build_minimizers(pa_ctx *c, FragWork &W, const FragCall &a, FragLayout &L, uint32_t *m_out) {
  const std::function<void()> meanwhile = [&a, &L]() { layout_fragments(a, L); };
  uint32_t m = 0;
  PA_TRY(dispatch_minimizers(c, W, a.d_packed, a.d_mask, a.arena_bases, a.n_contigs, a.k, a.w, &m, &meanwhile));
  PA_TRY(W.contig_mini_off.reserve((uint64_t)(a.n_contigs + 2) * 4));
  PA_TRY(PA_LAUNCH(c, contig_offsets_kernel, ceil_div(a.n_contigs + 1, kThreads), kThreads, 0, W.mini_contig.as<uint32_t>(), m, a.n_contigs,
                   W.contig_mini_off.as<uint32_t>()));
  std::vector<uint32_t> cbo(a.n_contigs + 1, 0);
  for (uint32_t ci = 0; ci < a.n_contigs; ++ci) cbo[ci + 1] = cbo[ci] + (a.h_contig_len[ci] >> kBucketShift) + 2;
  PA_REQUIRE((uint64_t)cbo[a.n_contigs] < (1ULL << 31), "pa_fragani: bucket index too large");
  PA_TRY(upload(c, W.contig_bucket_off, cbo));
  PA_HIP(hipStreamSynchronize(c->stream));
  PA_TRY(W.bucket_first.reserve((uint64_t)cbo[a.n_contigs] * 4 + 16));
  PA_TRY(PA_LAUNCH(c, bucket_index_kernel, ceil_div(cbo[a.n_contigs], kThreads), kThreads, 0, W.mini_wpos.as<uint32_t>(),
                   W.contig_mini_off.as<uint32_t>(), W.contig_bucket_off.as<uint32_t>(), a.n_contigs, cbo[a.n_contigs], W.bucket_first.as<uint32_t>()));
  *m_out = m;
  return PA_OK;
}

// ---- 2. dictionary of minimizer hashes: ids, postings, same-hash links, frequency cut, look-up table
// The dictionary holds the minimizers of the REFERENCE genomes asked for (a worker asked for one subject column sorts
// and lists one genome's minimizers, and its seed-hit arrays are that small too); the query genomes' minimizers find
// their hashes in it by value.  With every genome a reference the minimizers know their hash ids themselves.
// `*which_out`: which of W.vals holds the postings' minimizers.
int build_dictionary(pa_ctx *c, FragWork &W, const FragCall &a, uint32_t m, int *which_out) {
  const bool restricted = !(a.ref0 == 0 && a.ref1 == a.n_genomes);
  uint32_t m_lo = 0, m_hi = m;
  if (restricted) {
    uint32_t c_lo = 0, c_hi = a.n_contigs;  // the contigs of the reference range (contigs are listed genome by genome)
    while (c_lo < a.n_contigs && a.h_contig_genome[c_lo] < a.ref0) ++c_lo;
    c_hi = c_lo;
    while (c_hi < a.n_contigs && a.h_contig_genome[c_hi] < a.ref1) ++c_hi;
    PA_TRY(pa_copy_to_host(c, &m_lo, W.contig_mini_off.as<uint32_t>() + c_lo, 4));
    PA_TRY(pa_copy_to_host(c, &m_hi, W.contig_mini_off.as<uint32_t>() + c_hi, 4));
  }
  const uint32_t md = m_hi - m_lo;  // minimizers in the dictionary
  const uint64_t md_room = std::max<uint32_t>(md, 1u);
  // (the two key buffers of the sort are the halves of ONE allocation: once the index stands they are free, and the seed
  // hits of the batches, 8 bytes each, go there -- memory this process has touched already instead of fresh pages)
  uint64_t *keys[2];
  PA_TRY(pa_carve(W.keys[0], "fragani keys", [&](Carve &k) { keys[0] = k.take<uint64_t>(md_room); keys[1] = k.take<uint64_t>(md_room); }));
  for (int b = 0; b < 2; ++b) PA_TRY(W.vals[b].reserve(md_room * 4));
  PA_TRY(W.flags.reserve(md_room * 8 + 64));
  W.index_key_room = md_room;
  PA_TRY(W.mini_id.reserve((uint64_t)m * 4));
  PA_TRY(W.prev_same.reserve((uint64_t)m * 4));
  PA_TRY(W.post_cw.reserve(md_room * 8));
  PA_TRY(W.post_g.reserve(md_room * 2 + 16));
  uint32_t *vals[2] = {W.vals[0].as<uint32_t>(), W.vals[1].as<uint32_t>()};
  int which = 0;
  PA_HIP(hipMemsetAsync(W.prev_same.p, 0xff, (uint64_t)m * 4, c->stream));  // -1: no earlier occurrence
  uint32_t n_ids = 0;
  if (md) {
    const uint64_t gm = ceil_div(md, kThreads);
    PA_TRY(PA_LAUNCH(c, mini_keys_kernel, gm, kThreads, 0, W.mini_hash.as<uint32_t>(), W.mini_wpos.as<uint32_t>(), m_lo, md, keys[0], vals[0]));
    PA_TRY(pa_radix_sort_pairs(c, keys, vals, md, 0, 32, false, &which));
    uint32_t *d_flags = W.flags.as<uint32_t>(), *d_pos = d_flags + md;
    PA_TRY(PA_LAUNCH(c, key_heads_kernel, gm, kThreads, 0, keys[which], md, d_flags));
    uint64_t n_ids64 = 0;
    PA_TRY(pa_scan_total_u32(c, d_flags, d_pos, md, W.slot<uint64_t>(kScanTotal), &n_ids64));
    n_ids = (uint32_t)n_ids64;
    PA_REQUIRE(n_ids < (1u << 31), "pa_fragani: %u distinct minimizer hashes (limit 2^31)", n_ids);
    PA_TRY(W.post_start.reserve((uint64_t)(n_ids + 2) * 4));
    PA_TRY(W.uniq_hash.reserve((uint64_t)(n_ids + 2) * 4));
    // (the contig of every block of minimizers: the look-back words of minimizer_kernel are free again)
    const uint32_t n_blocks = (uint32_t)(((uint64_t)m + (1u << kContigBlockShift) - 1u) >> kContigBlockShift);
    PA_TRY(W.block_counts.reserve((uint64_t)n_blocks * 4 + 16));
    PA_TRY(PA_LAUNCH(c, block_contig_kernel, ceil_div(n_blocks, kThreads), kThreads, 0, W.mini_contig.as<uint32_t>(), m, W.block_counts.as<uint32_t>()));
    PA_TRY(PA_LAUNCH(c, postings_kernel, gm, kThreads, 0, keys[which], vals[which], d_flags, d_pos, md, n_ids, W.mini_contig.as<uint32_t>(),
                     W.mini_id.as<uint32_t>(), W.post_start.as<uint32_t>(), W.prev_same.as<int32_t>(), W.mini_wpos.as<uint32_t>(),
                     W.contig_genome.as<uint32_t>(), W.post_cw.as<uint64_t>(), W.post_g.as<uint16_t>(), W.contig_mini_off.as<uint32_t>(), a.n_contigs,
                     W.uniq_hash.as<uint32_t>(), W.block_counts.as<uint32_t>()));
    PA_TRY(cut_frequent_postings(c, W, d_flags, d_pos, vals[which], vals[1 - which], reinterpret_cast<uint32_t *>(keys[1 - which]), md, n_ids,
                                 a.h_contig_genome, a.n_contigs, a.n_genomes));
  } else {  // the reference genomes hold no minimizer: an empty dictionary
    PA_TRY(W.post_start.reserve(16));
    PA_TRY(W.uniq_hash.reserve(16));
    PA_TRY(W.hash_cut.reserve(16));
    PA_HIP(hipMemsetAsync(W.post_start.p, 0, 8, c->stream));
    PA_HIP(hipMemsetAsync(W.hash_cut.p, 0, 8, c->stream));
  }
  W.index_ids = n_ids;
  if (restricted) {
    uint32_t bits = 10;
    while ((1ull << bits) < 2ull * n_ids + 1) ++bits;
    W.index_lookup_bits = bits;
    PA_TRY(W.lookup_at.reserve((16ull << bits) + 16));
    PA_HIP(hipMemsetAsync(W.lookup_at.p, 0xff, 16ull << bits, c->stream));
    PA_TRY(PA_LAUNCH(c, lookup_insert_kernel, ceil_div(n_ids, kThreads), kThreads, 0, W.uniq_hash.as<uint32_t>(), W.post_start.as<uint32_t>(),
                     W.hash_cut.as<uint32_t>(), n_ids, bits, W.lookup_at.as<uint4>()));
  }
  *which_out = which;
  return PA_OK;
}

// The index (minimizers, bucket index, dictionary, postings) is complete: a later call may take it over.  A call that
// took it over itself leaves the reference range the dictionary was built for as it is.
void remember_index(FragWork &W, const FragCall &a, uint32_t m, int which) {
  W.index_packed = a.d_packed; W.index_arena_bases = a.arena_bases; W.index_contigs = a.n_contigs; W.index_genomes = a.n_genomes;
  W.index_k = a.k; W.index_frag_len = a.frag_len; W.index_m = m; W.index_which = which;
  if (!a.reuse) { W.index_ref0 = a.ref0; W.index_ref1 = a.ref1; }
  W.index_valid = true;
}

// ---- what the batches share: the tables by sketch size, the bins of the reference range, each genome's first contig,
// which way the segments are listed
int prepare_run(pa_ctx *c, FragWork &W, const FragCall &a, const FragLayout &L, FragRun &R) {
  const uint32_t bin_base = L.genome_bin_off[a.ref0];
  R.range_bins = std::max<uint32_t>(L.genome_bin_off[a.ref1] - bin_base, 1u);
  // Mashmap's statistics per sketch size and the identity of every (shared, s): functions of k alone, ~10 ms of binomial
  // tails and logarithms on the host -- made once per context and k (the device copies stay where they are), not in
  // every call with the device waiting
  if (W.tables_k != a.k) {
    std::vector<uint32_t> mh(kQMax + 1), ms(kQMax + 1);
    PA_TRY(pa_fragani_tables(a.k, kQMax, mh.data(), ms.data()));
    std::vector<float> ident((uint64_t)(kQMax + 1) * (kQMax + 1), 0.0f);
    for (uint32_t s = 1; s <= (uint32_t)kQMax; ++s)
      for (uint32_t x = 0; x <= s; ++x) ident[(uint64_t)s * (kQMax + 1) + x] = (float)pa_fragani_identity(x, s, a.k);
    W.tables_k = 0;
    PA_TRY(upload(c, W.tab_min_hits, mh));
    PA_TRY(upload(c, W.tab_min_shared, ms));
    PA_TRY(upload(c, W.ident_tab, ident));
    PA_HIP(hipStreamSynchronize(c->stream));  // (the vectors go out of scope)
    W.tables_k = a.k;
  }
  // The table of best fragments per reference bin holds the bins of the reference range only (a worker asked for one
  // subject column keeps 1 700 bins per query genome instead of 1.7 million): bin numbers relative to the range's first;
  // genomes outside it get an empty run of bins, so the reduction gives them nothing, as an all-zero table did.
  std::vector<uint32_t> cbo_rel(L.contig_bin_off.size()), gbo_rel(L.genome_bin_off.size());
  for (size_t i = 0; i < L.contig_bin_off.size(); ++i) cbo_rel[i] = L.contig_bin_off[i] - std::min(L.contig_bin_off[i], bin_base);
  for (size_t g = 0; g < L.genome_bin_off.size(); ++g)
    gbo_rel[g] = std::min<uint32_t>(L.genome_bin_off[g] - std::min(L.genome_bin_off[g], bin_base), (uint32_t)R.range_bins);
  PA_TRY(upload(c, W.contig_bin_off, cbo_rel));
  PA_TRY(upload(c, W.genome_bin_off, gbo_rel));
  PA_HIP(hipStreamSynchronize(c->stream));

  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_BATCH_HITS")) R.hit_limit = std::max<uint64_t>(1, strtoull(v, nullptr, 10));  // tests: force the halving
  PA_TRY(W.scalars.reserve(kBatchScalarBytes));
  // The bucketed pipeline needs an LDS counter per reference genome for each of a workgroup's waves and
  // 16-bit fields for query window ids and for contigs within a genome; otherwise the sorted pipeline runs.
  std::vector<uint32_t> gfc(a.n_genomes + 1, a.n_contigs);
  uint32_t most_contigs = 0;
  for (uint32_t ci = a.n_contigs; ci-- > 0;) gfc[a.h_contig_genome[ci]] = ci;
  for (uint32_t g = a.n_genomes; g-- > 0;) if (gfc[g] == a.n_contigs) gfc[g] = gfc[g + 1];  // genome without contigs
  for (uint32_t g = 0; g < a.n_genomes; ++g) most_contigs = std::max(most_contigs, gfc[g + 1] - gfc[g]);
  bool genome_major = true;
  for (uint32_t ci = 1; ci < a.n_contigs; ++ci) genome_major = genome_major && a.h_contig_genome[ci] >= a.h_contig_genome[ci - 1];
  PA_REQUIRE(genome_major, "pa_fragani: contigs must be listed genome by genome");
  PA_TRY(upload(c, W.genome_first_contig, gfc));
  PA_HIP(hipStreamSynchronize(c->stream));
  R.trace = PA_TOOL_ENV("PA_FRAGANI_TRACE") != nullptr;  // per-batch sizes on stderr
  const char *hits_env = PA_TOOL_ENV("PA_FRAGANI_HITS");  // PA_FRAGANI_HITS=sorted: the path of more than 8 192 genomes, for any number (tests)
  const bool force_sorted = hits_env && hits_env[0] == 's';
  const bool fields_fit = a.count_windows <= 0xffffu && most_contigs <= 0xffffu;
  PA_REQUIRE(fields_fit, "pa_fragani: fragment length %u or %u contigs in one genome exceed the 16-bit fields of the "
                         "mapping kernel", a.frag_len, most_contigs);
  R.use_buckets = !force_sorted && (uint64_t)kBucketWaves * a.n_genomes * 4u <= 128u * 1024u;
  // stretch capacity: the expected minimizers of one window (density 2 / (w + 1)) plus a third, in steps of 64
  const uint32_t per_window = (uint32_t)(2.0 * a.count_windows / (a.w + 1.0));
  R.ref_cap = std::min<uint32_t>(kRefCapMax, std::max<uint32_t>(256u, (per_window * 4u / 3u + 63u) / 64u * 64u));
  PA_HIP(hipMemsetAsync(W.slot(kSketchOverflow), 0, kSketchOverflow.bytes(), c->stream));
  return PA_OK;
}

// ---- one batch
// The query genomes from g0 on whose fragments and whose table of best fragments fit a batch
int choose_batch(const FragCall &a, const FragLayout &L, const FragRun &R, uint32_t g0, uint32_t batch_frags, FragBatch &B) {
  const uint64_t kMaxTableBytes = 1ULL << 31;
  uint32_t g1 = g0 + 1;
  while (g1 < a.qry1 && L.genome_frag_off[g1 + 1] - L.genome_frag_off[g0] <= batch_frags &&
         (uint64_t)(g1 + 1 - g0) * R.range_bins * 8 <= kMaxTableBytes)
    ++g1;
  B.g0 = g0; B.g1 = g1; B.nq = g1 - g0;
  B.f0 = L.genome_frag_off[g0];
  B.nf = L.genome_frag_off[g1] - B.f0;
  PA_REQUIRE(B.nf < (1u << 20), "pa_fragani: genome %u alone has %u fragments (limit 2^20)", g0, B.nf);
  return PA_OK;
}

// The batch's fragments on the device, room for their sketches, the batch's counters zeroed
int stage_batch(pa_ctx *c, FragWork &W, const FragCall &a, const FragLayout &L, const FragRun &R, FragBatch &B) {
  const uint32_t f0 = B.f0, nf = B.nf;
  std::vector<uint32_t> fc(L.frag_contig.begin() + f0, L.frag_contig.begin() + f0 + nf),
      fn(L.frag_no.begin() + f0, L.frag_no.begin() + f0 + nf), fg(nf);
  for (uint32_t i = 0; i < nf; ++i) fg[i] = a.h_contig_genome[fc[i]] - B.g0;
  PA_TRY(upload(c, W.frag_contig, fc));
  PA_TRY(upload(c, W.frag_no, fn));
  PA_TRY(upload(c, W.frag_genome_local, fg));
  PA_HIP(hipStreamSynchronize(c->stream));
  // The batch's working arrays go into memory the index build has left behind wherever they fit (a fresh process pays
  // ~65 ms per GB for the FIRST use of device memory -- more than the kernels of a whole 1 000-genome run for the 6 GB
  // these are): the fragments' sketches into the sort's spare value buffer, the seed hits into its key buffers, the
  // table of best fragments into the flag / scan scratch.  (All three are dead once the index stands, also for a call
  // that takes the index over.)
  const uint64_t per = (uint64_t)nf * kQMax;
  DevBuf &spare = W.vals[1 - R.which];
  if (spare.bytes >= 3 * per * 4) {
    B.q_hash = spare.as<uint32_t>(); B.q_pos = B.q_hash + per; B.q_id = B.q_pos + per;
  } else {
    PA_TRY(W.q_hash.reserve(per * 4));
    PA_TRY(W.q_pos.reserve(per * 4));
    PA_TRY(W.q_id.reserve(per * 4));
    B.q_hash = W.q_hash.as<uint32_t>(); B.q_pos = W.q_pos.as<uint32_t>(); B.q_id = W.q_id.as<uint32_t>();
  }
  PA_TRY(W.q_s.reserve((uint64_t)nf * 4));
  PA_TRY(W.q_tab.reserve((uint64_t)nf * kQtBuckets * 2));  // the sketches' bucket tables
  PA_TRY(W.q_cut.reserve((uint64_t)nf * 4));
  PA_TRY(W.hit_count.reserve((uint64_t)nf * 4));
  PA_TRY(W.hit_off.reserve((uint64_t)nf * 4));
  PA_HIP(hipMemsetAsync(W.slot(kMaxHits), 0, kMaxHits.bytes(), c->stream));
  return PA_OK;
}

// ---- 3. the fragments' sketches and the number of seed hits of each
int seed_batch(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, FragBatch &B) {
  const uint32_t nf = B.nf;
  PA_TRY(W.frag_d.reserve((uint64_t)nf * 4));
  PA_TRY(PA_LAUNCH(c, windows_without_selection_kernel, ceil_div(nf, kThreads), kThreads, 0, a.d_packed, a.d_mask, a.arena_bases,
                   W.contig_start.as<uint64_t>(), a.k, (uint32_t)a.w, W.frag_contig.as<uint32_t>(), W.frag_no.as<uint32_t>(), nf, a.frag_len,
                   a.count_windows, W.frag_d.as<uint32_t>(), W.ambiguous(a.d_packed)));
  PA_TRY(PA_LAUNCH(c, query_sketch_kernel, ceil_div(nf, kThreads / 64), kThreads, 0, W.frag_d.as<uint32_t>(), W.frag_contig.as<uint32_t>(),
                   W.frag_no.as<uint32_t>(), nf, a.frag_len, a.count_windows, W.contig_mini_off.as<uint32_t>(), W.contig_bucket_off.as<uint32_t>(),
                   W.bucket_first.as<uint32_t>(), W.mini_hash.as<uint32_t>(), W.mini_wpos.as<uint32_t>(), W.mini_id.as<uint32_t>(),
                   W.post_start.as<uint32_t>(), B.q_hash, B.q_pos, B.q_id, W.q_s.as<uint32_t>(), W.hit_count.as<uint32_t>(),
                   W.slot(kSketchOverflow), W.slot(kMaxHits), W.q_cut.as<uint32_t>(), R.restricted ? W.lookup_at.as<uint4>() : nullptr,
                   W.index_lookup_bits, W.q_tab.as<uint32_t>()));
  PA_TRY(pa_exclusive_scan_u32(c, W.hit_count.as<uint32_t>(), W.hit_off.as<uint32_t>(), nf, W.slot<uint64_t>(kScanTotal)));
  uint32_t longest[kMaxHits.words];  // [0] most seed hits of one fragment, [1] the longest sketch
  ReadBack rb(c);
  PA_TRY(rb.queue(W.slot<uint64_t>(kScanTotal), &B.n_hits));
  PA_TRY(rb.queue(W.slot(kMaxHits), longest, kMaxHits.words));
  PA_TRY(rb.wait());
  B.max_hits = longest[0];
  B.s_cap = std::min<uint32_t>(kQMax, ((longest[1] + 63u) / 64u) * 64u);
  return PA_OK;
}

// The batch's table of best fragments, zeroed: in the index build's flag / scan scratch where it fits
int clear_table(pa_ctx *c, FragWork &W, const FragRun &R, FragBatch &B) {
  const uint64_t bytes = (uint64_t)B.nq * R.range_bins * 8;
  if (R.use_buckets && W.flags.bytes >= bytes) {
    B.table = W.flags.as<unsigned long long>();  // (the sorted path keeps its head flags there)
  } else {
    PA_TRY(W.table.reserve(bytes));
    B.table = W.table.as<unsigned long long>();
  }
  PA_HIP(hipMemsetAsync(B.table, 0, bytes, c->stream));
  return PA_OK;
}

// ---- 4. seed hits and their segments
// Room for the hits: in the sort's key buffers where they fit
int begin_hits(FragWork &W, const FragBatch &B, SegLists &S) {
  const bool hits_in_sort_keys = W.keys[0].bytes >= B.n_hits * 8;
  if (!hits_in_sort_keys) PA_TRY(W.hkeys[0].reserve(B.n_hits * 8));
  PA_TRY(W.hvals[0].reserve(B.n_hits * 4));  // (written by the paths that order the hits as a whole only)
  S.hk[0] = hits_in_sort_keys ? W.keys[0].as<uint64_t>() : W.hkeys[0].as<uint64_t>();
  S.hv[0] = W.hvals[0].as<uint32_t>();
  PA_TRY(W.run_g.reserve(256));  // the mapping kernel's event counters (-DPA_MAP_STATS)
  return PA_OK;
}
// The radix sort of a whole batch's hits (only it needs the ping-pong copies), over the key's 44 low bits and the fragment number above them
int sort_all_hits(pa_ctx *c, FragWork &W, const FragBatch &B, SegLists &S) {
  PA_TRY(W.hkeys[1].reserve(B.n_hits * 8));
  PA_TRY(W.hvals[1].reserve(B.n_hits * 4));
  S.hk[1] = W.hkeys[1].as<uint64_t>();
  S.hv[1] = W.hvals[1].as<uint32_t>();
  int bits = 44;
  for (uint32_t x = B.nf; x > 1; x >>= 1) ++bits;
  bits = (bits + 1 + 7) & ~7;
  if (bits > 64) bits = 64;
  return pa_radix_sort_pairs(c, S.hk, S.hv, B.n_hits, 0, bits, false, &S.hw);
}

// The launch shapes of the two bucketing kernels, and what a pass found
struct BucketPass {
  uint32_t seg_cap, lds_bytes, stage_cap, stage_lds;
  bool stage_hits;
  uint32_t n_big = 0, max_big = 0;  // segments too long for the register sort, the longest of them
};
int bucket_pass(pa_ctx *c, FragWork &W, const FragCall &a, const FragBatch &B, SegLists &S, BucketPass &P, bool write_all) {
  uint32_t *d_seg_counters = W.slot(kSegCounters);
  unsigned long long *d_cursor64 = W.slot<unsigned long long>(kSegCursor);
  PA_HIP(hipMemsetAsync(d_seg_counters, 0, kSegCounters.bytes(), c->stream));
  PA_HIP(hipMemsetAsync(d_cursor64, 0, kSegCursor.bytes(), c->stream));
  if (P.stage_hits && !write_all)
    PA_TRY(PA_LAUNCH_RAISE_LDS(c, bucket_hits_staged_kernel, B.nf, kStageWaves * 64, P.stage_lds, B.nf, B.q_pos, B.q_id, W.q_s.as<uint32_t>(),
                               W.hit_off.as<uint32_t>(), W.post_g.as<uint16_t>(), W.post_cw.as<uint64_t>(), a.n_genomes,
                               W.tab_min_hits.as<uint32_t>(), S.hk[0], W.seg_a0.as<uint32_t>(), W.seg_nh.as<uint32_t>(), W.seg_f.as<uint32_t>(),
                               P.seg_cap, d_seg_counters, d_cursor64, a.ref0, a.ref1, P.stage_cap));
  else
    PA_TRY(PA_LAUNCH_RAISE_LDS(c, bucket_hits_kernel, ceil_div(B.nf, kBucketWaves), kBucketWaves * 64, P.lds_bytes, B.nf, B.q_pos, B.q_id,
                               W.q_s.as<uint32_t>(), W.hit_off.as<uint32_t>(), W.post_g.as<uint16_t>(), W.post_cw.as<uint64_t>(), a.n_genomes,
                               W.tab_min_hits.as<uint32_t>(), S.hk[0], S.hv[0], W.seg_a0.as<uint32_t>(), W.seg_nh.as<uint32_t>(),
                               W.seg_f.as<uint32_t>(), P.seg_cap, d_seg_counters, d_cursor64, a.ref0, a.ref1, write_all));
  uint32_t hc32[kSegCounters.words];
  unsigned long long cursor64 = 0;
  ReadBack rb(c);
  PA_TRY(rb.queue(d_seg_counters, hc32, kSegCounters.words));
  PA_TRY(rb.queue(d_cursor64, &cursor64));
  PA_TRY(rb.wait());
  S.n_keep = (uint32_t)cursor64;
  S.n_large = (uint32_t)(cursor64 >> 32);
  S.large_at = P.seg_cap - S.n_large;
  P.n_big = hc32[1];
  P.max_big = hc32[2];
  PA_REQUIRE((uint64_t)S.n_keep + S.n_large <= P.seg_cap, "pa_fragani: %u + %u segments exceed the list capacity %u",
             S.n_keep, S.n_large, P.seg_cap);
  return PA_OK;
}

// hits bucketed by (fragment, reference genome); segments listed by the same kernel, the long ones at the end of the lists
int list_segments_bucketed(pa_ctx *c, FragWork &W, const FragCall &a, const FragBatch &B, SegLists &S) {
  PA_TRY(begin_hits(W, B, S));
  const uint32_t n_genomes = a.n_genomes;
  BucketPass P;
  const uint64_t seg_cap64 = std::min<uint64_t>(B.n_hits, (uint64_t)B.nf * n_genomes);
  P.seg_cap = (uint32_t)std::min<uint64_t>(seg_cap64, 0xfffffff0ull);
  PA_TRY(W.seg_a0.reserve((uint64_t)P.seg_cap * 4 + 16));
  PA_TRY(W.seg_nh.reserve((uint64_t)P.seg_cap * 4 + 16));
  PA_TRY(W.seg_f.reserve((uint64_t)P.seg_cap * 4 + 16));
  P.lds_bytes = (uint32_t)kBucketWaves * n_genomes * 4u;
  // one fragment per workgroup with the listed pairs' hits staged in LDS (whole-sector writes) when the two per-genome
  // arrays leave room for a staging area; the batch that is about to be ordered as a whole (write_all) keeps the
  // wave-per-fragment form, which writes every slot
  // (four workgroups of eight waves per CU: 40 KB of LDS each)
  const uint32_t lds_room = 40u * 1024u;
  P.stage_cap = n_genomes * 8u + 8192u <= lds_room ? ((lds_room - n_genomes * 8u) / 8u) & ~63u : 0u;
  P.stage_lds = P.stage_cap * 8u + n_genomes * 8u;
  P.stage_hits = P.stage_cap >= 1024u;
  PA_TRY(bucket_pass(c, W, a, B, S, P, false));
  S.presorted = false;
  uint32_t frag_sort_max = kFragSortMax;  // tests: PA_FRAGANI_SORT_MAX=600 sends a 60-copy repeat family down this path
  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_SORT_MAX")) frag_sort_max = (uint32_t)std::max(1, atoi(v));
  if (P.n_big && P.max_big > frag_sort_max) {
    // a repeat family with more hits than one LDS sort takes: order the whole batch by key; the
    // (fragment, genome) slices keep their places because contigs are numbered genome by genome -- provided every
    // slot holds its own key, so the bucketing runs again and this time also writes the hits of the pairs that are
    // not listed (they are skipped otherwise: unwritten slots would be sorted into other fragments' ranges)
    PA_TRY(bucket_pass(c, W, a, B, S, P, true));
    PA_TRY(sort_all_hits(c, W, B, S));
    S.presorted = true;
  } else if (P.n_big) {
    const uint32_t n_big = P.n_big;
    PA_TRY(W.seg_list.reserve((uint64_t)n_big * 8 + 16));
    uint32_t *big_a0 = W.seg_list.as<uint32_t>(), *big_nh = big_a0 + n_big;
    PA_HIP(hipMemsetAsync(W.slot(kBigCursor), 0, kBigCursor.bytes(), c->stream));
    PA_TRY(PA_LAUNCH(c, big_segments_kernel, ceil_div(S.n_large, kThreads), kThreads, 0, W.seg_a0.as<uint32_t>() + S.large_at,
                     W.seg_nh.as<uint32_t>() + S.large_at, S.n_large, big_a0, big_nh, W.slot(kBigCursor)));
    uint32_t np2_max = 2;
    while (np2_max < P.max_big) np2_max <<= 1;
    const uint32_t sort_lds = np2_max * 12u;
    // (contig, window id) to the top, the rank below
    PA_TRY(PA_LAUNCH_RAISE_LDS(c, frag_sort_kernel, n_big, kFragSortThreads, sort_lds, S.hk[0], S.hv[0], big_a0, big_nh, np2_max,
                               kHitRankRotation));
  }
  return PA_OK;
}

// general path (more than 8 192 genomes): all hits sorted by key, segments from head flags
int list_segments_sorted(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, const FragBatch &B, SegLists &S) {
  PA_TRY(begin_hits(W, B, S));
  const uint64_t n_hits = B.n_hits;
  PA_TRY(PA_LAUNCH(c, fill_hits_kernel, ceil_div(B.nf, kThreads / 64), kThreads, 0, B.nf, B.q_pos, B.q_id, W.q_s.as<uint32_t>(),
                   W.hit_off.as<uint32_t>(), W.post_start.as<uint32_t>(), W.vals[R.which].as<uint32_t>(), W.mini_wpos.as<uint32_t>(),
                   W.mini_contig.as<uint32_t>(), S.hk[0], S.hv[0]));
  if (B.max_hits <= kFragSortMax) {  // every fragment's hits fit one LDS sort
    uint32_t np2_max = 2;
    while (np2_max < B.max_hits) np2_max <<= 1;
    const uint32_t lds_bytes = np2_max * 12u;
    PA_TRY(PA_LAUNCH_RAISE_LDS(c, frag_sort_kernel, B.nf, kFragSortThreads, lds_bytes, S.hk[0], S.hv[0], W.hit_off.as<uint32_t>(),
                               W.hit_count.as<uint32_t>(), np2_max, 0u));
  } else {
    PA_TRY(sort_all_hits(c, W, B, S));
  }
  PA_TRY(W.flags.reserve(n_hits * 8 + 64));
  uint32_t *hf = W.flags.as<uint32_t>(), *hp = hf + n_hits;
  const uint64_t gh = ceil_div(n_hits, kThreads);
  PA_TRY(PA_LAUNCH(c, segment_heads_kernel, gh, kThreads, 0, S.hk[S.hw], (uint32_t)n_hits, W.contig_genome.as<uint32_t>(), hf));
  uint64_t total = 0;
  PA_TRY(pa_scan_total_u32(c, hf, hp, n_hits, W.slot<uint64_t>(kScanTotal), &total));
  const uint32_t n_segs = (uint32_t)total;
  PA_TRY(W.seg_start.reserve((uint64_t)(n_segs + 2) * 4));
  PA_TRY(PA_LAUNCH(c, segment_starts_kernel, gh, kThreads, 0, hf, hp, (uint32_t)n_hits, W.seg_start.as<uint32_t>()));
  // most segments are chance hits of unrelated genomes (fewer hits than any L1 run needs): drop them
  // here, one thread each, instead of spending a workgroup launch on each in the mapping kernel
  const uint64_t gs = ceil_div(n_segs, kThreads);
  PA_TRY(PA_LAUNCH(c, segment_keep_kernel, gs, kThreads, 0, S.hk[S.hw], W.seg_start.as<uint32_t>(), n_segs, W.q_s.as<uint32_t>(),
                   W.tab_min_hits.as<uint32_t>(), W.contig_genome.as<uint32_t>(), a.ref0, a.ref1, hf));
  PA_TRY(pa_scan_total_u32(c, hf, hp, n_segs, W.slot<uint64_t>(kScanTotal), &total));
  S.n_keep = (uint32_t)total;
  PA_TRY(W.seg_list.reserve((uint64_t)(S.n_keep + 1) * 4));
  PA_TRY(W.seg_a0.reserve((uint64_t)S.n_keep * 4 + 16));
  PA_TRY(W.seg_nh.reserve((uint64_t)S.n_keep * 4 + 16));
  PA_TRY(PA_LAUNCH(c, segment_list_kernel, gs, kThreads, 0, hf, hp, n_segs, W.seg_list.as<uint32_t>()));
  return PA_LAUNCH(c, segments_from_list_kernel, ceil_div(S.n_keep, kThreads), kThreads, 0, W.seg_start.as<uint32_t>(), W.seg_list.as<uint32_t>(),
                   S.n_keep, W.seg_a0.as<uint32_t>(), W.seg_nh.as<uint32_t>());
}

// ---- 4. (continued) mapping
// One list of segments through segment_records_kernel and the general mapping kernel.  kAll: every segment's hits fit the
// smaller LDS footprint.
template <bool kAll>
int launch_map(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, const FragBatch &B, const SegLists &S,
               const uint32_t *list_a0, const uint32_t *list_nh, const uint32_t *list_f, uint32_t count, uint32_t hit_cap) {
  if (count == 0) return PA_OK;
#ifdef PA_TOOLS
  const char *cut_env = PA_TOOL_ENV("PA_MAP_CUT");  // tools: the mapping kernel cut short after a phase (timing by difference)
  const uint32_t map_cut = cut_env ? (uint32_t)atoi(cut_env) : 0xffffffffu;
#endif
  PA_TRY(W.seg_rec.reserve((uint64_t)count * 48));
  PA_TRY(PA_LAUNCH(c, segment_records_kernel, ceil_div(count, kThreads), kThreads, 0, S.hk[S.hw], list_a0, list_nh, list_f, count,
                   W.q_s.as<uint32_t>(), W.q_cut.as<uint32_t>(), W.tab_min_hits.as<uint32_t>(), W.tab_min_shared.as<uint32_t>(),
                   W.contig_genome.as<uint32_t>(), W.genome_first_contig.as<uint32_t>(), W.contig_mini_off.as<uint32_t>(),
                   W.contig_bucket_off.as<uint32_t>(), W.frag_genome_local.as<uint32_t>(), W.seg_rec.as<uint4>()));
  int status = PA_OK;
  auto launch = [&](auto cap) {
    status = PA_LAUNCH(c, (map_segments_kernel<cap(), kAll>), count, 64, eval_lds_bytes(B.s_cap, hit_cap, cap()) + PA_MAP_LDS_PAD, S.hk[S.hw],
                       S.hv[S.hw], W.seg_rec.as<uint4>(), count, S.presorted, B.q_hash, W.q_tab.as<uint32_t>(),
                       W.frag_genome_local.as<uint32_t>(), a.frag_len, a.count_windows, W.tab_min_shared.as<uint32_t>(),
                       W.contig_mini_off.as<uint32_t>(), W.contig_bucket_off.as<uint32_t>(), W.bucket_first.as<uint32_t>(),
                       W.mini_hash.as<uint32_t>(), W.mini_wpos.as<uint32_t>(), W.prev_same.as<int32_t>(), W.contig_bin_off.as<uint32_t>(),
                       R.range_bins, B.table, W.run_g.as<uint32_t>(), B.s_cap, hit_cap PA_MAP_CUT_ARG);
  };
  if (!dispatch_value(R.ref_cap, value_list<256, 5, 64>{}, launch)) launch(std::integral_constant<int, 512>{});  // the longest stretch
  return status;
}

// The bucketed lists' short segments: the tiny-segment filter, then those of at most kSparseHits hits through
// map_sparse_kernel and the rest -- and what the sparse kernel hands on -- through the general kernel
int map_short_segments(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, const FragBatch &B, const SegLists &S) {
  const uint32_t n_keep = S.n_keep;
  PA_TRY(W.seg2_a0.reserve((uint64_t)n_keep * 4 + 16));
  PA_TRY(W.seg2_nh.reserve((uint64_t)n_keep * 4 + 16));
  PA_TRY(W.seg2_f.reserve((uint64_t)n_keep * 4 + 16));
  // segments of at most kSparseHits hits go to map_sparse_kernel (listed from the back of the same arrays), unless
  // the hits carry their ranks in the sort's payload (a batch ordered as a whole)
  uint32_t sparse_max = S.presorted ? 0u : kSparseHits;
  // tests: 0 = every segment through the general kernel (the switch can only take the sparse kernel away: its key layout
  // is the bucketed one)
  if (const char *v = PA_TOOL_ENV("PA_FRAGANI_SPARSE")) sparse_max = (atoi(v) && !S.presorted) ? kSparseHits : 0u;
  unsigned long long *d_pre_cursor = W.slot<unsigned long long>(kPreCursor);
  PA_HIP(hipMemsetAsync(d_pre_cursor, 0, kPreCursor.bytes(), c->stream));
  PA_TRY(PA_LAUNCH(c, prefilter_segments_kernel, ceil_div(n_keep, kThreads), kThreads, 0, S.hk[S.hw], W.seg_a0.as<uint32_t>(),
                   W.seg_nh.as<uint32_t>(), W.seg_f.as<uint32_t>(), n_keep, W.q_s.as<uint32_t>(), W.tab_min_hits.as<uint32_t>(),
                   W.q_cut.as<uint32_t>(), a.frag_len, W.seg2_a0.as<uint32_t>(), W.seg2_nh.as<uint32_t>(), W.seg2_f.as<uint32_t>(), d_pre_cursor,
                   sparse_max));
  unsigned long long pre_cursor = 0;
  PA_TRY(pa_read_back(c, d_pre_cursor, &pre_cursor));
  const uint32_t n_small = (uint32_t)pre_cursor, n_sparse = (uint32_t)(pre_cursor >> 32);
  if (R.trace)
    fprintf(stderr, "pa_fragani: genomes %u..%u: %u fragments, %llu seed hits, %u + %u listed segments, %u left "
                    "after the tiny-segment filter\n", B.g0, B.g1, B.nf, (unsigned long long)B.n_hits, n_keep, S.n_large, n_small);
  PA_TRY(launch_map<true>(c, W, a, R, B, S, W.seg2_a0.as<uint32_t>(), W.seg2_nh.as<uint32_t>(), W.seg2_f.as<uint32_t>(), n_small,
                          (uint32_t)kHitCapSmall));
  if (n_sparse == 0) return PA_OK;
  const uint32_t at = n_keep - n_sparse;  // the sparse list sits at the back of the same arrays
  PA_TRY(W.seg_over.reserve((uint64_t)n_sparse * 12 + 16));
  uint32_t *over_a0 = W.seg_over.as<uint32_t>(), *over_nh = over_a0 + n_sparse, *over_f = over_nh + n_sparse;
  uint32_t *d_over_n = W.slot(kSparseOver);
  PA_HIP(hipMemsetAsync(d_over_n, 0, kSparseOver.bytes(), c->stream));
#ifdef PA_MAP_STATS
#define PA_SPARSE_STATS_ARG , W.run_g.as<uint32_t>()
#else
#define PA_SPARSE_STATS_ARG
#endif
  PA_TRY(PA_LAUNCH(c, map_sparse_kernel, n_sparse, 64, 0, S.hk[S.hw], W.seg2_a0.as<uint32_t>() + at, W.seg2_nh.as<uint32_t>() + at,
                   W.seg2_f.as<uint32_t>() + at, n_sparse, W.q_s.as<uint32_t>(), B.q_hash, W.frag_genome_local.as<uint32_t>(), a.frag_len,
                   a.count_windows, W.tab_min_hits.as<uint32_t>(), W.tab_min_shared.as<uint32_t>(), W.contig_mini_off.as<uint32_t>(),
                   W.contig_bucket_off.as<uint32_t>(), W.bucket_first.as<uint32_t>(), W.mini_hash.as<uint32_t>(), W.mini_wpos.as<uint32_t>(),
                   W.prev_same.as<int32_t>(), W.contig_bin_off.as<uint32_t>(), R.range_bins, B.table, over_a0, over_nh, over_f,
                   d_over_n PA_SPARSE_STATS_ARG));
#undef PA_SPARSE_STATS_ARG
  uint32_t n_over = 0;
  PA_TRY(pa_read_back(c, d_over_n, &n_over));
  if (R.trace) fprintf(stderr, "pa_fragani: %u segments of at most %u hits in the sparse kernel, %u of them handed on\n", n_sparse, kSparseHits, n_over);
  // what does not fit the simple form (a hash twice in a stretch, over-long windows or ranges) goes through the general kernel
  return launch_map<true>(c, W, a, R, B, S, over_a0, over_nh, over_f, n_over, (uint32_t)kHitCapSmall);
}

int map_batch(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, const FragBatch &B, const SegLists &S) {
#ifdef PA_MAP_STATS
  PA_HIP(hipMemsetAsync(W.run_g.p, 0, 256, c->stream));
#endif
  if (!R.use_buckets)
    return launch_map<false>(c, W, a, R, B, S, W.seg_a0.as<uint32_t>(), W.seg_nh.as<uint32_t>(), nullptr, S.n_keep, (uint32_t)kHitCap);
  if (S.n_keep) PA_TRY(map_short_segments(c, W, a, R, B, S));
  return launch_map<false>(c, W, a, R, B, S, W.seg_a0.as<uint32_t>() + S.large_at, W.seg_nh.as<uint32_t>() + S.large_at,
                           W.seg_f.as<uint32_t>() + S.large_at, S.n_large, (uint32_t)kHitCap);
}

#ifdef PA_MAP_STATS
// the event counters of the two mapping kernels (PA_FRAGANI_TRACE)
int print_map_stats(pa_ctx *c, const FragWork &W) {
  uint32_t st[64];
  PA_TRY(pa_copy_to_host(c, st, W.run_g.p, 256));
  fprintf(stderr, "pa_fragani: map stats: %u segments at L1 with %u hits, %u candidates, %u groups, %u begins past the bound, "
                  "%u rounds, %u stretch entries, %u windows evaluated, %u fine passes, %u cooperative, %u begins in rounds, "
                  "%u begins finished, %u rounds without items, %u second passes, %u windows with an exact value, %u of them at or above the bar, "
                  "%u begins dropped by the tight bound, %u rounds ended by it; rounds by seed hits of the segment (<= 7, 8-15, 16-31, 32-63, "
                  "64-127, 128-255, more): %u %u %u %u %u %u %u, segments: %u %u %u %u %u %u %u; work model: %u minimizers in the candidates' ranges, "
                  "%u states tying their candidate's optimum; past the tight bound: %u rounds, %u begins, %u windows, %u of them at or above the bar; %u begins dropped by the bound asked at a round's end; %u segments that are one run of hits (no L1 scan) with %u hits; hits within 4096 window ids on one contig (ordered by counting): %u segments, all but one hit: %u, all but two: %u\n",
          st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], st[9], st[10], st[11], st[12], st[13], st[14], st[15], st[16], st[17],
          st[18], st[19], st[20], st[21], st[22], st[23], st[24], st[25], st[26], st[27], st[28], st[29], st[30], st[31], st[32], st[33], st[40], st[39], st[37], st[38], st[41], st[42], st[46], st[43], st[44], st[45]);
  fprintf(stderr, "pa_fragani: sparse stats: %u segments with a candidate, %u candidates, %u groups of begins evaluated, %u begins, %u states, %u begins tying "
                  "their candidate's best when folded; %u one-run segments with strays; %u begins with enough hits left out because they lie between two tying begins and hold no more hits than those share, %u groups between the ties passed over unseen, %u groups that hold a candidate's first or last tying begin, %u candidates whose first hit lies past the batch of 512 window ids\n",
          st[48], st[49], st[50], st[51], st[52], st[53], st[47], st[58], st[59], st[54], st[55]);
  return PA_OK;
}
#endif

// ---- 5. per pair of the batch: kept fragments and the sum of their identities
int reduce_batch(pa_ctx *c, FragWork &W, const FragCall &a, const FragRun &R, const FragBatch &B) {
  PA_TRY(W.matched.reserve((uint64_t)B.nq * a.n_genomes * 4));
  PA_TRY(W.ident_sum.reserve((uint64_t)B.nq * a.n_genomes * 8));
  return PA_LAUNCH(c, reduce_pairs_kernel, B.nq * a.n_genomes, 64, 0, B.table, R.range_bins, W.genome_bin_off.as<uint32_t>(), a.n_genomes,
                   W.ident_tab.as<float>(), W.matched.as<uint32_t>(), W.ident_sum.as<double>());
}
// the batch's rows of the two result matrices to the host: whole, or the columns of the reference range only
int copy_out_batch(pa_ctx *c, FragWork &W, const FragCall &a, const FragBatch &B) {
  const uint32_t n_genomes = a.n_genomes, out_cols = a.out_cols, nq = B.nq;
  if (out_cols == n_genomes) {
    PA_HIP(hipMemcpyAsync(a.h_matched + (uint64_t)B.g0 * n_genomes, W.matched.p, (uint64_t)nq * n_genomes * 4,
                          hipMemcpyDeviceToHost, c->stream));
    PA_HIP(hipMemcpyAsync(a.h_ident_sum + (uint64_t)B.g0 * n_genomes, W.ident_sum.p, (uint64_t)nq * n_genomes * 8,
                          hipMemcpyDeviceToHost, c->stream));
  } else if (out_cols) {
    PA_HIP(hipMemcpy2DAsync(a.h_matched + (uint64_t)B.g0 * out_cols, (size_t)out_cols * 4, W.matched.as<uint32_t>() + a.out_col0,
                            (size_t)n_genomes * 4, (size_t)out_cols * 4, nq, hipMemcpyDeviceToHost, c->stream));
    PA_HIP(hipMemcpy2DAsync(a.h_ident_sum + (uint64_t)B.g0 * out_cols, (size_t)out_cols * 8, W.ident_sum.as<double>() + a.out_col0,
                            (size_t)n_genomes * 8, (size_t)out_cols * 8, nq, hipMemcpyDeviceToHost, c->stream));
  }
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}

// ---- the pipeline
int fragani_ex_impl(pa_ctx *c, FragCall &a) {
  PA_TRY(check_call(c, a));
  FragWork &W = frag_work(c);
  PA_TRY(stage_contigs(c, W, a.h_contig_start, a.h_contig_len, a.h_contig_genome, a.n_contigs, a.n_genomes, a.arena_bases));
  if (a.reuse) {
    bool no_fragments = false;
    PA_TRY(check_reuse(W, a, &no_fragments));
    if (no_fragments) return PA_OK;
  }

  // the reference index: built (stages 1 and 2), or the last call's taken over
  std::optional<ProfScope> prof;  // phases timed for bench.py: index build, seeding, mapping
  W.index_valid = false;          // until this call has passed stage 2 (or taken it over)
  prof.emplace(c, PA_PROF_FRAG_INDEX);
  FragLayout L;
  FragRun R;
  uint32_t m = W.index_m;
  if (a.reuse) layout_fragments(a, L);
  else PA_TRY(build_minimizers(c, W, a, L, &m));
  if (m == 0 || L.frag_contig.empty()) {  // nothing to map (and nothing a later call could not take over)
    prof.reset();
    PA_HIP(hipStreamSynchronize(c->stream));
    if (m == 0) remember_index(W, a, m, 0);
    return PA_OK;
  }
  R.which = W.index_which;
  if (!a.reuse) PA_TRY(build_dictionary(c, W, a, m, &R.which));
  remember_index(W, a, m, R.which);
  R.restricted = !(W.index_ref0 == 0 && W.index_ref1 == a.n_genomes);
  PA_TRY(prepare_run(c, W, a, L, R));
  prof.reset();

  // batches of query genomes
  uint32_t batch_frags = PA_FRAGANI_BATCH_FRAGS;
  for (uint32_t g0 = a.qry0; g0 < a.qry1;) {
    FragBatch B;
    PA_TRY(choose_batch(a, L, R, g0, batch_frags, B));
    if (B.nf == 0) { g0 = B.g1; continue; }
    PA_TRY(stage_batch(c, W, a, L, R, B));
    prof.emplace(c, PA_PROF_FRAG_SEED);
    PA_TRY(seed_batch(c, W, a, R, B));
    if (B.n_hits >= R.hit_limit && B.nq > 1) {  // closely related or repetitive genomes: fewer query genomes per batch
      batch_frags = std::max<uint32_t>(1u, std::min(batch_frags, B.nf) / 2u);
      prof.reset();
      continue;  // the same g0 again
    }
    if (R.trace) fprintf(stderr, "pa_fragani: batch of genomes %u..%u: %u fragments, %llu seed hits\n", B.g0, B.g1, B.nf, (unsigned long long)B.n_hits);
    PA_REQUIRE(B.n_hits < (1ULL << 31), "pa_fragani: %llu seed hits for the fragments of genome %u alone (limit 2^31); highly "
               "repetitive input", (unsigned long long)B.n_hits, g0);
    PA_TRY(clear_table(c, W, R, B));
    if (B.n_hits) {
      SegLists S;
      if (R.use_buckets) PA_TRY(list_segments_bucketed(c, W, a, B, S));
      else PA_TRY(list_segments_sorted(c, W, a, R, B, S));
      prof.reset();
      prof.emplace(c, PA_PROF_FRAG_MAP);
      PA_TRY(map_batch(c, W, a, R, B, S));
#ifdef PA_MAP_STATS
      if (R.trace) PA_TRY(print_map_stats(c, W));
#endif
    }
    PA_TRY(reduce_batch(c, W, a, R, B));
    prof.reset();
    PA_TRY(copy_out_batch(c, W, a, B));
    g0 = B.g1;
  }
  uint32_t h_over[2] = {0, 0};
  PA_TRY(pa_copy_to_host(c, h_over, W.slot(kSketchOverflow), kSketchOverflow.bytes()));
  if (h_over[0]) {
    pa_set_error("pa_fragani: %u fragment sketches exceeded %d minimizers (fragLen too long for this window); "
                 "those sketches were truncated", h_over[0], kQMax);
    return PA_E_CAPACITY;
  }
  return PA_OK;
}

}  // namespace

void pa_fragani_release(pa_ctx *c) {
  delete static_cast<FragWork *>(c->frag_work);
  c->frag_work = nullptr;
}

extern "C" {

int pa_fragani_window(uint32_t k, uint32_t frag_len) { return window_size_for((int)k, (int)frag_len); }

// The fragment-ANI workspace of a context: bytes held now, the most it ever held (buffers only grow: the same until
// pa_fragani_release), and the cap (0: none).  A cap bounds what later calls may ask the device for: a call that would
// pass it ends with PA_E_NOMEM and a message naming the call and the sizes, the workspace as it was.
int pa_fragani_workspace(pa_ctx *c, uint64_t *held_bytes, uint64_t *peak_bytes, uint64_t *cap_bytes) {
  PA_REQUIRE(c, "pa_fragani_workspace: null context");
  const FragWork *W = static_cast<const FragWork *>(c->frag_work);
  if (held_bytes) *held_bytes = W ? W->budget.held : 0;
  if (peak_bytes) *peak_bytes = W ? W->budget.peak : 0;
  if (cap_bytes) *cap_bytes = W ? W->budget.cap : 0;
  return PA_OK;
}
int pa_fragani_set_workspace_cap(pa_ctx *c, uint64_t cap_bytes) {
  PA_REQUIRE(c, "pa_fragani_set_workspace_cap: null context");
  frag_work(c).budget.cap = cap_bytes;
  return PA_OK;
}

int pa_fragani_set_ambiguous(pa_ctx *c, const uint32_t *d_packed, const uint64_t *h_pos, const uint8_t *h_byte, uint64_t n) {
  PA_REQUIRE(c && (n == 0 || (d_packed && h_pos && h_byte)), "pa_fragani_set_ambiguous: null argument");
  PA_REQUIRE(n < (1ULL << 31), "pa_fragani_set_ambiguous: %llu residues (limit 2^31)", (unsigned long long)n);
  for (uint64_t i = 1; i < n; ++i)
    PA_REQUIRE(h_pos[i] > h_pos[i - 1], "pa_fragani_set_ambiguous: positions must ascend (entry %llu)", (unsigned long long)i);
  PA_HIP(hipSetDevice(c->device));
  FragWork &W = frag_work(c);
  if (n == 0 && W.amb_n == 0) return PA_OK;
  if (n && W.amb_n == n && W.amb_for == (const void *)d_packed && memcmp(W.amb_host_pos.data(), h_pos, n * 8) == 0 &&
      memcmp(W.amb_host_byte.data(), h_byte, n) == 0)
    return PA_OK;  // the list the context holds already (a reusable index stays reusable)
  W.index_valid = false;  // an index built with another list (or none) hashed those residues differently
  W.amb_for = nullptr;
  W.amb_n = 0;
  W.amb_host_pos.clear();
  W.amb_host_byte.clear();
  if (n == 0) return PA_OK;
  W.amb_host_pos.assign(h_pos, h_pos + n);
  W.amb_host_byte.assign(h_byte, h_byte + n);
  PA_TRY(W.amb_pos.reserve(n * 8));
  PA_TRY(W.amb_byte.reserve(n + 16));
  PA_HIP(hipMemcpyAsync(W.amb_pos.p, h_pos, n * 8, hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipMemcpyAsync(W.amb_byte.p, h_byte, n, hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipStreamSynchronize(c->stream));
  W.amb_for = d_packed;
  W.amb_n = (uint32_t)n;
  return PA_OK;
}

int pa_fragani_tables(uint32_t k, uint32_t s_max, uint32_t *h_min_hits, uint32_t *h_min_shared) {
  if (!h_min_hits || !h_min_shared) { pa_set_error("pa_fragani_tables: null argument"); return PA_E_INVALID; }
  h_min_hits[0] = h_min_shared[0] = 0;
  for (uint32_t s = 1; s <= s_max; ++s) {
    const int mh = relaxed_min_hits((int)s, (int)k);
    h_min_hits[s] = (uint32_t)(mh < 1 ? 1 : mh);
    h_min_shared[s] = (uint32_t)min_shared_for((int)s, (int)k);
  }
  return PA_OK;
}

// fastANI holds the Jaccard estimate, the Mash distance and the identity as floats (Mashmap's j2md takes and returns a
// float, and nucIdentity = 100 * (1 - mash_dist) is float arithmetic): the value here is that float, widened.
double pa_fragani_identity(uint32_t shared, uint32_t s, uint32_t k) {
  if (!s) return 0.0;
  const float j = (float)(1.0 * shared / s);
  float d;
  if (j == 0) d = 1.0f;
  else if (j == 1) d = 0.0f;
  else d = (float)((-1.0 / (int)k) * std::log(2.0 * j / (1 + j)));
  return (double)(100 * (1 - d));
}

int pa_fragani_sketch(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                      const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
                      uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t window, uint32_t *h_hash,
                      uint32_t *h_wpos, uint32_t *h_contig, uint64_t cap, uint64_t *n_out) {
  PA_REQUIRE(c && d_packed && d_mask && n_out, "pa_fragani_sketch: null argument");
  PA_REQUIRE(window >= 1 && window <= 64, "pa_fragani_sketch: window %u outside [1,64]", window);
  PA_HIP(hipSetDevice(c->device));
  FragWork &W = frag_work(c);
  W.index_valid = false;  // the minimizer arrays are about to be overwritten
  PA_TRY(stage_contigs(c, W, h_contig_start, h_contig_len, h_contig_genome, n_contigs, n_genomes, arena_bases));
  uint32_t m = 0;
  PA_TRY(dispatch_minimizers(c, W, d_packed, d_mask, arena_bases, n_contigs, k, (int)window, &m));
  *n_out = m;
  if (m > cap) { pa_set_error("pa_fragani_sketch: %u minimizers, room for %llu", m, (unsigned long long)cap); return PA_E_CAPACITY; }
  if (m) {
    PA_HIP(hipMemcpyAsync(h_hash, W.mini_hash.p, (uint64_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    PA_HIP(hipMemcpyAsync(h_wpos, W.mini_wpos.p, (uint64_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    PA_HIP(hipMemcpyAsync(h_contig, W.mini_contig.p, (uint64_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  }
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}

int pa_fragani(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
               const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
               uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t frag_len, uint32_t ref0, uint32_t ref1,
               uint32_t *h_total_frags, uint32_t *h_matched, double *h_ident_sum) {
  return pa_fragani_ex(c, d_packed, d_mask, arena_bases, h_contig_start, h_contig_len, h_contig_genome, n_contigs,
                       n_genomes, k, frag_len, 0, n_genomes, ref0, ref1, 0, h_total_frags, h_matched, h_ident_sum);
}

int pa_fragani_ex(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                  const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
                  uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t frag_len, uint32_t qry0, uint32_t qry1,
                  uint32_t ref0, uint32_t ref1, uint32_t flags, uint32_t *h_total_frags, uint32_t *h_matched,
                  double *h_ident_sum) {
  FragCall call{d_packed, d_mask, arena_bases, h_contig_start, h_contig_len, h_contig_genome, n_contigs, n_genomes, k,
                frag_len, qry0, qry1, ref0, ref1, flags, h_total_frags, h_matched, h_ident_sum};
  const int status = fragani_ex_impl(c, call);
  if (status == PA_E_NOMEM && c && c->frag_work) {
    // A call that ends for want of memory -- the cap, or the device -- gives back what the workspace held (the buffers that
    // had grown for it included), so that a smaller call starts from nothing instead of from a half-grown workspace; the
    // index of an earlier call goes with it.  The list of residues that are neither ACGT nor N stays (a few bytes).
    FragWork &W = frag_work(c);
    (void)hipStreamSynchronize(c->stream);
    W.each_buffer([&W](DevBuf &b) { if (&b != &W.amb_pos && &b != &W.amb_byte) b.release(); });
    W.index_valid = false;
    W.tables_k = 0;
  }
  return status;
}

}  // extern "C"
