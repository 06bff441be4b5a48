// fragani_rules.inc -- part of fragani.hip (included there, inside its anonymous namespace: one translation unit): the layout of a seed hit's key and the rules of the mapping that map_segments_kernel and map_sparse_kernel share -- the L1 rule, a candidate's first begin, a begin's widest window, the bar, the fold of ties, the report.  Each is stated here once; the kernels call them.

// ============================================================== the key of a seed hit
// 64 bits: the window id of the reference minimizer in the low 24 (contigs are shorter than 2^24), its contig in the 20
// above -- together the hit's PLACE, 44 bits -- and on top either the query fragment (20 bits: hits ordered as a whole,
// postings) or, for a bucketed hit, the rank of its hash in the fragment's sketch: 9 bits at kHitRankShift, the 11 bits
// between left zero.
constexpr uint32_t kHitWindowBits = 24, kHitContigBits = 20, kHitPlaceBits = kHitWindowBits + kHitContigBits;
constexpr uint32_t kHitFragmentBits = 20, kHitRankBits = 9, kHitRankShift = 55;
static_assert(kHitPlaceBits + kHitFragmentBits == 64, "window id, contig and fragment tile the key");
static_assert(kHitRankShift >= kHitPlaceBits && kHitRankShift + kHitRankBits == 64, "place, spare bits and rank tile the key");
static_assert((1u << kHitRankBits) >= (uint32_t)kQMax, "a rank in a sketch fits its field");
constexpr uint32_t kHitWindowMax = (1u << kHitWindowBits) - 1u;
constexpr uint64_t kHitPlaceMask = (1ULL << kHitPlaceBits) - 1ULL;
constexpr __host__ __device__ uint32_t hit_window(uint64_t key) { return (uint32_t)key & kHitWindowMax; }
constexpr __host__ __device__ uint32_t hit_contig(uint64_t key) { return (uint32_t)(key >> kHitWindowBits) & ((1u << kHitContigBits) - 1u); }
constexpr __host__ __device__ uint64_t hit_place(uint64_t key) { return key & kHitPlaceMask; }  // contig << 24 | window id
constexpr __host__ __device__ uint32_t hit_fragment(uint64_t key) { return (uint32_t)(key >> kHitPlaceBits); }
constexpr __host__ __device__ uint32_t hit_rank(uint64_t key) { return (uint32_t)(key >> kHitRankShift); }
constexpr __host__ __device__ uint64_t place_of(uint32_t contig, uint32_t window) { return ((uint64_t)contig << kHitWindowBits) | window; }
constexpr __host__ __device__ uint64_t hit_key_of_fragment(uint32_t fragment, uint64_t place) { return ((uint64_t)fragment << kHitPlaceBits) | place; }
constexpr __host__ __device__ uint64_t hit_key_of_rank(uint32_t rank, uint64_t place) { return ((uint64_t)rank << kHitRankShift) | place; }
// A posting (post_cw) is the place of a reference minimizer with its GENOME on top, so that bucketing needs no second lookup.
constexpr __host__ __device__ uint64_t posting_of(uint32_t genome, uint64_t place) { return hit_key_of_fragment(genome, place); }
constexpr __host__ __device__ uint32_t posting_genome(uint64_t cw) { return hit_fragment(cw); }
// A bucketed hit turned left by this many bits has its place on top and the rank below it (frag_sort_kernel's `rot`).
constexpr uint32_t kHitRankRotation = 64u - kHitPlaceBits;
// The sort key of a bucketed hit inside a wave (stage_hits_sorted, map_sparse_kernel): the place on top of the rank -- a
// (contig, window id) occurs once in a segment, the rank decides nothing.
constexpr __host__ __device__ uint64_t hit_sort_key(uint64_t key) { return (hit_place(key) << kHitRankBits) | hit_rank(key); }
constexpr __host__ __device__ uint32_t sort_key_rank(uint64_t k) { return (uint32_t)k & ((1u << kHitRankBits) - 1u); }
constexpr __host__ __device__ uint32_t sort_key_window(uint64_t k) { return hit_window(k >> kHitRankBits); }
constexpr __host__ __device__ uint32_t sort_key_contig(uint64_t k) { return hit_contig(k >> kHitRankBits); }

// ============================================================== L1
// Run a is valid when hits a .. a+mh-1 share a contig and span < frag_len window ids; its candidate range of window starts
// is [y.w - fragLen + 1, x.w] (x, y: the run's first and last hit); ranges that touch on one contig merge (hits are in
// (contig, window) order, so both ends only grow and "touches the merged range" is "touches the previous run's").
__device__ __forceinline__ bool l1_run_valid(uint32_t c_first, uint32_t w_first, uint32_t c_last, uint32_t w_last, uint32_t frag_len) {
  return c_last == c_first && w_last - w_first < frag_len;
}
__device__ __forceinline__ uint32_t l1_range_start(uint32_t w_last, uint32_t frag_len) { return w_last + 1u > frag_len ? w_last + 1u - frag_len : 0u; }
// a valid run on contig c whose range starts at cs opens a new candidate, after a valid run on prev_c whose range ended at prev_ce
__device__ __forceinline__ bool l1_opens_candidate(bool have_prev, uint32_t prev_c, uint32_t prev_ce, uint32_t c, uint32_t cs) {
  return !have_prev || prev_c != c || cs > prev_ce;
}
// fastANI keeps every candidate as a mapping, orders a fragment's mappings by identity and lets each overwrite the one
// before: of several candidates that share equally many minimizers the LAST one -- the candidates come in (contig,
// position) order -- is the fragment's mapping.
__device__ __forceinline__ bool candidate_is_the_mapping(int32_t c_best, int32_t best_shared) { return c_best >= 0 && c_best >= best_shared; }

// ============================================================== a candidate's slide
// Window ids of 512 minimizers from the start of the range's bucket on ([lo, hi): the bucket of the range's start cs, m1:
// the end of the contig's minimizers), in ONE batch of loads: the first begin is the first of them at or past the range's
// start (a bucket holds ~20: it lies among the first 64), and the rest say where the slide ends, where the range of
// begins ends and where the first seed hit sits -- the search for the first begin and the batch were two memory round
// trips, one waiting for the other.  (The groups re-read their own 64 window ids later: they are in L2 by then, and eight
// registers are free.)  b_lo: the first begin; wpv[q] of a lane: the window id of minimizer origin + 64 q + lane.
constexpr int kStartBatch = 8;
__device__ __forceinline__ void slide_first_begin(const uint32_t *mini_wpos, uint32_t m1, uint32_t lo, uint32_t hi, uint32_t cs,
                                                  uint32_t lane, uint32_t &b_lo, uint32_t &origin, uint32_t (&wpv)[kStartBatch]) {
  auto load_batch = [&]() {
#pragma unroll
    for (int q = 0; q < kStartBatch; ++q) {
      const uint32_t t = origin + (uint32_t)q * 64u + lane;
      wpv[q] = t < m1 ? mini_wpos[t] : 0xffffffffu;
    }
  };
  origin = lo;
  load_batch();
  const uint64_t ge = __ballot(lo + lane < hi && wpv[0] >= cs);
  if (ge) {
    b_lo = lo + (uint32_t)__builtin_ctzll(ge);
  } else if (hi - lo <= 64u) {
    b_lo = hi;  // the first minimizer of the next bucket (still in the batch)
  } else {  // a bucket of more than 64 minimizers (low-complexity sequence): searched on, the batch loaded again from the begin found
    b_lo = hi;
    for (uint32_t base = lo + 64u; base < hi; base += 64) {
      const uint32_t t = base + lane;
      const uint64_t ge2 = __ballot(t < hi && mini_wpos[t] >= cs);
      if (ge2) { b_lo = base + (uint32_t)__builtin_ctzll(ge2); break; }
    }
    origin = b_lo;
    load_batch();
  }
}

// ============================================================== per begin, per group of begins
// The begin's widest window: the window ids from its minimizer's (wp) to below w_end -- its last state ends where the next
// begin's minimizer (wp_next) comes in, or where the slide ends.
struct WidestWindow { uint32_t wp, wp_next, w_end; };
__device__ __forceinline__ WidestWindow begin_widest_window(const uint32_t *mini_wpos, uint32_t m1, uint32_t b, bool has, uint32_t i_max, uint32_t count_windows) {
  const uint32_t wp = has ? mini_wpos[b] : 0u;
  const uint32_t wp_next = (has && b + 1u < m1) ? mini_wpos[b + 1u] : 0xffffffffu;
  return {wp, wp_next, min(wp_next - 1u, i_max) + count_windows};
}
// What a window must share to matter (ties matter): the best of its candidate so far or of the fragment's best mapping so
// far, and never less than a mapping needs to be reported (floor_bar: tab_min_shared[s]).
__device__ __forceinline__ int32_t shared_bar(int32_t c_best, int32_t best_shared, int32_t floor_bar) {
  const int32_t bar = c_best > best_shared ? c_best : best_shared;
  return bar < floor_bar ? floor_bar : bar;
}
// Fold a group of evaluated begins into the candidate's optimum: most shared; window ids (a state's position is its
// begin's) of the first and of the last begin that has it -- the groups of a candidate do not come in slide order.  `top`:
// the lanes that hold group_best (not empty, group_best >= c_best), in slide order; wp: the lane's position.  A strictly
// better group starts the ties anew (true is returned).
__device__ __forceinline__ bool fold_ties(int32_t group_best, uint64_t top, uint32_t wp, int32_t &c_best, uint32_t &c_first, uint32_t &c_last) {
  const uint32_t w_first = __shfl(wp, __builtin_ctzll(top), 64), w_last = __shfl(wp, 63 - __builtin_clzll(top), 64);
  const bool better = group_best > c_best;
  c_last = better ? w_last : max(c_last, w_last);
  c_first = better ? w_first : min(c_first, w_first);
  c_best = group_best;
  return better;
}
// The report: a fragment's mapping goes into the table of its genome with atomicMax, the identity as a 30-bit fixed-point
// quotient on top, so that the best mapping of a bin stays; fastANI buckets the reference by fragLen - 20, and the
// mapping's position is the mean of its first and last optimal state's (bin_off: contig_bin_off of the mapping's contig).
__device__ __forceinline__ unsigned long long mapping_packed(int32_t shared, uint32_t s) {
  const uint64_t jq = ((uint64_t)shared << 30) / s;
  return ((unsigned long long)jq << 32) | ((unsigned long long)shared << 16) | s;
}
__device__ __forceinline__ uint64_t mapping_bin(uint32_t bin_off, uint32_t w_first, uint32_t w_last, uint32_t frag_len) {
  return bin_off + (w_first + w_last) / 2u / (frag_len - 20u);
}
