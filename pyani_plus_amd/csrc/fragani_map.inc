// fragani_map.inc -- part of fragani.hip (included there, inside its anonymous namespace: one translation unit): the general mapping kernel: one wave per (fragment, reference genome) segment -- L1 scan, the exact slide, bit tables, the tight bound.

// Reference minimizers of one stretch (the windows of up to 64 starts) held in LDS: a compile-time parameter of the
// mapping kernel, chosen per call from the expected minimizers per window (map_ref_cap) -- 320 for fastANI's defaults
// (237 per window): with 512 the per-lane arrays cost registers and waves (1.04 s against 0.99 s for the 1 000-genome
// run), with 256 most windows no longer fit and take the cooperative path (2.9 s).
constexpr uint32_t kRefCapMax = 512;
// LDS of one segment's wave, carved from dynamic shared memory so that the query-hash arrays are only as
// long as the longest fragment sketch of the batch (s_cap): ~8 KB per wave instead of 17 KB, which is what
// sets how many of these latency-bound waves a CU keeps in flight.
struct EvalShared {
  uint32_t *qh;        // [s_cap] the fragment's sketch, ascending
  uint32_t *cnt;       // [s_cap + 64] reference-only hashes per rank gap (cooperative evaluation of one over-long window);
  uint32_t *tab;       //   the same memory: the bit tables of the windowed evaluation (eval_tab_words)
  uint32_t *matched;   // [kQMax / 32] bitset over query ranks (cooperative evaluation of one over-long window)
  uint32_t *cand;      // [4 * 8] candidates of the L1 scan waiting for their evaluation: contig, first and last start, first hit
  uint32_t *scan;      // [24] the L1 scan's state while the candidates it has listed are evaluated [0..10], the best mapping so far [16..23]
  uint32_t *lmask;     // [kLmaskWords] one bit per staged hit: the rank of its hash lies below the pivot of the tight bound;
  uint32_t *lpre;      // [kLmaskWords] set bits in the words before (so "hits below the pivot among the first i" is two reads)
  uint32_t *hw;        // [kHitCap] window id of each staged hit << 8 | rank of its hash in the fragment's sketch >> 1
  uint16_t *hc;        // [kHitCap] contig of each staged hit, relative to the segment's first
  uint16_t *ref_w;     // [kRefCap] window id relative to the first minimizer's of the stretch
  uint16_t *prev;      // [kRefCap] 1 + stretch position of the same hash earlier in the stretch, 0: none
  uint16_t *qt;        // [kQtBuckets] the fragment's sketch bucketed by the top bits of the hash: first rank (10 bits) | hashes in the bucket (6 bits)
};
constexpr uint32_t kLmaskWords = (uint32_t)kHitCap / 32u + 2u;  // a word per 32 staged hits, one more for "all of them", even
__device__ __forceinline__ uint32_t staged_hit(uint32_t window, uint32_t rank) { return (window << 8) | (rank >> 1); }  // EvalShared::hw
// Bit tables of the windowed evaluation: one row per query rank r = the stretch positions (one bit each, kRefCap / 32
// words) whose minimizer has rank <= r among the fragment's hashes.  Coarse rows stand at every kCoarse-th rank; the
// fine rows cover kFineGroups coarse groups at a time, every rank of them.
constexpr uint32_t kCoarseShift = 4, kCoarse = 1u << kCoarseShift;
#ifndef PA_MAP_FINE_GROUPS
#define PA_MAP_FINE_GROUPS 2
#endif
constexpr uint32_t kFineGroups = PA_MAP_FINE_GROUPS, kFineRows = kFineGroups * kCoarse + 1u;
__host__ __device__ inline uint32_t eval_tab_words(uint32_t s_cap, uint32_t ref_cap) {
  const uint32_t t = (s_cap / kCoarse + 1u + kFineRows) * (ref_cap / 16u), c = s_cap + 64u;  // coarse and fine rows of two halves
  return ((t > c ? t : c) + 3u) & ~3u;
}
__host__ __device__ inline uint32_t eval_lds_bytes(uint32_t s_cap, uint32_t hit_cap, uint32_t ref_cap) {
  return 4u * s_cap + 4u * eval_tab_words(s_cap, ref_cap) + 4u * (kQMax / 32) + 128u + 96u + 8u * kLmaskWords + hit_cap * 6u + ref_cap * 4u +
         2u * kQtBuckets;
}
// The arrays whose length is known at compile time come first, so that their addresses are constants of the kernel
// (immediate offsets of the LDS instructions, no registers); the fragment's sketch and the tables follow.
__device__ __forceinline__ EvalShared eval_carve(uint32_t *base, uint32_t s_cap, uint32_t hit_cap, uint32_t kRefCap) {
  EvalShared sh;
  sh.matched = base;
  sh.cand = sh.matched + kQMax / 32;
  sh.scan = sh.cand + 32;
  sh.lmask = sh.scan + 24;
  sh.lpre = sh.lmask + kLmaskWords;
  sh.qt = reinterpret_cast<uint16_t *>(sh.lpre + kLmaskWords);  // (2 kLmaskWords is a multiple of 4: still on a 16-byte boundary)
  sh.hw = reinterpret_cast<uint32_t *>(sh.qt + kQtBuckets);
  sh.hc = reinterpret_cast<uint16_t *>(sh.hw + hit_cap);
  sh.ref_w = sh.hc + hit_cap;  // hit_cap and kRefCap are multiples of 64: everything stays on 16-byte boundaries
  sh.prev = sh.ref_w + kRefCap;
  sh.qh = reinterpret_cast<uint32_t *>(sh.prev + kRefCap);
  sh.cnt = sh.qh + s_cap;  // s_cap is a multiple of 64: the tables start on a 16-byte boundary
  sh.tab = sh.cnt;
  return sh;
}

// One record per listed segment: what a mapping wave needs before it can load anything else -- where the hits are, the
// fragment, its sketch size, the seed hits a run needs, the first contig of the reference genome -- gathered by one
// thread per segment, so that the wave starts with one scalar load instead of a chain of five dependent ones.
// Three uint4: {first hit, hits, fragment, sketch size} {hits a run needs, first contig, hashes of the sketch that lost seed hits to the
// frequency cut, shared minimizers a mapping needs} {end of the first contig's minimizers, its first bucket, the next contig's first
// bucket, the fragment's genome in the batch}; sketch size 0 = nothing to do.
__global__ __launch_bounds__(kThreads) void segment_records_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_a0, const uint32_t *__restrict__ seg_nh,
    const uint32_t *__restrict__ seg_f /* null: the fragment is the top of the key */, uint32_t n_segs,
    const uint32_t *__restrict__ q_s, const uint32_t *__restrict__ q_cut, const uint32_t *__restrict__ tab_min_hits,
    const uint32_t *__restrict__ tab_min_shared, const uint32_t *__restrict__ contig_genome,
    const uint32_t *__restrict__ genome_first_contig, const uint32_t *__restrict__ contig_mini_off,
    const uint32_t *__restrict__ contig_bucket_off, const uint32_t *__restrict__ frag_genome_local, uint4 *__restrict__ rec) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_segs) return;
  const uint32_t a0 = seg_a0[i], nh = seg_nh[i];
  const uint64_t key = keys[a0];
  const uint32_t f = seg_f ? seg_f[i] : hit_fragment(key);
  uint32_t s = q_s[f];
  const uint32_t mh = s ? tab_min_hits[s] : 0u, ms = s ? tab_min_shared[s] : 0u;
  if (nh < mh) s = 0;  // chance matches with unrelated genomes: fewer seed hits than any L1 run needs
  const uint32_t hc_base = genome_first_contig[contig_genome[hit_contig(key)]];
  rec[3 * (uint64_t)i] = make_uint4(a0, nh, f, s);
  rec[3 * (uint64_t)i + 1] = make_uint4(mh, hc_base, q_cut[f], ms);
  rec[3 * (uint64_t)i + 2] = make_uint4(contig_mini_off[hc_base + 1u], contig_bucket_off[hc_base], contig_bucket_off[hc_base + 1u], frag_genome_local[f]);
}

// the segment's hits from the hit array into LDS, in order: window id and rank (see EvalShared::hw), contig relative to
// the genome's first.  The hits come as the bucketing pass left them: the rank on top of the place (hit_key_of_rank).
// `loaded(nearest, widest)`: called once the hits are there, before they are ordered, with the smallest window id and the
// largest relative contig of the segment -- what the caller wants to ask the memory for while the ordering goes on.
// What a fragment leaves in a genome of its species is, nearly always, ONE cluster of hits -- its own locus: one contig, a
// span of at most a fragment length -- and now and then one or two stray hits somewhere else (96 % of the segments at 1 000
// genomes).  Such hits are ordered by COUNTING instead of by the network: around a pivot hit a window of kCountSpan window
// ids, a bit per window id (two hits never share a contig and a window id), prefix counts over the words; a hit's place is
// the number of bits below its own, the at most two hits outside the window go before or after by comparison.  Some
// eighty vector instructions for up to 256 hits where the bitonic network takes six hundred; the arrays it leaves are the
// same.  A pivot that is itself a stray leaves (nearly) all hits outside: once more with another hit, then the network.
// `scratch`: 2 * kCountWords words of LDS that nothing else uses while the hits are staged (the memory of the bit tables).
#ifndef PA_MAP_COUNT_SORT
#define PA_MAP_COUNT_SORT 1  // 0 in a test build: every segment through the network
#endif
constexpr uint32_t kCountWords = 256, kCountSpan = 32u * kCountWords;  // four words per lane; the pivot in the middle
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}
template <int E, class Loaded>
__device__ __forceinline__ void stage_hits_sorted(const uint64_t *__restrict__ seg_keys, uint32_t nh, uint32_t hc_base,
                                                  uint32_t lane, uint32_t *hw, uint16_t *hc, uint32_t *scratch, Loaded &&loaded) {
  uint64_t k[E];
  uint32_t widest = 0, furthest = 0, nearest = 0xffffffffu;  // largest relative contig, largest and smallest window id of the segment
  // (loads without a branch -- past the segment's end its last hit, discarded --, all of them asked for before any is looked
  // at: with the load under the test the compiler waited for each before it asked for the next, four round trips for four keys)
  uint64_t raws[E];
#pragma unroll
  for (int q = 0; q < E; ++q) raws[q] = seg_keys[min(lane * (uint32_t)E + (uint32_t)q, nh - 1u)];
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
    const uint64_t raw = raws[q];
    k[q] = e < nh ? hit_sort_key(raw) : ~0ULL;
    if (e < nh) {
      widest = max(widest, hit_contig(raw) - hc_base);
      furthest = max(furthest, hit_window(raw));
      nearest = min(nearest, hit_window(raw));
    }
  }
  widest = pa_dev::wave_max_dpp(widest);
  furthest = pa_dev::wave_max_dpp(furthest);
  nearest = pa_dev::wave_min_dpp(nearest);
  loaded(nearest, widest);
  if (PA_MAP_COUNT_SORT) {
    for (uint32_t attempt = 0; attempt < 2u; ++attempt) {
      const uint64_t pivot = hit_place(readlane_u64(raws[0], attempt));  // hit 0, then hit E (past the segment's end: its last hit)
      const uint32_t pw = hit_window(pivot), base = pw > kCountSpan / 2u ? pw - kCountSpan / 2u : 0u;
      const uint64_t lo_key = place_of(hit_contig(pivot), base);  // the window: this contig, window ids [base, base + kCountSpan)
      uint32_t out_q = 0, n_out = 0;  // bit q: the lane's hit q lies outside the window
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
        const uint64_t mine = hit_place(raws[q]);
        const bool inside = hit_contig(mine) == hit_contig(pivot) && hit_window(mine) - base < kCountSpan;  // (below the base: the difference wraps)
        const bool out = e < nh && !inside;
        out_q |= (out ? 1u : 0u) << q;
        n_out += (uint32_t)__popcll(__ballot(out));
      }
      if (n_out > 2u) continue;
      uint64_t o1 = ~0ULL, o2 = ~0ULL;  // the keys of the hits outside
      if (n_out) {
#pragma unroll
        for (int q = 0; q < E; ++q) {
          for (uint64_t m = __ballot((out_q >> q) & 1u); m; m &= m - 1) {
            const uint64_t key = hit_place(readlane_u64(raws[q], (uint32_t)__builtin_ctzll(m)));
            if (o1 == ~0ULL) o1 = key; else o2 = key;
          }
        }
      }
      const uint32_t n_cluster = nh - n_out, n_low = (o1 < lo_key ? 1u : 0u) + (o2 < lo_key ? 1u : 0u);
      uint32_t *bits = scratch, *before = scratch + kCountWords;
      reinterpret_cast<uint4 *>(bits)[lane] = make_uint4(0u, 0u, 0u, 0u);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
        const uint32_t rel = hit_window(raws[q]) - base;
        if (e < nh && !((out_q >> q) & 1u)) atomicOr(&bits[rel >> 5], 1u << (rel & 31u));
      }
      __builtin_amdgcn_wave_barrier();
      {
        const uint4 mine = reinterpret_cast<const uint4 *>(bits)[lane];  // words 4 lane .. 4 lane + 3
        const uint32_t c0 = (uint32_t)__popc(mine.x), c1 = (uint32_t)__popc(mine.y), c2 = (uint32_t)__popc(mine.z), c3 = (uint32_t)__popc(mine.w);
        const uint32_t ex = pa_dev::wave_incl_scan_dpp(c0 + c1 + c2 + c3) - (c0 + c1 + c2 + c3) + n_low;
        reinterpret_cast<uint4 *>(before)[lane] = make_uint4(ex, ex + c0, ex + c0 + c1, ex + c0 + c1 + c2);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
        if (e < nh) {
          const uint64_t mine = hit_place(raws[q]);
          const uint32_t wpos = hit_window(mine), rel = wpos - base;
          uint32_t at;
          if ((out_q >> q) & 1u) at = (mine < lo_key ? 0u : n_cluster) + (o1 < mine ? 1u : 0u) + (o2 < mine ? 1u : 0u);
          else at = before[rel >> 5] + (uint32_t)__popc(bits[rel >> 5] & ((1u << (rel & 31u)) - 1u));
          hw[at] = staged_hit(wpos, hit_rank(raws[q]));
          hc[at] = (uint16_t)(hit_contig(mine) - hc_base);
        }
      }
      return;
    }
  }
  // 32-bit keys where contig, window id and rank fit (uniform): one shuffle, a minimum, a maximum and a select per key and
  // stage.  A genome of one contig of up to 8 Mb always does.
  const uint32_t w_bits = 32u - (uint32_t)__builtin_clz(furthest | 1u);
  if (((uint64_t)(widest + 1u) << w_bits) <= (1ull << 23)) {
    uint32_t k32[E];
#pragma unroll
    for (int q = 0; q < E; ++q) {
      const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
      k32[q] = 0xffffffffu;
      if (e < nh) {
        const uint32_t c_rel = sort_key_contig(k[q]) - hc_base, wpos = sort_key_window(k[q]);
        k32[q] = (((c_rel << w_bits) | wpos) << kHitRankBits) | sort_key_rank(k[q]);
      }
    }
    bitonic_sort_lanes<E, uint32_t>(k32, lane);
#pragma unroll
    for (int q = 0; q < E; ++q) {
      const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
      if (e < nh) {
        const uint32_t cw = k32[q] >> kHitRankBits;
        hw[e] = staged_hit(cw & ((1u << w_bits) - 1u), sort_key_rank(k32[q]));
        hc[e] = (uint16_t)(cw >> w_bits);
      }
    }
    return;
  }
  bitonic_sort_lanes<E, uint64_t>(k, lane);
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
    if (e < nh) {
      hw[e] = staged_hit(sort_key_window(k[q]), sort_key_rank(k[q]));
      hc[e] = (uint16_t)(sort_key_contig(k[q]) - hc_base);
    }
  }
}

// The phases of map_segments_kernel in the order they run.  In the tools build the kernel takes one of these as an argument
// and ends after that phase (or leaves a part out): tools/map_cut.py times the phases by difference -- results wrong --
// and READS THIS LIST (name = number, // description), so the kernel and the tool cannot disagree about what a cut means.
enum MapCut : uint32_t {
  kCutHeader = 10,         // segment record and sketch loaded
  kCutStaged = 11,         // hits loaded, ordered, staged
  kCutSketchTable = 1,     // bucket table of the sketch
  kCutL1 = 2,              // L1 scan: candidates listed, none evaluated
  kCutCandidate = 3,       // candidate set-up: begins, end of the slide, hit range
  kCutGroupBounds = 4,     // seed-hit bounds of every group of begins, no rounds (nothing raises the bar: an upper estimate)
  kCutStretch = 5,         // first round only: stretch loaded, window ends found
  kCutRanks = 6,           // first round only: stretch ranked against the sketch
  kCutCoarseTable = 7,     // first round only: coarse bit table built
  kCutCoarseSearch = 8,    // first round only: window masks and coarse search
  kCutNone = 9,            // the whole kernel
  kCutNoSecondPass = 21,   // the whole kernel without the second pass of rounds with more than 64 items
  kCutNoFinePass = 22,     // the whole kernel without the fine passes
  kCutFirstGroupOnly = 23, // the whole kernel, the group of the expected optimum only (one group per candidate)
  kCutFirstRound = 24,     // first round only, complete: stretch, ranks, tables, coarse search, fine passes, fold (one round per candidate)
};
#ifdef PA_TOOLS
#define PA_MAP_CUT_PARAM , uint32_t cut
#define PA_MAP_CUT_ARG , map_cut
#define PA_CUT(k) do { if (cut == (k)) return; } while (0)
#define PA_CUT_IS(k) (cut == (k))
#else
#define PA_MAP_CUT_PARAM
#define PA_MAP_CUT_ARG
#define PA_CUT(k) do { } while (0)
#define PA_CUT_IS(k) false
#endif
// one wave per (fragment, reference genome) segment
// States a round evaluates at most, a lane each per pass (64: one pass, 128: two over the same tables), and the lane of a
// group of begins at which the expected optimum is put.  The states of the begins from lane 0 on fill the round: with 2.2
// states per begin 64 of them are the begins of 29 lanes, so the optimum is among them -- and the begins of the group before
// are 21 and more away from it, fewer of them within reach of the bar.  Measured on one box (1 000 genomes, frag_map):
// lane 10 410 ms, 14 405, 20 401, 22 402, 24 402, 27 403; two passes of 64 with the optimum at lane 32: 413.
#ifndef PA_MAP_ROUND_ITEMS
#define PA_MAP_ROUND_ITEMS 64
#endif
#ifndef PA_MAP_CENTRE_LANE
#define PA_MAP_CENTRE_LANE 20
#endif
constexpr uint32_t kRoundItems = PA_MAP_ROUND_ITEMS, kCentreLane = PA_MAP_CENTRE_LANE;
#ifndef PA_MAP_BOUND_IN_ROUND
#define PA_MAP_BOUND_IN_ROUND 1
#endif
constexpr bool kBoundInRound = PA_MAP_BOUND_IN_ROUND != 0;
#ifndef PA_MAP_L1_ONE_RUN
#define PA_MAP_L1_ONE_RUN 1  // 0 in a test build: every segment goes through the L1 scan
#endif
constexpr bool kL1OneRun = PA_MAP_L1_ONE_RUN != 0;
#ifndef PA_MAP_L1_STRAYS
#define PA_MAP_L1_STRAYS 1  // 0 in a test build: only segments that are one run and nothing else skip the L1 scan
#endif
constexpr bool kL1Strays = PA_MAP_L1_STRAYS != 0;
#ifndef PA_MAP_WAVES
#define PA_MAP_WAVES 4  // waves per SIMD the register allocation aims at: 128 VGPRs, the kernel takes 126 and spills none (80 registers / 6 waves: 0.64 s instead of 0.48 s for the 1 000-genome run)
#endif
// a segment's seed hits by their bit length, for the event counters that come in seven slots: <= 7, 8-15, 16-31, ..., 256 and more
__device__ __forceinline__ uint32_t seed_hits_slot(uint32_t nh) {
  const uint32_t bits = 32u - (uint32_t)__builtin_clz(nh | 1u);
  return min(6u, bits > 3u ? bits - 3u : 0u);
}
// kAllStaged: the launch holds only segments of at most hit_cap hits (the bucketed path's list of short segments), so
// every access to a hit is an LDS read and the choice is not made per access.
template <uint32_t kRefCap, bool kAllStaged>
__global__ __launch_bounds__(64, PA_MAP_WAVES) void map_segments_kernel(
    uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint4 *__restrict__ seg_rec, uint32_t n_segs,
    bool presorted, const uint32_t *__restrict__ q_hash, const uint32_t *__restrict__ q_tab, const uint32_t *__restrict__ frag_genome_local, uint32_t frag_len,
    uint32_t count_windows, const uint32_t *__restrict__ tab_min_shared,
    const uint32_t *__restrict__ contig_mini_off, const uint32_t *__restrict__ contig_bucket_off,
    const uint32_t *__restrict__ bucket_first, const uint32_t *__restrict__ mini_hash,
    const uint32_t *__restrict__ mini_wpos, const int32_t *__restrict__ prev_same,
    const uint32_t *__restrict__ contig_bin_off, uint64_t table_stride, unsigned long long *__restrict__ table,
    uint32_t *__restrict__ run_g, uint32_t s_cap, uint32_t hit_cap PA_MAP_CUT_PARAM) {
  extern __shared__ uint32_t eval_lds[];
  // the short-segment launch stages up to kHitCapSmall hits, the other one up to kHitCap (what the host passes as hit_cap)
  constexpr uint32_t kStageCap = kAllStaged ? (uint32_t)kHitCapSmall : (uint32_t)kHitCap;
  const EvalShared sh = eval_carve(eval_lds, s_cap, kStageCap, kRefCap);
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= n_segs) return;
  // (One workgroup per segment.  Waves that go through many segments each -- no launch per segment -- were tried in round 6:
  // the loop keeps the kernel's arguments and the scan state alive across segments, 15 vector registers spilled, mapping
  // 430 ms against 368; profiles/README.md.)
#ifdef PA_MAP_STATS  // event counts of the mapping kernel in run_g[0 .. 15] (tools: -DPA_MAP_STATS, PA_FRAGANI_TRACE=1)
#define PA_STAT(slot, v) do { const uint32_t pa_stat_v = (uint32_t)(v); if (lane == 0) atomicAdd(&run_g[slot], pa_stat_v); } while (0)  // (v may hold a ballot: every lane evaluates it)
#else
#define PA_STAT(slot, v) do { } while (0)
  (void)run_g;
#endif
  const uint4 rec0 = seg_rec[3 * (uint64_t)blockIdx.x], rec1 = seg_rec[3 * (uint64_t)blockIdx.x + 1], rec2 = seg_rec[3 * (uint64_t)blockIdx.x + 2];  // segment_records_kernel
  const uint32_t a0 = rec0.x, nh = rec0.y, f = rec0.z, s = rec0.w, mh = rec1.x;
  const int32_t unseeded = (int32_t)rec1.z;  // hashes of the sketch whose reference occurrences are not all seed hits (frequency cut)
  if (s == 0) return;  // no sketch, or fewer seed hits than any L1 run needs
  PA_STAT(0, 1);   // segments that reach L1
  PA_STAT(25 + seed_hits_slot(nh), 1);  // ... by their seed hits
  PA_STAT(1, nh);  // their seed hits
  // segments of up to kHitCap hits are staged in LDS; larger ones (repeats: rRNA operons, IS elements)
  // are read in place from the sorted hit arrays
  // contigs are kept relative to the reference genome's first one, window ids of the query as 16 bits: the
  // host takes this kernel only when both fit
  const uint32_t hc_base = rec1.y;
  const bool staged = kAllStaged || nh <= kStageCap;
  (void)hit_cap;
  auto HW = [&](uint32_t i) -> uint32_t { return staged ? sh.hw[i] >> 8 : hit_window(keys[a0 + i]); };
  // "the window id of hit i is below w" without the shift (the searches of the bounds ask nothing else)
  // (window ids stay below 2^24 - 1: contigs are shorter than 2^24)
  auto HW_below = [&](uint32_t i, uint32_t w) -> bool {
    return staged ? sh.hw[i] < ((w < kHitWindowMax ? w : kHitWindowMax) << 8) : hit_window(keys[a0 + i]) < w;
  };
  auto HC = [&](uint32_t i) -> uint32_t {
    return staged ? hc_base + sh.hc[i] : hit_contig(keys[a0 + i]);
  };
  // The fragment's sketch, 16 bytes per lane and turn (s_cap is a multiple of 64; a row of q_hash holds kQMax hashes).  The
  // It waits in registers (two turns per lane at most) while the hits are loaded and ordered: the loads are in flight together
  // instead of one after the other.
  // The bucket table of the fragment's sketch (query_sketch_kernel makes it, once per fragment: some twenty-five reference
  // genomes share it) waits in registers likewise.
  const uint4 qtab0 = reinterpret_cast<const uint4 *>(q_tab + (uint64_t)f * (kQtBuckets / 2u))[lane];
  uint4 sketch0 = make_uint4(0u, 0u, 0u, 0u), sketch1 = make_uint4(0u, 0u, 0u, 0u);  // (kQMax / 4 = 128 turns of 16 bytes at most: two per lane)
  {
    const uint4 *src4 = reinterpret_cast<const uint4 *>(q_hash + (uint64_t)f * kQMax);
    if (lane < s_cap / 4u) sketch0 = src4[lane];
    if (lane + 64u < s_cap / 4u) sketch1 = src4[lane + 64u];
  }
  static_assert(kQMax <= 512, "two 16-byte turns per lane hold a sketch");
  PA_CUT(kCutHeader);  // segment header and sketch
  // The bounds of the reference genome's FIRST contig in the minimizer and bucket arrays -- where a one-contig genome's
  // candidates all lie -- come with the segment's record.  And when all hits lie on that contig, the buckets the first
  // candidate's range can start in are known before the hits are ordered: a range starts at (its mh-th hit) + 1 - fragLen, a
  // few window ids past (the smallest hit) + 1 - fragLen.  Four entries of the bucket index from there on are asked for now,
  // with a VECTOR load (a scalar one would share its counter with the LDS traffic of the ordering and be waited for at once),
  // and are there when the candidate is set up: one more memory round trip off its path.
  const uint32_t c0_m1 = rec2.x, c0_bb = rec2.y, c0_b1 = rec2.z;
  uint32_t spec_bk0 = 0xffffffffu, spec_first = 0;  // first bucket asked for (none); lane j: bucket_first of bucket spec_bk0 + j (clamped to the closing entry)
  auto ask_buckets = [&](uint32_t nearest, uint32_t widest) {
    if (widest != 0u) return;  // hits on other contigs than the first
    const uint32_t nb0 = c0_b1 - c0_bb - 1u;
    spec_bk0 = min(l1_range_start(nearest, frag_len) >> kBucketShift, nb0);
    spec_first = bucket_first[c0_bb + min(spec_bk0 + (lane & 3u), nb0)];
  };
  if (staged) {
    if (presorted) {
      for (uint32_t i = lane; i < nh; i += 64) {  // hits ordered as a whole: the fragment on top of the key, the rank in the payload
        const uint64_t key = keys[a0 + i];
        sh.hw[i] = staged_hit(hit_window(key), vals[a0 + i] & ((1u << kHitRankBits) - 1u));
        sh.hc[i] = (uint16_t)(hit_contig(key) - hc_base);
      }
    } else {
      // the bucketing pass leaves a segment's hits in no particular order: ordered in registers on their way to LDS
      if (nh <= 64u) stage_hits_sorted<1>(keys + a0, nh, hc_base, lane, sh.hw, sh.hc, sh.tab, ask_buckets);
      else if (nh <= 128u) stage_hits_sorted<2>(keys + a0, nh, hc_base, lane, sh.hw, sh.hc, sh.tab, ask_buckets);
      else if (kAllStaged || nh <= 256u) stage_hits_sorted<4>(keys + a0, nh, hc_base, lane, sh.hw, sh.hc, sh.tab, ask_buckets);
      else if constexpr (!kAllStaged) stage_hits_sorted<8>(keys + a0, nh, hc_base, lane, sh.hw, sh.hc, sh.tab, ask_buckets);
    }
  }
  if (lane < s_cap / 4u) reinterpret_cast<uint4 *>(sh.qh)[lane] = sketch0;
  if (lane + 64u < s_cap / 4u) reinterpret_cast<uint4 *>(sh.qh)[lane + 64u] = sketch1;
  PA_CUT(kCutStaged);  // hits staged in order
#ifdef PA_MAP_STATS
  if (staged && nh >= 6u) {  // how the hits lie: all within kCountSpan window ids on one contig (ordered by counting), or all but one or two
    __syncthreads();
    auto fits = [&](uint32_t a, uint32_t b) { return sh.hc[a] == sh.hc[b] && (sh.hw[b] >> 8) - (sh.hw[a] >> 8) < kCountSpan; };
    const bool all = fits(0u, nh - 1u);
    const bool but_one = !all && (fits(1u, nh - 1u) || fits(0u, nh - 2u));
    const bool but_two = !all && !but_one && (fits(2u, nh - 1u) || fits(1u, nh - 2u) || fits(0u, nh - 3u));
    PA_STAT(43, all ? 1u : 0u);
    PA_STAT(44, but_one ? 1u : 0u);
    PA_STAT(45, but_two ? 1u : 0u);
  }
#endif
  // (sh.cnt is zeroed where the cooperative evaluation uses it: the bit tables of the rounds live in the same memory)
  if (lane < (uint32_t)kQMax / 32) sh.matched[lane] = 0;
  // The fragment's hashes bucketed by their top kQtBits bits: a reference minimizer's rank among them is then the
  // bucket's first rank plus a search among the bucket's few hashes (a fraction of a hash per bucket on average)
  // instead of log2(s) dependent LDS reads.  Buckets with more than 63 hashes (degenerate sketches) switch it off.
  uint32_t qsteps = 0;  // halving steps of the in-bucket search; 0xffffffff: table not usable
  {
    reinterpret_cast<uint4 *>(sh.qt)[lane] = qtab0;
    uint32_t most = max(max(qtab0.x >> 26, (qtab0.x >> 10) & 63u), max(qtab0.y >> 26, (qtab0.y >> 10) & 63u));
    most = max(most, max(max(qtab0.z >> 26, (qtab0.z >> 10) & 63u), max(qtab0.w >> 26, (qtab0.w >> 10) & 63u)));
    most = pa_dev::wave_max_dpp(most);
    qsteps = most >= 63u ? 0xffffffffu : (most ? 32u - (uint32_t)__builtin_clz(most) : 0u);  // (the counts come clamped to 63)
  }
  __syncthreads();

  // number of hits whose (contig, window id) is below (c, w0) and below (c, w1) -- the hits are in that order, so these
  // are the bounds of the hits on contig c with window id in [w0, w1).  Uniform arguments: the wave counts side by
  // side, every lane its own hits, instead of searching (no chain of dependent reads).
  auto hit_range = [&](uint32_t c, uint32_t w0, uint32_t w1, uint32_t &below0, uint32_t &below1) {
    const uint64_t k0 = ((uint64_t)c << 32) | w0, k1 = ((uint64_t)c << 32) | w1;
    uint32_t n0 = 0, n1 = 0;
    for (uint32_t chunk = 0; chunk < nh; chunk += 64) {
      const uint32_t i = min(chunk + lane, nh - 1u);
      const uint64_t k = ((uint64_t)HC(i) << 32) | HW(i);
      const bool in = chunk + lane < nh;
      n0 += (uint32_t)__popcll(__ballot(in & (k < k0)));
      n1 += (uint32_t)__popcll(__ballot(in & (k < k1)));
    }
    below0 = n0;
    below1 = n1;
  };
  // first hit index in [lo, lo + 2^steps) and below hi whose window id is >= w, inside an index range that lies on one
  // contig; `steps` is uniform (the longest range any lane has), every lane takes that many halvings without a branch
  // (Two halvings per turn with the three hits they can ask about read side by side -- half the chain of dependent LDS
  // reads, half as many again in all -- was tried for this search and the one for the window ends: 400 against 397 ms.)
  auto hit_lower_bound_w = [&](uint32_t lo, uint32_t hi, uint32_t w, uint32_t steps) -> uint32_t {
    uint32_t pos = lo;  // hits [lo, pos) are below w
    for (uint32_t step = steps ? 1u << (steps - 1u) : 0u; step > 0u; step >>= 1) {
      const uint32_t idx = pos + step;
      const bool ok = (idx <= hi) & HW_below(min(idx, nh) - 1u, w);
      pos = ok ? idx : pos;
    }
    return pos;
  };

  // One over-long window (more than kRefCap minimizers: low-complexity or N-riddled sequence) straight from HBM,
  // the whole wave on it: reference-only hashes are counted per query-rank gap, matches set a bit, one scan
  // gives how many of the fragment's smallest hashes sit in the bottom-s of the union.  Uniform result.
  auto eval_window_coop = [&](uint32_t b0, uint32_t e) -> uint32_t {
    for (uint32_t t = b0 + lane; t < e; t += 64) {
      if (prev_same[t] >= (int32_t)b0) continue;  // the same hash already counted inside this window
      const uint32_t h = mini_hash[t];
      const uint32_t r = lower_bound_u32(sh.qh, 0, s, h);
      if (r < s && sh.qh[r] == h) atomicOr(&sh.matched[r >> 5], 1u << (r & 31u));
      else atomicAdd(&sh.cnt[r], 1u);
    }
    __syncthreads();
    uint32_t x;
    {
      const uint32_t per = s / 64u + 1u;  // buckets per lane: s + 1 of them
      uint32_t local_sum = 0;
      for (uint32_t q = 0; q < per; ++q) {
        const uint32_t r = lane * per + q;
        if (r <= s) local_sum += sh.cnt[r];
      }
      uint32_t prefix = wave_excl_scan(local_sum, lane), acc = 0;
      for (uint32_t q = 0; q < per; ++q) {
        const uint32_t r = lane * per + q;
        if (r <= s) {
          const uint32_t cr = sh.cnt[r];
          sh.cnt[r] = 0;  // ready for the next use
          const int32_t room = (int32_t)s - (int32_t)r - (int32_t)prefix;
          if (room > 0) acc += cr < (uint32_t)room ? cr : (uint32_t)room;
          prefix += cr;
        }
      }
      x = wave_sum(acc);
    }
    const uint32_t take = s - x;  // the `take` smallest query hashes are in the bottom-s of the union
    uint32_t shared = 0;
    if (lane < (uint32_t)kQMax / 32) {
      const uint32_t lo_bit = lane * 32u;
      uint32_t m = sh.matched[lane];
      sh.matched[lane] = 0;
      if (take <= lo_bit) m = 0;
      else if (take < lo_bit + 32u) m &= (1u << (take - lo_bit)) - 1u;
      shared = __popc(m);
    }
    shared = wave_sum(shared);
    __syncthreads();
    return shared;
  };

  PA_CUT(kCutSketchTable);  // staging, sort, bucket table
  // The best mapping so far lives in LDS (sh.scan[16..19]: it is looked at once per candidate, and values kept in
  // registers across the whole kernel were spills): shared minimizers; contig; window ids of the first minimizers of its
  // first and of its last optimal state.
  // kBestT: how many of the fragment's smallest hashes lie in the bottom-s of the union with the best window so far (T
  // below) -- the pivot rank of the tight bound; 0xffffffff: not known.
  // kLmaskPivot: the pivot sh.lmask stands for (the hits are the segment's: the bits outlive a candidate).
  enum { kBestShared = 16, kBestC, kBestFirst, kBestLast, kBestT, kLmaskPivot };
  constexpr uint32_t kNoT = 0xffffffffu;
  if (lane == 0) {
    sh.scan[kBestShared] = 0xffffffffu;  // -1
    sh.scan[kBestC] = 0xffffffffu;
    sh.scan[kBestT] = kNoT;
    sh.scan[kLmaskPivot] = kNoT;
  }
  uint32_t half0 = 1;
  while (2u * half0 <= s) half0 *= 2u;

  // ---- L2, the exact slide (oracle/fragani_oracle.c, L2 rule 2).  The window at position i of the candidate's contig
  // holds the minimizers of the reference windows [i, i + count_windows): from b = the last minimizer recorded at or
  // before i (still active in window i) to e = the first one recorded at or after i + count_windows.  The slide starts
  // at the first minimizer of the candidate range and ends as soon as e reaches the first minimizer at or past
  // rangeEnd + fragLen (or the contig's end): positions up to i_max = (window id of the minimizer before that) -
  // count_windows.  A STATE is a maximal run of positions with the same (b, e); its position is the window id of its first
  // minimizer b (Mashmap's), and per candidate the mapping position is the mean of the positions of the first and of the
  // last state with the most shared minimizers.
  // One lane per begin b, as a group of 64 begins is taken up: its states are the ends e from "first minimizer at or
  // after P[b] + count_windows" to "first at or after min(P[b+1] - 1, i_max) + count_windows", usually one or two.  In a
  // round the states of the group's pending begins are spread over the lanes in slide order (up to 64 of them: ITEMS),
  // the stretch of minimizers they cover (~300) is ranked against the fragment's hashes once and entered into bit tables
  // over (query rank x stretch position), and every lane finds, by two short searches over rows of those tables, how many
  // of the fragment's smallest hashes lie in the bottom-s of the union with its own window and how many of them the window
  // holds.  Begins none of whose windows can hold as many seed hits as the best so far shares are never evaluated.
  auto process_candidate = [&](uint32_t c, uint32_t cs, uint32_t ce, uint32_t first_hit_w) __attribute__((always_inline)) {
    PA_CUT(kCutL1);  // L1 only
    const int32_t best_shared = (int32_t)__builtin_amdgcn_readfirstlane((int)sh.scan[kBestShared]);  // (fixed while this candidate is evaluated)
    const bool on_first = c == hc_base;
    const uint32_t m1 = on_first ? c0_m1 : contig_mini_off[c + 1];
    const uint32_t bb = on_first ? c0_bb : contig_bucket_off[c], nb = (on_first ? c0_b1 : contig_bucket_off[c + 1]) - bb - 1;
    // the first begin and the batch of window ids after it (slide_first_begin), from the start of the range's bucket
    uint32_t b_lo, origin;
    uint32_t wpv[kStartBatch];
    {
      uint32_t bk = cs >> kBucketShift;
      if (bk >= nb) bk = nb;
      uint32_t lo, hi;
      if (on_first && bk >= spec_bk0 && bk - spec_bk0 < 3u) {  // asked for while the hits were ordered (spec_bk0 is 0xffffffff where nothing was)
        lo = (uint32_t)__builtin_amdgcn_readlane((int)spec_first, (int)(bk - spec_bk0));
        hi = bk < nb ? (uint32_t)__builtin_amdgcn_readlane((int)spec_first, (int)(bk - spec_bk0 + 1u)) : lo;
      } else {
        lo = bucket_first[bb + bk];
        hi = bk < nb ? bucket_first[bb + bk + 1] : lo;
      }
      slide_first_begin(mini_wpos, m1, lo, hi, cs, lane, b_lo, origin, wpv);
    }
    if (b_lo >= m1) return;
    uint32_t b_hi = 0xffffffffu, at = 0xffffffffu, i_max;
    uint32_t h_lo, h_hi;  // the seed hits any window of this candidate can hold: hits on contig c with window id in [cs, i_max + count_windows)
    uint32_t est = first_hit_w;  // where the optimum is expected
    {
      // (map_sparse_kernel has a copy of this block up to b_hi: a change here is a change there)
      // where the slide ends: the window's end may not reach the first minimizer at or past rangeEnd + fragLen (or the
      // contig's end); z = the window id of the minimizer before that one -- the largest of the batch below the limit when
      // the batch reaches the limit (it nearly always does: a candidate range spans at most two fragment lengths)
      const uint32_t limit = ce + frag_len;
      uint32_t z = 0;
      bool reached = false;
#pragma unroll
      for (int q = 0; q < kStartBatch; ++q) {
        z = wpv[q] < limit ? max(z, wpv[q]) : z;
        reached = reached || wpv[q] >= limit;
      }
      // window id of the first begin (the minimizers of the batch before it lie before the range: below every limit asked here)
      const uint32_t shift = b_lo - origin;  // <= 64
      const uint32_t wp_lo = shift < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)wpv[0], (int)shift) : (uint32_t)__builtin_amdgcn_readfirstlane((int)wpv[1]);
      if (wp_lo >= limit) return;  // no minimizer between the range's start and the limit
      if (__any(reached)) {
        z = pa_dev::wave_max_dpp(z);
      } else {
        const uint32_t last_end = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, limit);
        z = mini_wpos[last_end - 1];
      }
      if (z < wp_lo + count_windows) return;  // the first window's end is already at the limit: nothing is evaluated
      i_max = z - count_windows;
      hit_range(c, cs, i_max + count_windows, h_lo, h_hi);
      // Where the optimum is expected: a fragment that maps at P leaves its hits in [P, P + count_windows), so P is about the
      // middle of the candidate's first and last hit less half a window -- for a diverged pair, whose first matching minimizer
      // sits anywhere in the fragment, a better guess than the first hit itself (never past it: the optimum holds hits).
      if (h_hi > h_lo) {
        const uint32_t mid = (HW(h_lo) + HW(h_hi - 1u)) / 2u, half = count_windows / 2u;
        est = min(first_hit_w, max(cs, mid > half ? mid - half : 0u));
      }
      // the first begin past the slide's last position and the first one at the expected optimum: every lane the first of
      // its own eight, then the minimum over the wave (the window ids ascend with the begin index)
      uint32_t my_over = 0xffffffffu, my_reach = 0xffffffffu;
#pragma unroll
      for (int q = kStartBatch - 1; q >= 0; --q) {
        my_over = wpv[q] > i_max ? (uint32_t)q * 64u + lane : my_over;
        my_reach = wpv[q] >= est ? (uint32_t)q * 64u + lane : my_reach;
      }
      const uint32_t w_over = pa_dev::wave_min_dpp(my_over), w_reach = pa_dev::wave_min_dpp(my_reach);
      if (w_over != 0xffffffffu) b_hi = origin + w_over;
      if (w_reach != 0xffffffffu) at = origin + w_reach;
    }
    if (b_hi == 0xffffffffu) b_hi = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, i_max + 1u);  // a range of more than 512 begins
    if (at == 0xffffffffu) at = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, est);
    if (b_lo >= b_hi) return;
    PA_STAT(2, 1);  // candidates with begins
#ifdef PA_MAP_STATS
    // the work model's units (profiles/README.md): the minimizers of the candidate's range, each of which a perfect bound
    // still has to look at once (from the first begin to the end of the last window), and -- below -- the states that tie the
    // candidate's optimum, which no bound can spare
    PA_STAT(32, wpos_lower_bound(mini_wpos, bucket_first, bb, nb, i_max + count_windows) - b_lo);
    uint32_t stat_ties = 0;
    int32_t stat_best_of_candidate = -1;
    int32_t stat_bar = -1000;
#endif
    int32_t c_best = -1;
    uint32_t c_first = 0, c_last = 0;
    // T of this candidate's best state so far, until there is one that of the fragment's best mapping so far: the pivot of the tight bound
    uint32_t pivot_T = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.scan[kBestT]);
    // The begins are taken up in groups of 64 (one lane each), tiled so that the begin at the expected optimum sits in the
    // MIDDLE of its group (the tiles start `pad` begins before the first begin): that group goes first and sets the bar, and
    // with the tight bound below a begin more than a few matches away from the optimum is dropped -- the optimum in the
    // middle of the first group, the other groups are passed over or end with the bound.  (With the count of seed hits as
    // the only bound the tiling did not matter: the begins that passed spanned two groups by their number.)
    // A begin matters only if one of its windows can hold min_shared minimizers of the fragment (less is never reported)
    // and reach the best so far: first asked per group (seed hits between its first begin and the end of its last
    // window), then per begin.
    // (Tried in round 6: the tight bound asked for a neighbouring group against the stretch the group before has left in LDS,
    // before the group loads its own.  That stretch holds 75-100 % of such a begin's narrowest window, and the bound needs
    // nearly all of it: a quarter of the groups ended there, the others paid the test twice -- mapping 373 ms against 353.)
    const uint32_t pad = (kCentreLane - ((at - b_lo) & 63u)) & 63u;
    const uint32_t tile0 = b_lo - pad;  // (may wrap below zero: begins before b_lo take no part)
    const uint32_t n_groups = (b_hi - tile0 + 63u) / 64u;
    const int32_t floor_bar = (int32_t)rec1.w;  // (tab_min_shared[s], looked up by segment_records_kernel)
    const uint32_t h_steps = 32u - (uint32_t)__builtin_clz(h_hi - h_lo + 1u);  // 2^steps > the number of hits: enough halvings
    PA_CUT(kCutCandidate);  // candidate set-up
    const uint32_t g_first = min((at - tile0) / 64u, n_groups - 1u);
    for (uint32_t gi = 0; gi < n_groups; ++gi) {
      const uint32_t g = gi == 0 ? g_first : (gi <= g_first ? gi - 1u : gi);
      if (gi > 0 && PA_CUT_IS(kCutFirstGroupOnly)) break;  // (timing experiment: the group of the first seed hit only; results wrong)
      const uint32_t sb = tile0 + g * 64u;
      const uint32_t b = sb + lane;
      const bool has = b >= b_lo && b < b_hi;
      const WidestWindow ww = begin_widest_window(mini_wpos, m1, b, has, i_max, count_windows);
      const uint32_t wp = ww.wp, wp_next = ww.wp_next, w_end = ww.w_end;
      // what a window must reach to matter (ties matter) -- in SEED HITS: a window shares no more than the seed hits it holds
      // plus the sketch's hashes that the frequency cut took out of the seeds (nearly always none)
      const int32_t bar = shared_bar(c_best, best_shared, floor_bar) - unseeded;
      // A window with `bar` of the candidate's hits ends after the bar-th hit and does not begin after the bar-th hit
      // from the end: groups without such a begin are passed over before any counting
      if (bar > 0) {
        if ((uint32_t)bar > h_hi - h_lo) break;  // no window of this candidate holds that many (the bar only rises)
        const uint32_t w_after = HW(h_lo + (uint32_t)bar - 1u), w_upto = HW(h_hi - (uint32_t)bar);
        if (!__any(has && w_end > w_after && wp <= w_upto)) continue;
      }
      // Seed hits inside the begin's widest window: every occurrence of every query hash is a hit (but for the hashes the
      // frequency cut took out: `unseeded`, allowed for in the bar), so no window shares more.  Only "at least b of them" is ever asked: with i0 = the first hit at or after the begin, that is "hit
      // i0 + b - 1 exists and lies before the window's end" -- one search and one read instead of two searches.
      const uint32_t i0 = hit_lower_bound_w(h_lo, h_hi, wp, h_steps);
      auto holds_hits = [&](int32_t b) -> bool {
        const uint32_t idx = i0 + (uint32_t)max(b, 1) - 1u;
        return has & (idx < h_hi) & HW_below(min(idx, nh - 1u), w_end);
      };
      bool pending = bar > 0 ? holds_hits(bar) : has;
      if (PA_CUT_IS(kCutGroupBounds)) pending = false;  // seed-hit bounds of every group
      PA_STAT(3, 1);                              // groups of 64 begins
      PA_STAT(4, __popcll(__ballot(pending)));    // begins that pass the seed-hit bound
      uint32_t e_next = 0;  // end (minimizer index) of the begin's next state; 0: none of its states has been evaluated yet
      while (__any(pending)) {
        PA_STAT(5, 1);  // rounds
        PA_STAT(18 + seed_hits_slot(nh), 1);  // ... by the segment's seed hits
        const uint32_t first_lane = (uint32_t)__builtin_ctzll(__ballot(pending));
        const uint32_t base = sb + first_lane;  // stretch = minimizers [base, base + n)
        const uint32_t n = min(m1 - base, kRefCap);
        constexpr int kPer = (int)(kRefCap / 64u);
        uint32_t hh[kPer];
        uint32_t dup_q = 0;  // bit q: the lane's q-th entry repeats a hash met earlier in the stretch
        __syncthreads();
        // the stretch: hashes into registers, window ids (relative to the first) and duplicate links into LDS.  The first
        // entry's window id is what lane 0 loads first: taken from there (asked for by itself beforehand it was a scalar load
        // the whole batch of vector loads waited for, in every round)
        uint32_t w_raw[kPer];
        int32_t p_raw[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) {  // loads without a branch (beyond the stretch its last entry, discarded), all of them before any is looked at
          const uint32_t t = base + min((uint32_t)q * 64u + lane, n - 1u);
          w_raw[q] = mini_wpos[t];
          hh[q] = mini_hash[t];
          p_raw[q] = prev_same[t];
        }
        const uint32_t wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)w_raw[0]);
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
          const uint32_t x = (uint32_t)q * 64u + lane;
          const bool in = x < n;
          const uint32_t h = hh[q], dw = w_raw[q] - wbase;
          const int32_t pv = p_raw[q];
          hh[q] = in ? h : 0u;
          // the same hash earlier in the stretch (position + 1): a window keeps this occurrence only if it starts after that one
          const uint32_t p1 = (in && pv >= (int32_t)base) ? (uint32_t)(pv - (int32_t)base) + 1u : 0u;
          sh.prev[x] = (uint16_t)p1;
          dup_q |= (p1 ? 1u : 0u) << q;
          // (0xffff: far beyond any window of this stretch.  That holds for every call the host accepts: the winnowing window is at
          // most 64, so a fragment is at most ~8 000 residues (pa_fragani_window), a window ~8 000 window ids, and the 64 begins of a
          // group lie inside a candidate range whose gaps are shorter than a fragment: the ends a lane asks for stay well below
          // 0xfffe.  map_sparse_kernel, which sees segments this kernel never does, tests it and hands the segment on.)
          sh.ref_w[x] = (uint16_t)((dw > 0xfffeu || !in) ? 0xffffu : dw);
        }
        __syncthreads();
        // per begin: the ends of its first and last state inside the stretch, and how many of its remaining states the
        // stretch holds (a state with end x is held when entry x is in the stretch, or the stretch runs to the contig's end)
        const bool at_end = base + n == m1;
        const uint32_t lim = at_end ? n : n - 1u;
        const bool lane_on = pending && lane >= first_lane;  // (pending lanes are at or after first_lane by definition)
        uint32_t cnt = 0, xs0 = 0, xe_lo = 0, xe_hi = 0, top = 0;
        bool hi_known = false;
        {
          auto first_at_or_after = [&](uint32_t lo, uint32_t target) -> uint32_t {
            uint32_t hi = n;
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)sh.ref_w[mid] < target) lo = mid + 1; else hi = mid; }
            return lo;
          };
          const bool lane_has = has && lane >= first_lane;
          if (lane_has) xe_lo = first_at_or_after(min(b - base, n), wp + count_windows - wbase);
          // the last state of a begin ends where the first state of the next begin does, or one entry before that when
          // this very entry comes in at the next begin's position (the next lane has searched for it); the last begin of
          // the slide and the last lane search themselves
          const uint32_t xe_lo_next = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(min(lane + 1u, 63u) << 2), (int)xe_lo);
          // (that ONE lane's search is the whole wave's: the 64 entries from its first end on are compared at once -- the entries
          // ascend, those below the target are a prefix -- and only a begin with more than 64 states searches)
          const bool by_neighbour = lane < 63u && b + 1u < b_hi;
          uint32_t xe_own = 0;
          {
            const uint64_t own = __ballot(lane_on && !by_neighbour);
            if (own) {
              const int src = __builtin_ctzll(own);
              const uint32_t lo0 = (uint32_t)__builtin_amdgcn_readlane((int)xe_lo, src), tgt = (uint32_t)__builtin_amdgcn_readlane((int)(w_end - wbase), src);
              const uint32_t x = lo0 + lane;
              const uint64_t lt = __ballot(x < n && (uint32_t)sh.ref_w[min(x, kRefCap - 1u)] < tgt);
              xe_own = lt == ~0ULL ? first_at_or_after(lo0 + 64u, tgt) : lo0 + (uint32_t)__popcll(lt);
            }
          }
          if (lane_on) {
            if (by_neighbour) {
              const bool comes_in_there = xe_lo_next > 0u && (uint32_t)sh.ref_w[xe_lo_next - 1u] == wp_next + count_windows - 1u - wbase;
              xe_hi = xe_lo_next - (comes_in_there ? 1u : 0u);
            } else {
              xe_hi = xe_own;
            }
            xs0 = e_next ? e_next - base : xe_lo;
            top = min(xe_hi, lim);
            cnt = xs0 <= top ? top - xs0 + 1u : 0u;  // states of the begin the stretch holds
            hi_known = xe_hi < n || at_end;
          }
        }
        // ---- The tight bound.  With T = the number of the fragment's smallest hashes that lie in the bottom-s of the union
        // with a window (rank r is one of them iff r + c(r) < s, c(r) = the window's reference-only hashes below the
        // fragment's hash of rank r), the window shares its matches of rank < T.  For ANY pivot rank r0: c(r) >= c(r0) from
        // r0 on, hence T <= max(r0, s - c(r0)), and
        //     shared <= matches of rank < r0  +  min(matches of rank >= r0, max(0, s - r0 - c(r0))).
        // The matches of a begin's windows are seed hits, and a hit knows the rank of its hash: those below r0 among the
        // hits inside the begin's WIDEST window come from a bit per hit and two prefix counts (sh.lmask).  c(r0) is bounded
        // from below over the begin's NARROWEST window: stretch entries there whose hash is below the fragment's hash of
        // rank r0 -- entries that repeat a hash of the stretch left out, so that no hash counts twice -- less the hits below
        // r0 (they are such entries; taking those of the widest window only lowers the count).  With r0 = T of the best
        // window so far the bound is what the window would share if its reference-only hashes were as dense as that
        // window's: begins a few matches away from the optimum fail it, where the count of seed hits alone lets windows a
        // third of a fragment away pass (a window shares ~0.7 of its hits).  Asked before the stretch is ranked and the bit
        // tables are built -- the expensive part of a round --, for every pending begin at once.  Not asked when the
        // frequency cut took hashes of the sketch out of the seeds (their matches are not among the hits) and for segments
        // whose hits are not staged.
        // the bits of sh.lmask / sh.lpre for pivot r0 (kept while the pivot stays)
        auto lmask_for = [&](uint32_t r0) {
          if ((uint32_t)__builtin_amdgcn_readfirstlane((int)sh.scan[kLmaskPivot]) != r0) {  // the bits stand for another pivot
            for (uint32_t chunk = 0; chunk <= nh; chunk += 64) {
              const uint32_t i = chunk + lane;
              const uint64_t lm = __ballot(i < nh && (sh.hw[min(i, nh - 1u)] & 0xffu) < (r0 >> 1));
              if (lane == 0) { sh.lmask[chunk / 32u] = (uint32_t)lm; sh.lmask[chunk / 32u + 1u] = (uint32_t)(lm >> 32); }
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t n_words = 2u * (nh / 64u) + 2u;
            const uint32_t pc = lane < n_words ? (uint32_t)__popc(sh.lmask[min(lane, kLmaskWords - 1u)]) : 0u;
            const uint32_t ex = pa_dev::wave_incl_scan_dpp(pc) - pc;
            if (lane < n_words) sh.lpre[lane] = ex;
            if (lane == 0) sh.scan[kLmaskPivot] = r0;
            __builtin_amdgcn_wave_barrier();
          }
        };
        // prefix counts over the 2 kPer words of sh.matched (stretch entries below the pivot hash) into sh.tab, and the test
        // itself for the lanes `who`: true where no window of the begin can reach the bar
        auto tight_fails = [&](bool who, uint32_t r0) -> bool {
          uint32_t *bw = sh.matched;
          __builtin_amdgcn_wave_barrier();
          {
            const uint32_t pc = lane < 2u * (uint32_t)kPer ? (uint32_t)__popc(bw[min(lane, 2u * (uint32_t)kPer - 1u)]) : 0u;
            const uint32_t ex = pa_dev::wave_incl_scan_dpp(pc) - pc;
            if (lane < 2u * (uint32_t)kPer) sh.tab[lane] = ex;
          }
          __builtin_amdgcn_wave_barrier();
          auto below_upto = [&](uint32_t x) -> uint32_t {  // entries [0, x) below the pivot hash, x <= n
            const uint32_t w = min(x >> 5, 2u * (uint32_t)kPer - 1u), bits = x - (w << 5);
            const uint32_t m = bits >= 32u ? 0xffffffffu : (1u << bits) - 1u;
            return sh.tab[w] + (uint32_t)__popc(bw[w] & m);
          };
          auto hits_below = [&](uint32_t i) -> uint32_t {  // hits [0, i) whose rank lies below the pivot
            const uint32_t w = i >> 5;
            return sh.lpre[w] + (uint32_t)__popc(sh.lmask[w] & ((1u << (i & 31u)) - 1u));
          };
          const int32_t bar_full = shared_bar(c_best, best_shared, floor_bar);
          bool fails = false;
          if (who) {
            const uint32_t cb = below_upto(min(xe_lo, n)) - below_upto(min(b - base, n));
            const uint32_t i1 = hit_lower_bound_w(i0, h_hi, w_end, h_steps);
            const uint32_t mlow = hits_below(i1) - hits_below(i0), mhigh = (i1 - i0) - mlow;
            const uint32_t c2 = cb > mlow ? cb - mlow : 0u;
            const uint32_t room = s - r0 > c2 ? s - r0 - c2 : 0u;
            fails = (int32_t)(mlow + min(mhigh, room)) < bar_full;
          }
          return fails;
        };
        {
          if (staged && unseeded == 0 && pivot_T != kNoT) {
            const uint32_t r0 = min(pivot_T, s - 1u) & ~1u;  // even: a staged hit keeps its rank without the lowest bit
            lmask_for(r0);
            const uint32_t ph = sh.qh[r0];
            uint32_t *bw = sh.matched;   // 2 kPer words: stretch entries below the pivot hash; their prefix counts in sh.tab
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
              const uint32_t x = (uint32_t)q * 64u + lane;
              const uint64_t mb = __ballot((x < n) & (hh[q] < ph) & (((dup_q >> q) & 1u) == 0u));
              if (lane == 0) { bw[2 * q] = (uint32_t)mb; bw[2 * q + 1] = (uint32_t)(mb >> 32); }
            }
            const bool fails = tight_fails(lane_on, r0);
            PA_STAT(16, __popcll(__ballot(fails)));  // begins the tight bound drops
            pending = pending && !fails;
            if (!((__ballot(pending) >> first_lane) & 1ULL)) {  // the stretch was loaded for a begin that is gone: the next one, if any
              PA_STAT(17, 1);  // rounds that end here
              continue;
            }
#ifdef PA_MAP_STATS
            stat_bar = shared_bar(c_best, best_shared, floor_bar);  // this round goes on past the tight bound: how many of its windows reach the bar it was asked with?
            PA_STAT(39, __popcll(__ballot(lane_on && pending)));  // begins that pass the tight bound
            PA_STAT(40, 1);                                       // rounds that go on past it
#endif
          }
        }
#ifdef PA_MAP_STATS
        const int32_t stat_bar_round = stat_bar;
        stat_bar = -1000;
#endif
        uint32_t f_shared = 0, p_state = 0;  // p_state: the position of the lane's state = the window id of its begin
        uint32_t t_state = kNoT;             // its T, where the fine search found it
        bool counted = false;  // the lane holds the exact value of a state (a window found out of reach of the bar is done, but not counted)
        uint32_t taken = 0;
        bool complete = false;  // the begin's last state is behind it
        // fold the evaluated states into the candidate's optimum (fold_ties; the lanes hold the states in slide order).
        // The states that are not evaluated -- reached by taking in a minimizer the fragment does not hold -- share as many
        // as the state before them or fewer and have that state's begin, hence its position: they change neither.
#ifdef PA_MAP_STATS
        int32_t &stat_best = stat_best_of_candidate;
#endif
        auto fold_items = [&]() {
          const uint64_t dm = __ballot(counted);
          const int32_t group_best = (int32_t)pa_dev::wave_max_dpp(counted ? f_shared + 1u : 0u) - 1;
          if (dm && group_best >= c_best) {
            const uint64_t top_items = __ballot(counted && (int32_t)f_shared == group_best);
            fold_ties(group_best, top_items, p_state, c_best, c_first, c_last);
            const uint32_t tt = (uint32_t)__builtin_amdgcn_readlane((int)t_state, __builtin_ctzll(top_items));
            if (tt != kNoT) pivot_T = tt;
#ifdef PA_MAP_STATS
            stat_ties = (group_best > stat_best ? 0u : stat_ties) + (uint32_t)__popcll(top_items);
            stat_best = group_best;
#endif
          }
        };
        if (__builtin_amdgcn_readlane((int)cnt, (int)first_lane) == 0) {
          PA_STAT(9, 1);  // cooperative evaluations
          // the first pending begin's next window is longer than the stretch: the whole wave takes that one state from HBM
          const uint32_t wp0 = __shfl(wp, (int)first_lane, 64), we0 = __shfl(w_end, (int)first_lane, 64);
          const uint32_t en0 = __shfl(e_next, (int)first_lane, 64);
          const uint32_t e_abs = en0 ? en0 : wpos_lower_bound(mini_wpos, bucket_first, bb, nb, wp0 + count_windows);
          const uint32_t e_last = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, we0);
          if (e_abs <= e_last) {
            __syncthreads();
            for (uint32_t i = lane; i <= s; i += 64) sh.cnt[i] = 0;  // the cooperative form counts in the memory of the tables
            if (lane < (uint32_t)kQMax / 32) sh.matched[lane] = 0;    // (the rounds keep their bitmap of matching entries there)
            __syncthreads();
            const uint32_t v = eval_window_coop(base, e_abs);
            if (lane == first_lane) {
              f_shared = v;
              counted = true;
              p_state = wp0;
              e_next = e_abs + 1u;
            }
          }
          complete = lane == first_lane && e_abs + 1u > e_last;
          fold_items();
        } else {
          // ---- ranks of the lane's kPer minimizers among the fragment's hashes, for the part of the stretch that some
          // window of the pending begins reaches: the binary searches advance together, one halving step for all of them at
          // a time, so the LDS reads of a step are in flight at once
          const uint32_t n_rank = pa_dev::wave_max_dpp(lane_on ? top : 0u);
          uint32_t rank[kPer];
#pragma unroll
          for (int q = 0; q < kPer; ++q) rank[q] = 0;
          if (qsteps != 0xffffffffu) {
            uint32_t hi_r[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
              const uint32_t e = sh.qt[hh[q] >> kQtShift];
              rank[q] = e & 0x3ffu;          // hashes in the buckets below: all smaller
              hi_r[q] = rank[q] + (e >> 10);  // the hashes from here on are in higher buckets: all larger
            }
            for (uint32_t half = qsteps ? 1u << (qsteps - 1u) : 0u; half > 0; half >>= 1) {
#pragma unroll
              for (int q = 0; q < kPer; ++q) {
                const uint32_t idx = rank[q] + half;  // number of hashes below h is >= idx iff qh[idx - 1] < h
                if (idx <= hi_r[q] && sh.qh[idx - 1] < hh[q]) rank[q] = idx;
              }
            }
          } else {
            for (uint32_t half = half0; half > 0; half >>= 1) {  // half0 = largest power of two <= s: positions 0 .. 2*half0 - 1 >= s
#pragma unroll
              for (int q = 0; q < kPer; ++q) {
                const uint32_t idx = rank[q] + half;  // number of hashes below h is >= idx iff qh[idx - 1] < h
                if ((uint32_t)q * 64u + lane < n_rank && idx <= s && sh.qh[idx - 1] < hh[q]) rank[q] = idx;
              }
            }
          }
          // which entries match a hash of the fragment, as a bitmap over the stretch (scratch in the memory of the tables,
          // which are built later in the round)
          uint32_t match_q = 0;
          uint32_t *bm = sh.matched;  // (the cooperative evaluation, the other user of these words, clears them before it counts)
#pragma unroll
          for (int q = 0; q < kPer; ++q) {
            const uint32_t x = (uint32_t)q * 64u + lane;
            const bool is_match = (x < n_rank) & (rank[q] < s) & (sh.qh[min(rank[q], s - 1u)] == hh[q]);
            match_q |= (is_match ? 1u : 0u) << q;
            const uint64_t mb = __ballot(is_match);
            if (lane == 0) { bm[2 * q] = (uint32_t)mb; bm[2 * q + 1] = (uint32_t)(mb >> 32); }
          }
          __builtin_amdgcn_wave_barrier();
          // ---- which states are evaluated.  A state reached by taking in a minimizer that matches no hash of the fragment
          // (or repeats a hash the window holds) shares no more than the state before it, so the first state with the most
          // shared minimizers is never such a state, and the last one is the last evaluated state that has them or one of
          // the states right after it -- those are looked at once, when the candidate's other states are through (below).
          // Evaluated here: a begin's first state and every state reached by taking in a MATCHING minimizer.  Per round a
          // begin contributes the run of states from its first to its last such state among the next 16 (the few between
          // them ride along).
          // bit j: state xs0 + j is such a state
          uint32_t xa = xs0, len = 0;
          if (cnt) {
            const uint32_t p0 = xs0 - 1u, w0 = p0 >> 5;  // (xs0 >= 1: a window holds its begin)
            const uint64_t two = ((uint64_t)(w0 + 1u < (uint32_t)kQMax / 32u ? bm[w0 + 1u] : 0u) << 32) | bm[w0];
            uint32_t m = (uint32_t)(two >> (p0 & 31u));
            if (xs0 == xe_lo) m |= 1u;
            m &= (2u << min(top - xs0, 15u)) - 1u;
            if (m == 0u) {
              xa = xs0 + min(top - xs0, 15u) + 1u;  // nothing to evaluate among them
            } else {
              const uint32_t first = (uint32_t)__builtin_ctz(m), last = 31u - (uint32_t)__builtin_clz(m);
              xa = xs0 + first;
              len = last - first + 1u;
            }
          }
          // ---- the chosen states of the pending begins, in slide order, spread over the lanes: item t is state t - off of
          // the begin whose run of items [off, incl) holds t (runs laid out by a prefix sum of the counts).  A round takes up
          // to kRoundItems of them: 64, one pass of the lanes over the tables (128, two passes, is the form of the rounds before:
          // -DPA_MAP_ROUND_ITEMS=128); the begins whose states do not fit come back in a later round, if the bound lets them.
          const uint32_t incl = pa_dev::wave_incl_scan_dpp(len), off = incl - len;
          const uint32_t n_items = min(kRoundItems, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
          taken = off < kRoundItems ? min(len, kRoundItems - off) : 0u;
          // the begins: where their next state ends (past the states after the run that are not evaluated), and whether
          // the last state is behind them -- settled here, so that none of this is alive across the evaluation
          {
            uint32_t x_next = xs0;
            if (cnt) {
              x_next = taken == len ? xs0 + min(top - xs0, 15u) + 1u : xa + taken;
              e_next = base + x_next;
            }
            complete = lane_on && hi_known && x_next > xe_hi;
          }
          PA_CUT(kCutStretch);  // stretch loads and window ends
          PA_STAT(6, n_rank);                           // stretch entries ranked
          PA_STAT(7, n_items);                          // windows evaluated in the round
          PA_STAT(12, n_items == 0u ? 1u : 0u);
          PA_STAT(13, n_items > 64u ? 1u : 0u);
          if (n_items) {
            PA_CUT(kCutRanks);  // ranks
            // Every window of the round, one lane each, without ordering the stretch.  A window holds the stretch
            // positions [xs, xw) minus later occurrences of a hash it already holds: a bit mask W over the positions.  With
            // R_r / M_r = the positions of reference-only / matching minimizers of rank <= r among the fragment's hashes, the
            // reference-only minimizers below the fragment's hash of rank r number c(r) = |R_r & W|; that hash lies in the
            // bottom-s of the union iff r + c(r) < s, which holds for r < T and no other (r + c(r) grows strictly), and the
            // window shares |M_(T-1) & W| minimizers.  T comes from two searches per lane: over the rows at every kCoarse-th
            // rank, then over all ranks of the coarse group that holds it.  A row is R_r followed by M_r.
            uint32_t xs = 0, xw = 0;
            bool it_on = false;
            // the begin of item t: the first lane whose run ends past t (the run ends do not decrease over the lanes)
            auto item_setup = [&](uint32_t pass) {
              const uint32_t t = pass * 64u + lane;
              it_on = t < n_items;
              uint32_t src = 0;
              if (kRoundItems == 64u || pass == 0u) {  // the run starts marked in LDS (scratch in the memory of the tables), then a running maximum over the lanes
                sh.tab[lane] = 0u;
                __builtin_amdgcn_wave_barrier();
                if (len && off < 64u) sh.tab[off] = lane + 1u;
                __builtin_amdgcn_wave_barrier();
                src = max(pa_dev::wave_incl_max_scan_dpp(sh.tab[lane]), 1u) - 1u;
              } else {  // a search: the first lane whose run ends past t
#pragma unroll
                for (uint32_t step = 32; step > 0; step >>= 1) {
                  const uint32_t probe = src + step - 1u;
                  const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(min(probe, 63u) << 2), (int)incl);
                  src += (probe < 64u && v <= t) ? step : 0u;
                }
              }
              const int src_addr = (int)(min(src, 63u) << 2);
              const uint32_t packed = (uint32_t)__builtin_amdgcn_ds_bpermute(src_addr, (int)(((b - base) & 0x3ffu) | (xa << 10)));
              const uint32_t off_s = (uint32_t)__builtin_amdgcn_ds_bpermute(src_addr, (int)off);
              p_state = (uint32_t)__builtin_amdgcn_ds_bpermute(src_addr, (int)wp);  // the state's position: its begin's window id
              xs = it_on ? (packed & 0x3ffu) : 0u;                  // the window: stretch entries [xs, xw)
              xw = it_on ? (packed >> 10) + (t - off_s) : 0u;
            };
            item_setup(0u);
          constexpr uint32_t kW = kRefCap / 32u;  // words per half row; stretch position q * 64 + lane is bit (lane & 31) of word 2 q + (lane >> 5)
          constexpr uint32_t kRow = 2u * kW;
          const uint32_t n_coarse = s / kCoarse + 1u;  // the last row stands at a rank >= s: r + c(r) >= s holds there
          uint32_t *bc = sh.tab, *bf = sh.tab + n_coarse * kRow;
          __syncthreads();
          {
            uint4 *t4 = reinterpret_cast<uint4 *>(sh.tab);
            for (uint32_t i = lane; i < n_coarse * kRow / 4u; i += 64) t4[i] = make_uint4(0u, 0u, 0u, 0u);  // kRow is a multiple of 4
          }
          const uint16_t *prev16 = sh.prev;
          // word of an entry's bit inside a row (the matching half comes second)
          auto col_of = [&](int q) -> uint32_t { return 2u * (uint32_t)q + (lane >> 5) + (((match_q >> q) & 1u) ? kW : 0u); };
#pragma unroll
          for (int q = 0; q < kPer; ++q) {
            const uint32_t x = (uint32_t)q * 64u + lane;
            const uint32_t r = rank[q];
            const bool valid = (x < n_rank) & (r < s);  // inside the used part and below some hash of the fragment: in the rows from r on
            rank[q] = valid ? r : 0xffffffffu;
          }
          const bool any_dup = __any(dup_q != 0u);
          __syncthreads();
#pragma unroll
          for (int q = 0; q < kPer; ++q) {  // no branch: entries that are in no row add nothing to a word of the (not yet filled) fine rows
            const bool valid = rank[q] != 0xffffffffu;
            atomicOr(valid ? &bc[(rank[q] >> kCoarseShift) * kRow + col_of(q)] : &bf[lane], valid ? 1u << (lane & 31u) : 0u);
          }
          __syncthreads();
          // rows become prefixes: row g |= rows below it.  Lane = (pair of columns, run of rows); the runs of one column
          // pair are chained through the totals of the runs before
          auto prefix_or_rows = [&](uint32_t *rows, uint32_t n_rows) {
            constexpr uint32_t kRuns = 64u / kW;
            uint2 *rows2 = reinterpret_cast<uint2 *>(rows);  // kW column pairs per row
            const uint32_t cp = lane % kW, run = lane / kW;
            const uint32_t per = (n_rows + kRuns - 1u) / kRuns;
            const uint32_t r0 = min(n_rows, run * per), r1 = run < kRuns ? min(n_rows, r0 + per) : r0;
            uint2 acc = make_uint2(0u, 0u);
            for (uint32_t r = r0; r < r1; ++r) { const uint2 v = rows2[r * kW + cp]; acc.x |= v.x; acc.y |= v.y; }
            uint2 before = make_uint2(0u, 0u);
#pragma unroll
            for (uint32_t j = 1; j < kRuns; ++j) {
              const int from = (int)(lane >= kW * j ? lane - kW * j : lane);
              const uint32_t vx = (uint32_t)__shfl((int)acc.x, from, 64), vy = (uint32_t)__shfl((int)acc.y, from, 64);
              if (run >= j) { before.x |= vx; before.y |= vy; }
            }
            for (uint32_t r = r0; r < r1; ++r) {
              const uint2 v = rows2[r * kW + cp];
              before.x |= v.x; before.y |= v.y;
              rows2[r * kW + cp] = before;
            }
          };
          prefix_or_rows(bc, n_coarse);
          PA_CUT(kCutCoarseTable);  // coarse table
            for (uint32_t pass = 0; pass * 64u < n_items && !(pass && PA_CUT_IS(kCutNoSecondPass)); ++pass) {
              if (pass) item_setup(pass);
              // the lane's window as a mask over the stretch positions
              uint32_t wm[kW];
              {
                // bits [xs, xw) of the row, two words at a time: xs is below 64, so only the first pair has a lower end
                auto below = [](int32_t b) -> uint64_t {  // the b lowest bits of a pair of words, b clamped to 0 .. 64
                  const uint64_t m = b >= 64 ? ~0ULL : (1ULL << (b & 63)) - 1ULL;
                  return b <= 0 ? 0ULL : m;
                };
    #pragma unroll
                for (uint32_t w2 = 0; w2 < kW / 2u; ++w2) {
                  uint64_t m = below((int32_t)xw - (int32_t)(64u * w2));
                  if (w2 == 0) m &= ~below((int32_t)xs);
                  wm[2 * w2] = (uint32_t)m;
                  wm[2 * w2 + 1] = (uint32_t)(m >> 32);
                }
              }
              if (any_dup) {
    #pragma unroll
                for (int q = 0; q < kPer; ++q) {
                  for (uint64_t dmask = __ballot((dup_q >> q) & 1u); dmask; dmask &= dmask - 1) {
                    const uint32_t bit = (uint32_t)__builtin_ctzll(dmask);
                    if ((uint32_t)prev16[(uint32_t)q * 64u + bit] > xs) {  // the earlier occurrence lies inside this lane's window
                      if (bit < 32u) wm[2 * q] &= ~(1u << bit); else wm[2 * q + 1] &= ~(1u << (bit - 32u));
                    }
                  }
                }
              }
              auto count_in = [&](const uint32_t *half_row) -> uint32_t {
                const uint2 *row2 = reinterpret_cast<const uint2 *>(half_row);  // half rows start on 8-byte boundaries (kW is even)
                uint32_t c = 0;
    #pragma unroll
                for (uint32_t w = 0; w < kW / 2u; ++w) {
                  const uint2 v = row2[w];
                  c += __popc(v.x & wm[2 * w]) + __popc(v.y & wm[2 * w + 1]);
                }
                return c;
              };
              __syncthreads();
              // coarse: the first group g whose last rank r = kCoarse g + kCoarse - 1 has r + c(r) >= s (the last row always has)
              uint32_t g_lo = 0, g_hi = n_coarse - 1u;
              for (uint32_t span = n_coarse - 1u; span > 0u; span >>= 1) {  // as many halvings as the widest range needs
                const uint32_t mid = (g_lo + g_hi) >> 1;
                const bool ge = mid * kCoarse + (kCoarse - 1u) + count_in(bc + mid * kRow) >= s;
                const bool open = g_lo < g_hi;
                g_hi = (open & ge) ? mid : g_hi;
                g_lo = (open & !ge) ? mid + 1u : g_lo;
              }
              PA_CUT(kCutCoarseSearch);  // window masks, coarse search
              // fine: the groups of the lanes lie next to each other as a rule; kFineGroups of them per pass
              // A window shares |M_(T-1) & W| minimizers and T - 1 lies in the coarse group just found, so the matches up to the
              // group's last rank bound it from above (by the matches of at most 15 more ranks): windows that cannot reach
              // the bar any more -- most of a candidate's windows away from its optimum -- are done here, without the fine
              // tables, and are left out of the fold below (their exact value is below the bar, which is all that matters).
              const int32_t bar_now = shared_bar(c_best, best_shared, floor_bar);
              const bool in_reach = (int32_t)count_in(bc + g_lo * kRow + kW) >= bar_now;
              counted = it_on && in_reach;
              bool unresolved = counted && !PA_CUT_IS(kCutNoFinePass);
              while (__any(unresolved)) {
                PA_STAT(8, 1);  // fine passes
                const uint32_t g_cur = pa_dev::wave_min_dpp(unresolved ? g_lo : 0xffffffffu);
                const uint32_t band0 = g_cur * kCoarse;  // row t of the band: ranks <= band0 + t - 1; row 0 is the coarse row below
                __syncthreads();
                {
                  uint4 *f4 = reinterpret_cast<uint4 *>(bf);  // bf starts on a 16-byte boundary: kRow is a multiple of 4 words
                  const uint4 *below = reinterpret_cast<const uint4 *>(bc + (g_cur ? g_cur - 1u : 0u) * kRow);
                  for (uint32_t i = lane; i < kFineRows * kRow / 4u; i += 64)
                    f4[i] = (i < kRow / 4u && g_cur > 0u) ? below[i] : make_uint4(0u, 0u, 0u, 0u);
                }
                __syncthreads();
    #pragma unroll
                for (int q = 0; q < kPer; ++q) {
                  const uint32_t t = rank[q] - band0;  // wraps to something huge below the band
                  const bool valid = (rank[q] != 0xffffffffu) & (t < kFineRows - 1u);
                  atomicOr(valid ? &bf[(t + 1u) * kRow + col_of(q)] : &bc[lane], valid ? 1u << (lane & 31u) : 0u);
                }
                __syncthreads();
                prefix_or_rows(bf, kFineRows);
                __syncthreads();
                const bool now = unresolved && g_lo - g_cur < kFineGroups;
                // first rank r of the lane's group with r + c(r) >= s: the group's last rank has it
                uint32_t r_lo = g_lo * kCoarse, r_hi = r_lo + kCoarse - 1u;
                if (!now) r_lo = r_hi = band0;
                for (uint32_t step = 0; step < kCoarseShift; ++step) {
                  const uint32_t mid = (r_lo + r_hi) >> 1;
                  const bool ge = mid + count_in(bf + (mid - band0 + 1u) * kRow) >= s;
                  const bool open = r_lo < r_hi;
                  r_hi = (open & ge) ? mid : r_hi;
                  r_lo = (open & !ge) ? mid + 1u : r_lo;
                }
                const uint32_t c = count_in(bf + (r_lo - band0) * kRow + kW);  // matches of rank < T = r_lo
                if (now) { f_shared = c; t_state = r_lo; unresolved = false; }
              }
              __syncthreads();
              PA_STAT(14, __popcll(__ballot(counted)));  // windows whose exact value was found
#ifdef PA_MAP_STATS
              if (stat_bar_round != -1000) {
                PA_STAT(37, __popcll(__ballot(it_on)));                                              // windows of rounds that passed the tight bound
                PA_STAT(38, __popcll(__ballot(counted && (int32_t)f_shared >= stat_bar_round)));     // ... that reach the bar
              }
#endif
              PA_STAT(15, __popcll(__ballot(counted && (int32_t)f_shared >= shared_bar(c_best, best_shared, floor_bar))));  // ... at or above the bar
              fold_items();
            }
            PA_CUT(kCutFirstRound);  // first round only, complete: fine passes and fold included
            // The begins that keep states for a later round are asked the tight bound NOW -- with the bar and the pivot this
            // round has just set, against the stretch that is here: which entries lie below the pivot hash follows from
            // their ranks (rank < r0, or rank == r0 and no match), still in registers.  A begin dropped here never causes
            // another round: what a round costs is the wait for its stretch, not the instructions.
            if (kBoundInRound && staged && unseeded == 0 && pivot_T != kNoT && __any(lane_on && !complete)) {
              const uint32_t r0 = min(pivot_T, s - 1u) & ~1u;
              lmask_for(r0);
              uint32_t *bw = sh.matched;
#pragma unroll
              for (int q = 0; q < kPer; ++q) {
                const bool below_pivot = (rank[q] < r0) | ((rank[q] == r0) & (((match_q >> q) & 1u) == 0u));  // (rank 0xffffffff: not in the ranked part, or above every hash of the fragment)
                const uint64_t mb = __ballot(below_pivot & (((dup_q >> q) & 1u) == 0u));
                if (lane == 0) { bw[2 * q] = (uint32_t)mb; bw[2 * q + 1] = (uint32_t)(mb >> 32); }
              }
              const bool fails = tight_fails(lane_on && !complete, r0);
              PA_STAT(41, __popcll(__ballot(fails)));  // begins dropped by the bound asked at the end of a round
              pending = pending && !fails;
            }
          }
        }
        PA_STAT(10, __popcll(__ballot(lane_on)));   // begins taking part in the rounds
        PA_STAT(11, __popcll(__ballot(complete)));  // begins finished by the rounds
        pending = pending && !complete;
        // whoever can no longer reach the bar drops out
        {
          const int32_t bar2 = shared_bar(c_best, best_shared, floor_bar) - unseeded;
          pending = pending && (bar2 > 0 ? holds_hits(bar2) : true);
        }
      }
    }
#ifdef PA_MAP_STATS
    PA_STAT(33, stat_ties ? stat_ties : 1u);  // states tying the candidate's optimum (one probe where nothing was evaluated)
#endif
    if (c_best < 0) return;
    __syncthreads();
    if (candidate_is_the_mapping(c_best, best_shared) && lane == 0) {  // (of equals, the last)
      sh.scan[kBestShared] = (uint32_t)c_best; sh.scan[kBestC] = c; sh.scan[kBestFirst] = c_first; sh.scan[kBestLast] = c_last;
      sh.scan[kBestT] = pivot_T;
    }
    __syncthreads();
  };

  // ---- L1 (the rule: l1_run_valid, l1_range_start, l1_opens_candidate), sixty-four runs at a time.
  // The candidates a chunk of 64 runs closes are first listed (LDS, kListCap at a time), then evaluated: the evaluation
  // is in the code once and none of the scan's per-lane state is alive across it.  A chunk that closes more than
  // kListCap candidates is scanned again for the rest (`handled` = its breaks already listed).
#ifndef PA_MAP_LIST_CAP
#define PA_MAP_LIST_CAP 8  // 1 in a test build: every chunk with two closed candidates is then scanned twice
#endif
  constexpr uint32_t kListCap = PA_MAP_LIST_CAP;
  bool have_cur = false, have_prev = false;
  uint32_t cur_c = 0, cur_cs = 0, cur_ce = 0, cur_fw = 0, prev_c = 0, prev_ce = 0;
  uint64_t handled = 0;
  uint32_t chunk = 0;
  // What most segments are: all hits on one contig within one fragment length.  Then every run of mh hits is valid and
  // every run's range touches the one before (it starts at or before the segment's first hit): ONE candidate, known from
  // three hits -- its range starts fragLen - 1 before the mh-th hit and ends at the first hit of the last run -- and the
  // scan goes straight to its last turn, which lists it.
  // And what most of the others are: that one run plus ONE OR TWO STRAY hits -- chance matches on another contig or far away on
  // the same one (a third of the segments at 1 000 genomes hold one, an eighth two; with them 96 % of the segments are
  // covered).  In (contig, window id) order the strays stand at the ends: `lo` of them before the run, `hi` after it.  If no
  // run of mh hits that includes a stray is valid -- tested directly, a handful of comparisons -- the strays give no candidate
  // and take no part in the run's, whose range cannot reach them: the scan would list exactly the one candidate the run
  // alone gives.  The eight smallest and the eight largest hits are all that is asked (one read per lane, sixteen lanes).
  if (kL1OneRun && staged) {
    constexpr uint32_t kEnd = 8;  // hits known from each end
    const uint32_t at = lane < kEnd ? lane : nh - 2u * kEnd + lane;  // lanes 0-7: hits 0-7, lanes 8-15: hits nh-8 .. nh-1
    const bool enough = nh >= 2u * kEnd && mh <= kEnd - 2u;
    const uint32_t idx = enough ? min(at, nh - 1u) : (lane == 0u ? 0u : nh - 1u);  // (short segments: the first and the last hit, the old test)
    const uint32_t e_w = sh.hw[idx] >> 8, e_c = sh.hc[idx];
    auto W = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)e_w, (int)(i < kEnd ? i : i + 2u * kEnd - nh)); };  // i < 8 or i >= nh - 8
    auto C = [&](uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)e_c, (int)(i < kEnd ? i : i + 2u * kEnd - nh)); };
    // (l1_run_valid written out, the window ids read only where the contigs agree: as a call it changed the kernel's scalar spills)
    auto run_valid = [&](uint32_t i) { return C(i) == C(i + mh - 1u) && W(i + mh - 1u) - W(i) < frag_len; };  // (i and i + mh - 1 at the same end)
    uint32_t lo = 0xffffffffu, hi = 0;
    if (!enough) {
      const uint32_t w_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)e_w), w_last = (uint32_t)__builtin_amdgcn_readlane((int)e_w, 1);
      if (l1_run_valid((uint32_t)__builtin_amdgcn_readfirstlane((int)e_c), w_first, (uint32_t)__builtin_amdgcn_readlane((int)e_c, 1), w_last, frag_len)) {
        lo = 0;
        const uint32_t yw = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sh.hw[mh - 1u] >> 8));
        cur_c = hc_base + (uint32_t)__builtin_amdgcn_readfirstlane((int)e_c);
        cur_cs = l1_range_start(yw, frag_len);
        cur_ce = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sh.hw[nh - mh] >> 8));
        cur_fw = w_first;
      }
    } else {
      // fewest strays first: (0, 0), then one, then two
      constexpr uint32_t kTry[6][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {2, 0}, {0, 2}};
      for (uint32_t t = 0; t < (kL1Strays ? 6u : 1u) && lo == 0xffffffffu; ++t) {
        const uint32_t a = kTry[t][0], b = kTry[t][1];
        if (!(C(a) == C(nh - 1u - b) && W(nh - 1u - b) - W(a) < frag_len)) continue;  // the hits between are not one run
        bool stray_run = false;
        for (uint32_t i = 0; i < a; ++i) stray_run = stray_run || run_valid(i);                        // runs that begin with a stray
        for (uint32_t i = nh - b - mh + 1u; i + mh <= nh; ++i) stray_run = stray_run || run_valid(i);  // runs that end with one
        if (stray_run) break;  // strays that make a run of their own, or join the run's: the scan's business
        lo = a;
        hi = b;
      }
      if (lo != 0xffffffffu) {
        const uint32_t yw = W(lo + mh - 1u);
        cur_c = hc_base + C(lo);
        cur_cs = l1_range_start(yw, frag_len);
        cur_ce = W(nh - hi - mh);
        cur_fw = W(lo);
      }
    }
    if (lo != 0xffffffffu) {
      have_cur = true;
      chunk = nh;
      PA_STAT(42, 1);            // segments that are one run (strays or none)
      PA_STAT(46, nh);           // ... and their seed hits
      PA_STAT(47, lo + hi ? 1u : 0u);  // ... of them with strays
    }
  }
  for (;;) {
    const bool tail = chunk >= nh;  // one more turn after the last chunk lists the candidate still open
    uint32_t n_list = 0;
    auto list_current = [&]() {
      if (lane == 0) {
        uint4 *slot = reinterpret_cast<uint4 *>(sh.cand) + n_list;
        *slot = make_uint4(cur_c, cur_cs, cur_ce, cur_fw);
      }
      ++n_list;
    };
    if (tail) {
      if (have_cur) list_current();
    } else {
      const uint32_t i = chunk + lane;
      bool v = false;
      uint32_t c_i = 0, cs_i = 0, ce_i = 0;
      if (i + mh <= nh) {
        c_i = HC(i);
        ce_i = HW(i);
        const uint32_t yw = HW(i + mh - 1);
        v = l1_run_valid(c_i, ce_i, HC(i + mh - 1), yw, frag_len);
        cs_i = l1_range_start(yw, frag_len);
      }
      const uint64_t vm = __ballot(v);
      if (!vm) { chunk += 64; continue; }
      // the valid run before this lane's: in this chunk, or carried over from the chunks before
      const uint64_t below = vm & ((1ULL << lane) - 1ULL);
      const int pl = below ? 63 - __builtin_clzll(below) : 0;
      const uint32_t sc = __shfl(c_i, pl, 64), se = __shfl(ce_i, pl, 64);
      const bool hp = below ? true : have_prev;
      const uint32_t pc = below ? sc : prev_c, pe = below ? se : prev_ce;
      const bool brk = v && l1_opens_candidate(hp, pc, pe, c_i, cs_i);
      const uint64_t bm_all = __ballot(brk);
      uint64_t bm = bm_all & ~handled;
      if (!handled) {
        // valid runs before the first break of the chunk extend the carried candidate
        const uint64_t head = bm_all ? vm & ((1ULL << __builtin_ctzll(bm_all)) - 1ULL) : vm;
        if (head && have_cur) cur_ce = max(cur_ce, (uint32_t)__builtin_amdgcn_readlane((int)ce_i, 63 - __builtin_clzll(head)));
      }
      while (bm && n_list < kListCap) {
        const int bit = __builtin_ctzll(bm);
        bm &= bm - 1;
        handled |= 1ULL << bit;
        if (have_cur) list_current();
        const uint64_t upto = bm ? ((1ULL << __builtin_ctzll(bm)) - 1ULL) : ~0ULL;
        const uint64_t mine = vm & upto & ~((1ULL << bit) - 1ULL);  // the valid runs of this group inside the chunk
        // (uniform lane numbers: v_readlane puts the values into scalar registers, where the scan's state belongs)
        cur_c = (uint32_t)__builtin_amdgcn_readlane((int)c_i, bit);
        cur_cs = (uint32_t)__builtin_amdgcn_readlane((int)cs_i, bit);
        cur_fw = (uint32_t)__builtin_amdgcn_readlane((int)ce_i, bit);  // window id of the first hit of the candidate's first run
        cur_ce = (uint32_t)__builtin_amdgcn_readlane((int)ce_i, 63 - __builtin_clzll(mine));
        have_cur = true;
      }
      if (!bm) {  // the chunk is done
        const int last = 63 - __builtin_clzll(vm);
        prev_c = (uint32_t)__builtin_amdgcn_readlane((int)c_i, last);
        prev_ce = (uint32_t)__builtin_amdgcn_readlane((int)ce_i, last);
        have_prev = true;
        handled = 0;
        chunk += 64;
      }
    }
    // A turn that lists nothing (most do: a segment of 139 hits is three chunks and ends with ONE candidate) goes straight on.
    if (n_list == 0u) {
      if (tail) break;
      continue;
    }
    // The scan's state sits in LDS while the listed candidates are evaluated: kept in registers across the evaluation --
    // the register-hungriest part of the kernel -- it was spilled to scratch memory (HBM traffic, and a wait) at every turn.
    // (The last turn -- for nineteen segments in twenty the only one -- needs none of it back; handing its one candidate to the
    // evaluation straight from the scan's registers, without the list and the parking in LDS, was tried in round 6: the kernel
    // goes from 126 registers to 128 with four spilled, mapping 364 ms against 359.)
    if (lane == 0) {
      sh.scan[0] = chunk; sh.scan[1] = (have_cur ? 1u : 0u) | (have_prev ? 2u : 0u) | (tail ? 4u : 0u);
      sh.scan[2] = cur_c; sh.scan[3] = cur_cs; sh.scan[4] = cur_ce; sh.scan[5] = cur_fw; sh.scan[6] = prev_c; sh.scan[7] = prev_ce;
      sh.scan[8] = (uint32_t)handled; sh.scan[9] = (uint32_t)(handled >> 32); sh.scan[10] = n_list;
    }
    __syncthreads();
    for (uint32_t t = 0; t < sh.scan[10]; ++t) {
      const uint4 cand = reinterpret_cast<const uint4 *>(sh.cand)[t];
      process_candidate((uint32_t)__builtin_amdgcn_readfirstlane((int)cand.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)cand.y),
                        (uint32_t)__builtin_amdgcn_readfirstlane((int)cand.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)cand.w));
    }
    __syncthreads();
    {
      const uint32_t flags1 = sh.scan[1];
      chunk = sh.scan[0]; have_cur = flags1 & 1u; have_prev = (flags1 >> 1) & 1u;
      cur_c = sh.scan[2]; cur_cs = sh.scan[3]; cur_ce = sh.scan[4]; cur_fw = sh.scan[5]; prev_c = sh.scan[6]; prev_ce = sh.scan[7];
      handled = ((uint64_t)sh.scan[9] << 32) | sh.scan[8];
      if (flags1 & 4u) break;
    }
    __syncthreads();
  }

  __syncthreads();
  const int32_t best_shared = (int32_t)sh.scan[kBestShared];
  if (lane == 0 && best_shared >= 0 && (uint32_t)best_shared >= rec1.w) {  // (rec1.w: tab_min_shared[s]; rec2.w: frag_genome_local[f])
    const unsigned long long packed = mapping_packed(best_shared, s);
    const uint64_t bin = mapping_bin(contig_bin_off[sh.scan[kBestC]], sh.scan[kBestFirst], sh.scan[kBestLast], frag_len);
    atomicMax(&table[(uint64_t)rec2.w * table_stride + bin], packed);
  }
}
