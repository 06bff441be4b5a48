// fragani_sparse.inc -- part of fragani.hip (included there, inside its anonymous namespace: one translation unit): the mapping kernel for segments of at most eight seed hits: the hit-by-hit form of the windowed MinHash.

// ============================================================== 4b. segments of a handful of seed hits
// A pair of the same species that has diverged far leaves a fragment two to eight seed hits in a reference genome.  Such a
// segment is the mapping kernel's worst customer: every window that holds its few hits shares the same few minimizers or
// nearly, so the states that tie the optimum span hundreds of begins -- four or five rounds of ranking a stretch and
// building bit tables where a window holds eight matches at most (13 % of the segments, a quarter of the rounds at 1 000
// genomes).  With so few matches the windowed MinHash has a direct form: hit j, of rank r_j among the fragment's hashes,
// is shared by a window iff it lies in it and r_j + c_j < s, c_j = the window's reference-only minimizers below the hit's
// hash -- a count over a range of the stretch, two prefix sums per hit and state.  One wave per segment: no sketch, no
// rank, no table; per group of 64 begins the stretch's hashes are compared with the (at most eight) hit hashes, one bit
// mask and its prefix counts per hit go to LDS, and every begin that can still matter evaluates all its states (which begins
// those are, and in which order the groups are taken: at the group loop below).  Same candidates, same slide, same
// positions and ties as map_segments_kernel (the rules both call: fragani_rules.inc); whatever does not fit the
// simple form -- a hash met twice in a stretch, windows longer than the stretch -- sends the segment to
// map_segments_kernel through the overflow list.
constexpr uint32_t kSparseHits = kTinySegment;  // (16: 426 ms of mapping per 1 000-genome run against 419)
#ifndef PA_SPARSE_ENDS
#define PA_SPARSE_ENDS 1  // 0: every group of a candidate's begins is evaluated, left to right (the form before)
#endif
constexpr bool kSparseEnds = PA_SPARSE_ENDS != 0;
constexpr uint32_t kSparseCap = 384;  // stretch entries of a group of 64 begins (a window holds ~237: 5 sigma to spare)
__global__ __launch_bounds__(64) void map_sparse_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_a0, const uint32_t *__restrict__ seg_nh,
    const uint32_t *__restrict__ seg_f, uint32_t n_segs, const uint32_t *__restrict__ q_s, const uint32_t *__restrict__ q_hash,
    const uint32_t *__restrict__ frag_genome_local, uint32_t frag_len, uint32_t count_windows,
    const uint32_t *__restrict__ tab_min_hits, const uint32_t *__restrict__ tab_min_shared,
    const uint32_t *__restrict__ contig_mini_off, const uint32_t *__restrict__ contig_bucket_off,
    const uint32_t *__restrict__ bucket_first, const uint32_t *__restrict__ mini_hash, const uint32_t *__restrict__ mini_wpos,
    const int32_t *__restrict__ prev_same, const uint32_t *__restrict__ contig_bin_off, uint64_t table_stride,
    unsigned long long *__restrict__ table, uint32_t *__restrict__ over_a0, uint32_t *__restrict__ over_nh,
    uint32_t *__restrict__ over_f, uint32_t *__restrict__ over_n
#ifdef PA_MAP_STATS
    , uint32_t *__restrict__ run_g  // event counters of the stats build, slots 48 .. 59 (the general kernel's are below)
#endif
) {
#ifdef PA_MAP_STATS
#define PA_SSTAT(slot, v) do { const uint32_t pa_stat_v = (uint32_t)(v); if (threadIdx.x == 0) atomicAdd(&run_g[slot], pa_stat_v); } while (0)
#else
#define PA_SSTAT(slot, v) do { } while (0)
#endif
  constexpr int kPer = (int)(kSparseCap / 64u);
  constexpr uint32_t kWords = kSparseCap / 32u;  // 12
  __shared__ uint32_t s_hc[kSparseHits], s_hw[kSparseHits], s_hr[kSparseHits], s_ph[kSparseHits], s_pos[kSparseHits];
  __shared__ uint32_t s_cand[kSparseHits][4];
  __shared__ uint16_t s_refw[kSparseCap];
  __shared__ __attribute__((aligned(8))) uint32_t s_B[kSparseHits][kWords + 2];  // (a row is a whole number of 8-byte pairs: the ballots are stored as pairs)
  __shared__ uint32_t s_P[kSparseHits][kWords + 1];
  __shared__ uint32_t s_hitbits[kWords];  // a bit per stretch entry: the entry is one of the segment's hits
  const uint32_t lane = threadIdx.x;
  if (blockIdx.x >= n_segs) return;
  const uint32_t a0 = seg_a0[blockIdx.x], nh = seg_nh[blockIdx.x], f = seg_f[blockIdx.x];
  const uint32_t s = q_s[f];
  if (s == 0 || nh > kSparseHits) return;
  const uint32_t mh = tab_min_hits[s];
  if (nh < mh) return;
  const int32_t floor_bar = (int32_t)tab_min_shared[s];
  {  // the hits in (contig, window id) order, with the rank and the hash of each
    uint64_t k1[1];
    const uint64_t raw = lane < nh ? keys[a0 + lane] : 0ULL;
    k1[0] = lane < nh ? hit_sort_key(raw) : ~0ULL;
    bitonic_sort_lanes<1, uint64_t>(k1, lane);
    if (lane < nh) {
      const uint32_t r = sort_key_rank(k1[0]);
      s_hw[lane] = sort_key_window(k1[0]);
      s_hc[lane] = sort_key_contig(k1[0]);
      s_hr[lane] = r;
      s_ph[lane] = q_hash[(uint64_t)f * kQMax + r];
    }
  }
  __syncthreads();
  // ---- L1, one run after the other: at most eight hits
  uint32_t n_cand = 0;
  {
    bool have = false, have_prev = false;
    uint32_t cur_c = 0, cur_cs = 0, cur_ce = 0, cur_fw = 0, prev_c = 0, prev_ce = 0;
    for (uint32_t i = 0; i + mh <= nh; ++i) {
      const uint32_t c_i = s_hc[i], ce_i = s_hw[i], yw = s_hw[i + mh - 1u];
      if (!l1_run_valid(c_i, ce_i, s_hc[i + mh - 1u], yw, frag_len)) continue;
      const uint32_t cs_i = l1_range_start(yw, frag_len);
      if (l1_opens_candidate(have_prev, prev_c, prev_ce, c_i, cs_i)) {
        if (have) { if (lane == 0) { s_cand[n_cand][0] = cur_c; s_cand[n_cand][1] = cur_cs; s_cand[n_cand][2] = cur_ce; s_cand[n_cand][3] = cur_fw; } ++n_cand; }
        cur_c = c_i; cur_cs = cs_i; cur_ce = ce_i; cur_fw = ce_i; have = true;
      } else {
        cur_ce = max(cur_ce, ce_i);
      }
      prev_c = c_i; prev_ce = ce_i; have_prev = true;
    }
    if (have) { if (lane == 0) { s_cand[n_cand][0] = cur_c; s_cand[n_cand][1] = cur_cs; s_cand[n_cand][2] = cur_ce; s_cand[n_cand][3] = cur_fw; } ++n_cand; }
  }
  __syncthreads();
  PA_SSTAT(48, n_cand ? 1u : 0u);  // segments with a candidate
  PA_SSTAT(49, n_cand);            // candidates
  bool overflow = false;
  int32_t best_shared = -1;
  uint32_t best_c = 0, best_first = 0, best_last = 0;
  for (uint32_t ci = 0; ci < n_cand && !overflow; ++ci) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cand[ci][0]);
    const uint32_t cs = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cand[ci][1]);
    const uint32_t ce = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cand[ci][2]);
    const uint32_t m1 = contig_mini_off[c + 1];
    const uint32_t bb = contig_bucket_off[c], nb = contig_bucket_off[c + 1] - bb - 1;
    uint32_t b_lo, origin;
    uint32_t wpv[kStartBatch];
    {
      uint32_t bk = cs >> kBucketShift;
      if (bk >= nb) bk = nb;
      const uint32_t lo = bucket_first[bb + bk];
      const uint32_t hi = bk < nb ? bucket_first[bb + bk + 1] : lo;
      slide_first_begin(mini_wpos, m1, lo, hi, cs, lane, b_lo, origin, wpv);
    }
    if (b_lo >= m1) continue;
    uint32_t b_hi, i_max;
    // where the slide ends: a copy of the block in process_candidate of map_segments_kernel (fragani_map.inc) -- a change
    // here is a change there; as a shared function it changed both kernels' scalar spills
    {
      const uint32_t limit = ce + frag_len;
      uint32_t z = 0;
      bool reached = false;
#pragma unroll
      for (int q = 0; q < kStartBatch; ++q) {
        z = wpv[q] < limit ? max(z, wpv[q]) : z;
        reached = reached || wpv[q] >= limit;
      }
      const uint32_t shift = b_lo - origin;  // <= 64
      const uint32_t wp_lo = shift < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)wpv[0], (int)shift) : (uint32_t)__builtin_amdgcn_readfirstlane((int)wpv[1]);
      if (wp_lo >= limit) continue;
      if (__any(reached)) {
        z = pa_dev::wave_max_dpp(z);
      } else {  // a range of more than 512 minimizers (two far-apart runs merged): through the bucket index, as the general kernel does
        const uint32_t last_end = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, limit);
        z = mini_wpos[last_end - 1];
      }
      if (z < wp_lo + count_windows) continue;
      i_max = z - count_windows;
      uint32_t my_over = 0xffffffffu;
#pragma unroll
      for (int q = kStartBatch - 1; q >= 0; --q) my_over = wpv[q] > i_max ? (uint32_t)q * 64u + lane : my_over;
      const uint32_t w_over = pa_dev::wave_min_dpp(my_over);
      b_hi = w_over != 0xffffffffu ? origin + w_over : wpos_lower_bound(mini_wpos, bucket_first, bb, nb, i_max + 1u);
    }
    if (b_lo >= b_hi) continue;
    int32_t c_best = -1;
    uint32_t c_first = 0, c_last = 0;
    const uint32_t n_groups = (b_hi - b_lo + 63u) / 64u;
    // Of the states that tie a candidate's optimum only the FIRST and the LAST one count (the mapping's position is the mean of
    // their positions), and in a sparse segment four states in five tie: every window that holds the same few hits shares
    // the same few minimizers.  So a begin that lies BETWEEN two begins already known to tie the best so far is evaluated only
    // if it can share MORE -- if its widest window holds more hits than that --, and the groups are taken in the order that
    // makes most begins such begins: first the group of the begin at the candidate's first hit (the last begin that can hold
    // every hit), then the groups from the left upwards, then those from the right downwards.  Where the best is all the hits
    // the candidate holds (n_all: the hits on its contig between the first begin and the end of the last window; no window
    // shares more), a group between the tying begins is passed over without a look at its begins.
    uint32_t n_all = 0, g_start = 0;
    {
      const uint32_t wp_first = (uint32_t)__builtin_amdgcn_readlane((int)wpv[0], 0);  // (<= the first begin's window id: the batch starts at or before it)
      uint32_t hw_first = 0xffffffffu;
      for (uint32_t i = 0; i < nh; ++i) {
        const bool in = s_hc[i] == c && s_hw[i] >= wp_first && s_hw[i] < i_max + count_windows;
        n_all += in ? 1u : 0u;
        hw_first = in ? min(hw_first, s_hw[i]) : hw_first;
      }
      if (kSparseEnds && hw_first != 0xffffffffu) {
        uint32_t upto = 0;  // minimizers of the batch at or before the first hit
#pragma unroll
        for (int q = 0; q < kStartBatch; ++q) upto += wpv[q] <= hw_first ? 1u : 0u;
        upto = wave_sum(upto);
        uint32_t b_at = upto ? origin + upto - 1u : b_lo;
        if (upto == (uint32_t)kStartBatch * 64u) { b_at = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, hw_first + 1u) - 1u; PA_SSTAT(55, 1); }  // (past the batch)
        b_at = min(max(b_at, b_lo), b_hi - 1u);
        g_start = (b_at - b_lo) / 64u;
      }
    }
    uint32_t tie_lo = 0xffffffffu, tie_hi = 0u;  // the first and the last begin known to tie c_best (minimizer indices)
    for (uint32_t turn = 0; turn < n_groups && !overflow; ++turn) {
      const uint32_t g = !kSparseEnds ? turn : turn == 0u ? g_start : (turn <= g_start ? turn - 1u : n_groups + g_start - turn);
      do {
      const uint32_t sb = b_lo + g * 64u, b = sb + lane;
      const bool has = b < b_hi;
      if (kSparseEnds && c_best >= 0 && (uint32_t)c_best >= n_all && sb > tie_lo && sb + 63u < tie_hi) { PA_SSTAT(59, 1); break; }  // between the ties, and nothing shares more
      const WidestWindow ww = begin_widest_window(mini_wpos, m1, b, has, i_max, count_windows);
      const uint32_t wp = ww.wp, wp_next = ww.wp_next, w_end = ww.w_end;
      const int32_t bar = shared_bar(c_best, best_shared, floor_bar);
      uint32_t held = 0;  // seed hits inside the begin's widest window: no window of the begin shares more
      for (uint32_t i = 0; i < nh; ++i) held += (s_hc[i] == c && s_hw[i] >= wp && s_hw[i] < w_end) ? 1u : 0u;
      const bool between = kSparseEnds && c_best >= 0 && b > tie_lo && b < tie_hi;  // a tie here changes nothing
      const bool pending = has && (int32_t)held >= (between ? max(bar, c_best + 1) : bar);
      PA_SSTAT(58, __popcll(__ballot(has && (int32_t)held >= bar && !pending)));  // begins left out because they could only tie
      if (!__any(pending)) break;  // (the next group)
      PA_SSTAT(50, 1);  // groups of 64 begins with a begin that holds enough hits
      const uint32_t first_lane = (uint32_t)__builtin_ctzll(__ballot(pending));
      const uint32_t base = sb + first_lane, n = min(m1 - base, kSparseCap);
      __syncthreads();
      uint32_t hh[kPer];
      bool any_dup = false;
      uint32_t w_raw[kPer];  // (the first entry's window id from lane 0's first load, as in map_segments_kernel)
      int32_t p_raw[kPer];
#pragma unroll
      for (int q = 0; q < kPer; ++q) {  // all the loads before any is looked at
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
        hh[q] = in ? h : 0xffffffffu;
        any_dup = any_dup || (in && pv >= (int32_t)base);
        s_refw[x] = (uint16_t)((dw > 0xfffeu || !in) ? 0xffffu : dw);
      }
      if (__any(any_dup)) { overflow = true; break; }  // a hash twice in the stretch: the windows' distinct hashes are the general kernel's to count
      if (lane < kWords) s_hitbits[lane] = 0u;
      __syncthreads();
      const bool at_end = base + n == m1;
      auto first_at_or_after = [&](uint32_t lo, uint32_t target) -> uint32_t {
        uint32_t hi = n;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((uint32_t)s_refw[mid] < target) lo = mid + 1; else hi = mid; }
        return lo;
      };
      const bool lane_on = pending && lane >= first_lane;
      uint32_t xs = 0, xe_lo = 0, xe_hi = 0;
      // the end of a begin's first window: every begin from the first pending one on looks for it (a target past 0xfffe finds
      // nothing: the window runs past the stretch) ...
      const bool lane_has = has && lane >= first_lane;
      if (lane_has) {
        xs = b - base;
        xe_lo = first_at_or_after(min(xs, n), wp + count_windows - wbase);
      }
      // ... and the end of its LAST window is where the next begin's first window ends, or one entry before that when this very
      // entry comes in at the next begin's position (as in map_segments_kernel: one search per begin instead of two); the last
      // begin of the slide and the last lane search themselves
      {
        const uint32_t xe_lo_next = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(min(lane + 1u, 63u) << 2), (int)xe_lo);
        const bool by_neighbour = lane < 63u && b + 1u < b_hi;
        uint32_t xe_own = 0;
        const uint64_t own = __ballot(lane_on && !by_neighbour);  // (one lane at most: its search is the whole wave's, 64 entries at once)
        if (own) {
          const int src = __builtin_ctzll(own);
          const uint32_t lo0 = (uint32_t)__builtin_amdgcn_readlane((int)xe_lo, src), tgt = (uint32_t)__builtin_amdgcn_readlane((int)(w_end - wbase), src);
          const uint32_t x = lo0 + lane;
          const uint64_t lt = __ballot(x < n && (uint32_t)s_refw[min(x, n - 1u)] < tgt);
          xe_own = lt == ~0ULL ? first_at_or_after(lo0 + 64u, tgt) : lo0 + (uint32_t)__popcll(lt);
        }
        if (lane_on) {
          if (by_neighbour) {
            const bool comes_in_there = xe_lo_next > 0u && (uint32_t)s_refw[xe_lo_next - 1u] == wp_next + count_windows - 1u - wbase;
            xe_hi = xe_lo_next - (comes_in_there ? 1u : 0u);
          } else {
            xe_hi = xe_own;
          }
        }
      }
      // a window runs past the stretch, or past what a 16-bit offset from the stretch's first window id can say (entries that
      // far are all kept as 0xffff: at the contig's end they would all count as inside): the general kernel's
      if (__any(lane_on && (w_end - wbase > 0xfffeu || !(xe_hi < n || at_end)))) { overflow = true; break; }
      // where the hits sit in the stretch
      if (lane < nh) {
        uint32_t p = 0xffffffffu;
        if (s_hc[lane] == c && s_hw[lane] >= wbase && s_hw[lane] - wbase < 0xffffu) {
          const uint32_t x = first_at_or_after(0u, s_hw[lane] - wbase);
          if (x < n && (uint32_t)s_refw[x] == s_hw[lane] - wbase) p = x;
        }
        s_pos[lane] = p;
        if (p != 0xffffffffu) atomicOr(&s_hitbits[p >> 5], 1u << (p & 31u));
      }
      __syncthreads();
      // per hit: the stretch entries that are reference-only and below the hit's hash, as bits, with the counts of the bits
      // before each word.  An entry that carries a hit's hash IS one of the segment's hits (every occurrence of a hash of the
      // sketch in this genome is one: the sparse kernel takes fragments that lost no hash to the frequency cut), so the
      // matching entries are the hits' own places -- one bit mask, not a comparison per entry and hit --, and with their
      // hashes set to "above everything" the mask of a hit is ONE comparison per entry: the compare's result is the ballot.
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const uint32_t word = s_hitbits[2u * (uint32_t)q + (lane >> 5)];
        hh[q] = ((word >> (lane & 31u)) & 1u) ? 0xffffffffu : hh[q];
      }
      for (uint32_t i = 0; i < nh; ++i) {
        const uint32_t ph = s_ph[i];
        uint64_t mb[kPer];
#pragma unroll
        for (int q = 0; q < kPer; ++q) mb[q] = __ballot(hh[q] < ph);  // (entries past the stretch's end hold 0xffffffff: below no hash)
        if (lane == 0) {
#pragma unroll
          for (int q = 0; q < kPer; ++q) reinterpret_cast<uint2 *>(&s_B[i][0])[q] = make_uint2((uint32_t)mb[q], (uint32_t)(mb[q] >> 32));
        }
      }
      __syncthreads();
      static_assert(kWords <= 16u && kSparseHits % 4u == 0u, "a row of sixteen lanes scans one hit's words");
      for (uint32_t i0 = 0; i0 < nh; i0 += 4u) {  // four hits per turn: a row of sixteen lanes each
        const uint32_t i = i0 + (lane >> 4), wd = lane & 15u;
        const bool on = i < nh && wd < kWords;
        const uint32_t pc = on ? (uint32_t)__popc(s_B[i][wd]) : 0u;
        const uint32_t inc = pa_dev::row_incl_scan_dpp(pc);
        if (on) s_P[i][wd] = inc - pc;
        if (on && wd == kWords - 1u) { s_P[i][kWords] = inc; s_B[i][kWords] = 0u; }
      }
      __syncthreads();
      // every state of every pending begin: the window holds the stretch entries [xs, e), e from the begin's first end to its
      // last -- two states per turn: what a hit costs (where it sits, its count at the window's start) is paid once for both
      int32_t lane_best = -1;
      const uint32_t most = pa_dev::wave_max_dpp(lane_on ? xe_hi - xe_lo + 1u : 0u);
      // per hit, once per begin: the hit is shared while the window's count of reference-only entries below its hash stays
      // below room = s - rank + (that count at the window's start); 0: the hit lies before the begin
      uint32_t room[kSparseHits];
#pragma unroll
      for (uint32_t i = 0; i < kSparseHits; ++i) {
        room[i] = 0u;
        if (i < nh) {
          const uint32_t p = s_pos[i];
          if (lane_on && p != 0xffffffffu && p >= xs) {
            const uint32_t ws = xs >> 5;
            room[i] = s - s_hr[i] + s_P[i][ws] + (uint32_t)__popc(s_B[i][ws] & ((1u << (xs & 31u)) - 1u));  // (s > rank: never 0 for a hit inside)
          }
        }
      }
      for (uint32_t t = 0; t < most; t += 2u) {
        const uint32_t e0 = xe_lo + t, e1 = e0 + 1u;
        if (!(lane_on && e0 <= xe_hi)) continue;
        const bool second = e1 <= xe_hi;
        int32_t shared0 = 0, shared1 = 0;
#pragma unroll
        for (uint32_t i = 0; i < kSparseHits; ++i) {
          if (i >= nh) break;
          const uint32_t p = s_pos[i];
          if (!(room[i] != 0u && p < e1)) continue;  // (in neither window)
          const uint32_t w0 = e0 >> 5, word = s_B[i][w0];
          const uint32_t c0 = s_P[i][w0] + (uint32_t)__popc(word & ((1u << (e0 & 31u)) - 1u));
          const uint32_t c1 = c0 + ((word >> (e0 & 31u)) & 1u);  // (the window one entry longer: entry e0 on top)
          shared0 += (p < e0 && c0 < room[i]) ? 1 : 0;
          shared1 += (c1 < room[i]) ? 1 : 0;
        }
        lane_best = max(lane_best, max(shared0, second ? shared1 : -1));
      }
      PA_SSTAT(51, __popcll(__ballot(lane_on)));                                  // begins evaluated
      PA_SSTAT(52, wave_sum(lane_on ? xe_hi - xe_lo + 1u : 0u));                  // states evaluated
      const int32_t group_best = (int32_t)pa_dev::wave_max_dpp(lane_on ? (uint32_t)(lane_best + 1) : 0u) - 1;
      if (__any(lane_on) && group_best >= c_best) {
        const uint64_t top = __ballot(lane_on && lane_best == group_best);
        PA_SSTAT(53, __popcll(top));  // begins tying the best so far of their candidate when their group is folded (an upper count of the ties)
        const bool better = fold_ties(group_best, top, wp, c_best, c_first, c_last);
        const uint32_t b_first = sb + (uint32_t)__builtin_ctzll(top), b_last = sb + 63u - (uint32_t)__builtin_clzll(top);
        tie_hi = better ? b_last : max(tie_hi, b_last);
        tie_lo = better ? b_first : min(tie_lo, b_first);
      }
      } while (false);
    }
    if (overflow) break;
    PA_SSTAT(54, c_best >= 0 ? 1u + ((tie_lo - b_lo) / 64u != (tie_hi - b_lo) / 64u ? 1u : 0u) : 0u);  // groups that hold the candidate's first or last tying begin: what any order has to evaluate
    if (candidate_is_the_mapping(c_best, best_shared)) { best_shared = c_best; best_c = c; best_first = c_first; best_last = c_last; }  // (of equals, the last)
  }
  if (overflow) {  // (rare: one draw per such segment)
    if (lane == 0) {
      const uint32_t slot = atomicAdd(over_n, 1u);
      over_a0[slot] = a0; over_nh[slot] = nh; over_f[slot] = f;
    }
    return;
  }
  if (lane == 0 && best_shared >= 0 && (uint32_t)best_shared >= tab_min_shared[s]) {
    const unsigned long long packed = mapping_packed(best_shared, s);
    const uint64_t bin = mapping_bin(contig_bin_off[best_c], best_first, best_last, frag_len);
    atomicMax(&table[(uint64_t)frag_genome_local[f] * table_stride + bin], packed);
  }
}
