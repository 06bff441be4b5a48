// fragani_seed.inc -- part of fragani.hip (included there, inside its anonymous namespace: one translation unit): fragment sketches and seed hits: sketches as slices of the genome's minimizers, hits bucketed by reference genome (one fragment per workgroup, staged in LDS), segment lists, the tiny-segment filter, the paths that order hits as a whole.

// ============================================================== 3. fragment sketches
// fastANI sketches a fragment on its own: winnowing restarts at the fragment's first residue, and the first minimizer is
// selected at the window of the first USED k-mer at or after the fragment's w-th.  Here a fragment's sketch is a slice of its
// genome's minimizers, and that window is all the slice needs to know: d = the windows at the fragment's start at which
// nothing is selected = the k-mers from the w-th on that equal their own reverse complement (both strands hash alike; a
// residue that is not ACGT counts as the N it is hashed as, and stays where it is in the reverse complement: a run of N is
// such a k-mer), 0 nearly always; count_windows when no k-mer of the fragment is used from there on.
// One thread per fragment of the batch (the answer is in the first k-mer nearly always; the wave that builds the sketch
// would only wait for it).  (x0: arena position of the fragment's w-th k-mer.)
__global__ __launch_bounds__(kThreads) void windows_without_selection_kernel(
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask, uint64_t arena_bases,
    const uint64_t *__restrict__ contig_start, uint32_t k, uint32_t w, const uint32_t *__restrict__ frag_contig,
    const uint32_t *__restrict__ frag_no, uint32_t n_frags, uint32_t frag_len, uint32_t count_windows,
    uint32_t *__restrict__ frag_d, AmbiguousList amb) {
  const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_frags) return;
  const uint64_t x0 = contig_start[frag_contig[f]] + (uint64_t)frag_no[f] * frag_len + w - 1u;
  const uint32_t k_mask = k == 16u ? 0xffffffffu : ((1u << (2u * k)) - 1u);
  const uint64_t nw = arena_bases >> 4, nm = arena_bases >> 5;
  uint32_t d = 0;
  for (; d < count_windows; ++d) {
    const uint64_t x = x0 + d, wi = x >> 4, mi = x >> 5;
    const uint64_t w0 = wi < nw ? packed[wi] : 0u, w1 = wi + 1 < nw ? packed[wi + 1] : 0u;
    const uint32_t fwd = (uint32_t)(((w1 << 32) | w0) >> (2u * ((uint32_t)x & 15u))) & k_mask;  // base j in bits 2j, 2j+1
    const uint64_t m0 = mi < nm ? mask[mi] : 0xffffffffu, m1 = mi + 1 < nm ? mask[mi + 1] : 0xffffffffu;
    const uint32_t bad = (uint32_t)(((m1 << 32) | m0) >> ((uint32_t)x & 31u)) & ((1u << k) - 1u);
    // the reverse complement in the same layout: the 2-bit groups in reverse order, complemented; the unknown residues
    // in reverse order, as they are
    uint32_t r = __brev(fwd);
    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
    const uint32_t rc = (r >> (32u - 2u * k)) ^ k_mask;
    const uint32_t rbad = __brev(bad) >> (32u - k);
    uint32_t known = ~bad & 0xffffu;  // one bit per residue -> two
    known = (known | (known << 8)) & 0x00ff00ffu;
    known = (known | (known << 4)) & 0x0f0f0f0fu;
    known = (known | (known << 2)) & 0x33333333u;
    known = (known | (known << 1)) & 0x55555555u;
    known |= known << 1;
    if (!(bad == rbad && ((fwd ^ rc) & known & k_mask) == 0u)) break;  // a used k-mer
    // residues that are not ACGT stay where they are in the reverse complement: the strands are the same text only if the
    // letters at mirrored positions are the same letter (all N without a list)
    if (bad && amb.n) {
      bool same = true;
      for (uint32_t rest = bad; rest && same; rest &= rest - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(rest);
        if (j < k - 1u - j) same = ambiguous_letter(amb, x + j) == ambiguous_letter(amb, x + (k - 1u - j));
      }
      if (!same) break;  // a used k-mer
    }
  }
  frag_d[f] = d;
}

// The fragment's hashes bucketed by their top kQtBits bits -- first rank (10 bits) | hashes in the bucket (6 bits, clamped to 63) per
// bucket --: the mapping kernel finds a reference minimizer's rank among the fragment's hashes as the bucket's first rank
// plus a search among the bucket's few hashes.  Made here, once per fragment (q_tab: kQtBuckets 16-bit entries each).
constexpr uint32_t kQtBits = 9, kQtBuckets = 1u << kQtBits, kQtShift = 32u - kQtBits;
// fetch-and-add on a 16-bit LDS counter through a 32-bit atomic on the word that holds it (little-endian halves;
// the counts stay below 2^16, so the low half never carries into the high one)
__device__ __forceinline__ uint32_t atomicAdd_u16(uint16_t *counters, uint32_t idx) {
  uint32_t *word = reinterpret_cast<uint32_t *>(counters) + (idx >> 1);
  const uint32_t old = atomicAdd(word, (idx & 1u) ? 0x10000u : 1u);
  return (idx & 1u) ? (old >> 16) : (old & 0xffffu);
}

// one wave per fragment: slice of the contig's minimizers, sorted by (hash, slice index), first of each hash kept
__global__ __launch_bounds__(kThreads) void query_sketch_kernel(
    const uint32_t *__restrict__ frag_d, const uint32_t *__restrict__ frag_contig, const uint32_t *__restrict__ frag_no, uint32_t n_frags, uint32_t frag_len,
    uint32_t count_windows, const uint32_t *__restrict__ contig_mini_off, const uint32_t *__restrict__ contig_bucket_off,
    const uint32_t *__restrict__ bucket_first, const uint32_t *__restrict__ mini_hash,
    const uint32_t *__restrict__ mini_wpos, const uint32_t *__restrict__ mini_id, const uint32_t *__restrict__ post_start,
    uint32_t *__restrict__ q_hash, uint32_t *__restrict__ q_pos /* posting list length */,
    uint32_t *__restrict__ q_id /* first posting */, uint32_t *__restrict__ q_s,
    uint32_t *__restrict__ hit_count, uint32_t *__restrict__ overflow, uint32_t *__restrict__ max_hits,
    uint32_t *__restrict__ q_cut /* hashes of the sketch that lost seed hits to the frequency cut */,
    const uint4 *__restrict__ lookup /* null: every minimizer knows its hash id */, uint32_t lookup_bits, uint32_t *__restrict__ q_tab) {
  __shared__ uint64_t s_key[kThreads / 64][kQMax];
  __shared__ __attribute__((aligned(16))) uint16_t s_qt[kThreads / 64][kQtBuckets];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t f = blockIdx.x * (kThreads / 64) + wave;
  const bool active = f < n_frags;  // every wave takes part in the barriers below
  uint64_t *key = s_key[wave];
  uint32_t p = 0, b0 = 0, n = 0;
  if (active) {
    const uint32_t c = frag_contig[f];
    p = frag_no[f] * frag_len;
    const uint32_t m0 = contig_mini_off[c], m1 = contig_mini_off[c + 1];
    const uint32_t bb = contig_bucket_off[c], nb = contig_bucket_off[c + 1] - bb - 1;
    const uint32_t b = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, p);
    const uint32_t e = wpos_lower_bound(mini_wpos, bucket_first, bb, nb, p + count_windows);
    // the minimizer recorded last before the fragment belongs to its sketch unless a new one is recorded by the first
    // window at which the fragment, sketched alone, selects any
    const uint32_t d = frag_d[f];  // windows_without_selection_kernel
    const bool fresh = b < m1 && mini_wpos[b] <= p + d;
    b0 = (!fresh && b > m0) ? b - 1 : b;
    n = d < count_windows ? e - b0 : 0u;  // (no used k-mer from the w-th on: no sketch)
  }
  // A slice of more than kQMax minimizers is low-complexity sequence: inside a homopolymer run or an array of a short
  // unit every window records its (rightmost) minimum anew -- one minimizer per position, all with the same hash.  Runs of
  // equal hashes are taken as one entry each on the way in (the sketch is the set of hashes); only a slice that still
  // holds more than kQMax entries is refused.
  const bool long_slice = n > (uint32_t)kQMax;  // (uniform: one fragment per wave)
  if (long_slice) {
    uint32_t o = 0, carry = 0;
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t e = base + lane;
      const uint32_t h = e < n ? mini_hash[b0 + e] : 0u;
      uint32_t before = (uint32_t)__shfl_up((int)h, 1, 64);
      if (lane == 0) before = carry;
      const bool keep = e < n && (e == 0u || h != before);
      const uint64_t bal = __ballot(keep);
      const uint32_t at = o + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL));
      if (keep && at < (uint32_t)kQMax) key[at] = ((uint64_t)h << 16) | e;  // (e <= count_windows <= 65 535)
      o += (uint32_t)__popcll(bal);
      carry = (uint32_t)__shfl((int)h, 63, 64);
    }
    if (o > (uint32_t)kQMax) { if (lane == 0) atomicAdd(overflow, 1u); o = kQMax; }
    n = o;
    __builtin_amdgcn_wave_barrier();
  }
  // the slice's (hash, slice index) keys ordered in registers, E = 1, 2, 4 or 8 per lane by the size of the slice, and
  // left in LDS for the pass below (every wave has its own keys: no barrier between the waves of the workgroup)
  auto sort_slice = [&](auto e_tag) {
    constexpr int E = decltype(e_tag)::value;
    uint64_t k[E];
    if (long_slice) {
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
        k[q] = e < n ? key[e] : ~0ULL;
      }
    } else if (n) {  // (uniform: one fragment per wave)
      uint32_t hq[E];  // loads without a branch, all in flight together: past the slice its last minimizer, discarded
#pragma unroll
      for (int q = 0; q < E; ++q) hq[q] = mini_hash[b0 + min(lane * (uint32_t)E + (uint32_t)q, n - 1u)];
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const uint32_t e = lane * (uint32_t)E + (uint32_t)q;
        k[q] = e < n ? (((uint64_t)hq[q] << 16) | e) : ~0ULL;
      }
    } else {
#pragma unroll
      for (int q = 0; q < E; ++q) k[q] = ~0ULL;
    }
    __builtin_amdgcn_wave_barrier();  // (a long slice: every lane has its entries before any is overwritten)
    bitonic_sort_lanes<E, uint64_t>(k, lane);
#pragma unroll
    for (int q = 0; q < E; ++q) key[lane * (uint32_t)E + (uint32_t)q] = k[q];
  };
  if (n <= 64u) sort_slice(std::integral_constant<int, 1>{});
  else if (n <= 128u) sort_slice(std::integral_constant<int, 2>{});
  else if (n <= 256u) sort_slice(std::integral_constant<int, 4>{});
  else sort_slice(std::integral_constant<int, 8>{});
  __builtin_amdgcn_wave_barrier();
  if (!active) return;
  uint16_t *qt = s_qt[wave];
  for (uint32_t i = lane; i < kQtBuckets / 2u; i += 64) reinterpret_cast<uint32_t *>(qt)[i] = 0;
  __builtin_amdgcn_wave_barrier();
  // keep the first entry of every hash run (smallest slice index = smallest window id)
  uint32_t s = 0, hits = 0, cut_hashes = 0;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t i = base + lane;
    bool keep = false;
    uint32_t h = 0, idx = 0;
    if (i < n) {
      h = (uint32_t)(key[i] >> 16);
      idx = (uint32_t)(key[i] & 0xffffu);
      keep = (i == 0) || ((uint32_t)(key[i - 1] >> 16) != h);
    }
    const uint64_t bal = __ballot(keep);
    if (keep) {
      const uint32_t o = s + __popcll(bal & ((1ULL << lane) - 1ULL));
      // the minimizer's posting list as (first posting, length): the seeding kernels then go straight to the postings
      // instead of through two more dependent, uncoalesced reads of post_start per list
      uint32_t lo = 0, cnt = 0, mark = 0;  // (a hash the dictionary does not hold: an empty list)
      if (lookup) {  // the dictionary of the reference range only: by the hash's value
        const uint32_t mask = (1u << lookup_bits) - 1u;
        for (uint32_t slot = lookup_slot(h, lookup_bits);; slot = (slot + 1u) & mask) {
          const uint4 entry = lookup[slot];
          if (entry.y == 0xffffffffu) break;  // an empty slot: not there
          if (entry.x == h) { lo = entry.y; cnt = entry.z & 0x7fffffffu; mark = entry.z >> 31; break; }
        }
      } else {
        const uint32_t id_and_mark = mini_id[b0 + idx], id = id_and_mark & 0x7fffffffu;  // top bit: the hash lost seed hits to the frequency cut
        lo = post_start[id];
        cnt = post_start[id + 1] - lo;
        mark = id_and_mark >> 31;
      }
      q_hash[(uint64_t)f * kQMax + o] = h;
      atomicAdd_u16(qt, h >> kQtShift);
      q_pos[(uint64_t)f * kQMax + o] = cnt;
      q_id[(uint64_t)f * kQMax + o] = lo;
      hits += cnt;
      cut_hashes += mark;
    }
    s += __popcll(bal);
  }
  hits = wave_sum(hits);
  cut_hashes = wave_sum(cut_hashes);
  {  // the bucket table of the sketch
    __builtin_amdgcn_wave_barrier();
    constexpr uint32_t kOwnB = kQtBuckets / 64u;  // consecutive buckets per lane
    uint32_t cntb[kOwnB], local = 0;
#pragma unroll
    for (uint32_t q = 0; q < kOwnB; ++q) { cntb[q] = qt[lane * kOwnB + q]; local += cntb[q]; }
    uint32_t run = wave_excl_scan(local, lane);
    uint32_t packed[kOwnB / 2u];
#pragma unroll
    for (uint32_t q = 0; q < kOwnB; ++q) {
      const uint32_t e = run | (min(cntb[q], 63u) << 10);
      packed[q / 2u] = (q & 1u) ? packed[q / 2u] | (e << 16) : e;
      run += cntb[q];
    }
    static_assert(kOwnB == 8, "four words per lane");
    reinterpret_cast<uint4 *>(q_tab + (uint64_t)f * (kQtBuckets / 2u))[lane] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  }
  if (lane == 0) {
    q_s[f] = s;
    q_cut[f] = cut_hashes;
    hit_count[f] = hits;
    // running maxima of the batch; look first, most fragments do not raise them
    if (hits > __builtin_nontemporal_load(max_hits)) atomicMax(max_hits, hits);
    if (s > __builtin_nontemporal_load(max_hits + 1)) atomicMax(max_hits + 1, s);
  }
}

// ============================================================== 4. seed hits
__global__ __launch_bounds__(kThreads) void fill_hits_kernel(
    uint32_t n_frags, const uint32_t *__restrict__ q_pos, const uint32_t *__restrict__ q_id,
    const uint32_t *__restrict__ q_s, const uint32_t *__restrict__ hit_off, const uint32_t *__restrict__ post_start,
    const uint32_t *__restrict__ sorted_idx, const uint32_t *__restrict__ mini_wpos,
    const uint32_t *__restrict__ mini_contig, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (f >= n_frags) return;
  const uint32_t s = q_s[f];
  uint32_t base = hit_off[f];
  for (uint32_t i0 = 0; i0 < s; i0 += 64) {
    const uint32_t i = i0 + lane;
    uint32_t lo = 0, n = 0;
    if (i < s) {
      lo = q_id[(uint64_t)f * kQMax + i];  // (first posting, length) as query_sketch_kernel left them
      n = q_pos[(uint64_t)f * kQMax + i];
    }
    const uint32_t ex = wave_excl_scan(n, lane);
    for (uint32_t t = 0; t < n; ++t) {
      const uint32_t g = sorted_idx[lo + t];
      keys[base + ex + t] = hit_key_of_fragment(f, place_of(mini_contig[g], mini_wpos[g]));
      vals[base + ex + t] = i;  // the rank of the hit's hash among the fragment's (the sketch is in hash order)
    }
    base += wave_sum(n);
  }
}

__global__ __launch_bounds__(kThreads) void segment_heads_kernel(const uint64_t *__restrict__ keys, uint32_t n,
                                                                 const uint32_t *__restrict__ contig_genome,
                                                                 uint32_t *__restrict__ flags) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  bool head = i == 0;
  if (!head) {
    const uint64_t a = keys[i - 1], b = keys[i];
    head = hit_fragment(a) != hit_fragment(b) || contig_genome[hit_contig(a)] != contig_genome[hit_contig(b)];
  }
  flags[i] = head ? 1u : 0u;
}
__global__ __launch_bounds__(kThreads) void segment_starts_kernel(const uint32_t *__restrict__ flags,
                                                                  const uint32_t *__restrict__ pos, uint32_t n,
                                                                  uint32_t *__restrict__ seg_start) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) seg_start[pos[i]] = i;
  if (i == n - 1) seg_start[pos[i] + flags[i]] = n;
}

// ---- hits of one fragment, bucketed by reference genome --------------------------------------------
// One wave per fragment and an LDS counter per reference genome: count the postings of the fragment's
// minimizers per genome (from the 2-byte genome of every posting: a list of ~15 is one 64-byte sector; the list
// bounds come coalesced from query_sketch_kernel), scan, then write every hit into its genome's slice of the
// fragment's hit range.
// The (fragment, genome) segments fall out of the scan, so the ones that can hold an L1 run (>= min_hits
// seed hits) are listed right here; nothing is sorted -- the mapping kernel orders the <= kHitCap hits of a
// segment in LDS, longer segments (repeats) are listed for segment_sort.  Eight lanes walk one posting
// list, so a wave reads 8 lists at a time in 64-byte pieces.
constexpr int kBucketWaves = 4;
__global__ __launch_bounds__(kBucketWaves * 64) void bucket_hits_kernel(
    uint32_t n_frags, const uint32_t *__restrict__ q_pos, const uint32_t *__restrict__ q_id,
    const uint32_t *__restrict__ q_s, const uint32_t *__restrict__ hit_off, const uint16_t *__restrict__ post_genome,
    const uint64_t *__restrict__ post_cw, uint32_t n_genomes, const uint32_t *__restrict__ tab_min_hits,
    uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
    uint32_t *__restrict__ seg_a0, uint32_t *__restrict__ seg_nh, uint32_t *__restrict__ seg_f, uint32_t seg_cap,
    uint32_t *__restrict__ counters, unsigned long long *__restrict__ cursor64, uint32_t ref0, uint32_t ref1, bool write_all) {
  extern __shared__ uint32_t bk_lds[];
  __shared__ uint32_t s_part[kBucketWaves][2], s_draw[2];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t f = blockIdx.x * kBucketWaves + wave;
  const bool active = f < n_frags;  // a wave past the last fragment has an empty sketch and still takes part in the barriers
  uint32_t *hist = bk_lds + (uint64_t)wave * n_genomes;
  const uint32_t s = active ? q_s[f] : 0u;
  const uint32_t base = active ? hit_off[f] : 0u;
  for (uint32_t g = lane; g < n_genomes; g += 64) hist[g] = 0;
  // The posting list of every minimizer of the fragment, (first posting, length), into registers: lane l holds the
  // lists of minimizers l, l + 64, ...  Two rounds of independent loads instead of a chain of three dependent ones
  // per group of eight lists.
  constexpr int kListRegs = kQMax / 64;
  uint32_t lo_r[kListRegs], n_r[kListRegs];
#pragma unroll
  for (int j = 0; j < kListRegs; ++j) {
    const uint32_t i = (uint32_t)j * 64u + lane;
    const bool in = i < s;
    lo_r[j] = in ? q_id[(uint64_t)f * kQMax + i] : 0u;  // coalesced: (first posting, length) from query_sketch_kernel
    n_r[j] = in ? q_pos[(uint64_t)f * kQMax + i] : 0u;
  }
  __builtin_amdgcn_wave_barrier();
  // Sixteen lists per step, 32 lanes' worth of slots each: a lane has eight independent posting loads in flight (the
  // kernel waits on memory 93 % of the time; what counts is how many loads are outstanding).  Lists longer than 32
  // (repeat families) take further rounds of the same step.
  constexpr int kLoads = 8;
  auto for_each_posting = [&](const auto *__restrict__ postings, auto &&visit) {
    using Elem = std::remove_cv_t<std::remove_reference_t<decltype(postings[0])>>;
    for (uint32_t i0 = 0; i0 < s; i0 += 2u * kLoads) {
      uint32_t lo_blk = 0, n_blk = 0;  // this lane's pair of the 64 lists i0 belongs to
#pragma unroll
      for (int j = 0; j < kListRegs; ++j)
        if ((i0 >> 6) == (uint32_t)j) { lo_blk = lo_r[j]; n_blk = n_r[j]; }
      uint32_t lo_u[kLoads], n_u[kLoads];
      uint32_t longest = 0;
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const uint32_t i = i0 + 2u * (uint32_t)u + (lane >> 5);  // i0 is a multiple of 16: the 16 lists share one block of 64
        lo_u[u] = __shfl(lo_blk, (int)(i & 63u), 64);
        n_u[u] = __shfl(n_blk, (int)(i & 63u), 64);  // 0 past the fragment's last minimizer; every lane takes part in the shuffle
        longest = max(longest, n_u[u]);
      }
      longest = pa_dev::wave_max_dpp(longest);
      for (uint32_t r = 0; r < longest; r += 32) {
        const uint32_t slot = r + (lane & 31u);
        Elem cw[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) cw[u] = slot < n_u[u] ? postings[lo_u[u] + slot] : Elem(0);
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
          if (slot < n_u[u]) visit(i0 + 2u * (uint32_t)u + (lane >> 5), cw[u]);
      }
    }
  };
  // counting pass over the genome of every posting only (2 bytes each: a list of ~15 fits one 64-byte sector)
  for_each_posting(post_genome, [&](uint32_t, uint16_t g) { atomicAdd(&hist[g], 1u); });
  __builtin_amdgcn_wave_barrier();
  // exclusive scan over the genomes; then list the segments worth mapping.  The list cursors are global counters that
  // every workgroup of the launch draws from: ONE fetch-and-add per workgroup for both lists (atomics on one address
  // are served one after the other by the L2 -- with a draw per group of 64 genomes and wave, as this kernel had it,
  // 22 of its 23.7 ms per batch were spent queueing for that one address; profiles/r03_bucket_hits_ablation.txt).
  const uint32_t mh = s ? tab_min_hits[s] : 0xffffffffu;
  uint32_t carry = 0, n_small = 0, n_large = 0, n_big = 0, max_big = 0;
  for (uint32_t g0 = 0; g0 < n_genomes; g0 += 64) {
    const uint32_t g = g0 + lane;
    const uint32_t cnt = g < n_genomes ? hist[g] : 0u;
    const uint32_t off = carry + wave_excl_scan(cnt, lane);
    const bool keep = cnt >= mh && g >= ref0 && g < ref1;  // only the reference genomes asked for are mapped
    // the top bit marks a genome whose hits nobody will read (fewer than a run needs, or not asked for): the scatter
    // pass then does not write them -- lone 8-byte stores, a 64-byte sector each (offsets stay below 2^31)
    if (g < n_genomes) hist[g] = off | (keep ? 0u : 0x80000000u);
    const bool small = keep && cnt <= (uint32_t)kHitCapSmall;
    n_small += (uint32_t)__popcll(__ballot(small));
    n_large += (uint32_t)__popcll(__ballot(keep && !small));
    n_big += (uint32_t)__popcll(__ballot(keep && cnt > (uint32_t)kHitCap));
    if (keep && cnt > (uint32_t)kHitCap) max_big = max(max_big, cnt);
    carry += wave_sum(cnt);
  }
  const uint32_t total_hits = carry;
  if (n_big) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) max_big = max(max_big, (uint32_t)__shfl_xor((int)max_big, o, 64));
  }
  if (lane == 0) {
    s_part[wave][0] = n_small;
    s_part[wave][1] = n_large;
    if (n_big) { atomicAdd(&counters[1], n_big); atomicMax(&counters[2], max_big); }
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // both cursors in one 64-bit word: one draw per workgroup
    uint32_t ws = 0, wl = 0;
#pragma unroll
    for (int q = 0; q < kBucketWaves; ++q) { ws += s_part[q][0]; wl += s_part[q][1]; }
    unsigned long long got = 0;
    if (ws | wl) got = atomicAdd(cursor64, ((unsigned long long)wl << 32) | ws);
    s_draw[0] = (uint32_t)got;
    s_draw[1] = (uint32_t)(got >> 32);
  }
  __syncthreads();
  uint32_t s0 = s_draw[0], l0 = s_draw[1];
#pragma unroll
  for (int q = 0; q < kBucketWaves; ++q)
    if ((uint32_t)q < wave) { s0 += s_part[q][0]; l0 += s_part[q][1]; }
  if (n_small | n_large) {
    // short segments fill the list from the front, the ones over kHitCapSmall hits from the back: the two
    // classes are mapped by launches with different LDS footprints
    for (uint32_t g0 = 0; g0 < n_genomes; g0 += 64) {
      const uint32_t g = g0 + lane;
      uint32_t off = 0, cnt = 0;
      if (g < n_genomes) {
        off = hist[g] & 0x7fffffffu;
        cnt = (g + 1 < n_genomes ? (hist[g + 1] & 0x7fffffffu) : total_hits) - off;
      }
      const bool keep = cnt >= mh && g >= ref0 && g < ref1;
      const bool small = keep && cnt <= (uint32_t)kHitCapSmall, large = keep && !small;
      const uint64_t sm = __ballot(small), lm = __ballot(large);
      if (keep) {
        const uint64_t below = (1ULL << lane) - 1ULL;
        const uint32_t slot = small ? s0 + (uint32_t)__popcll(sm & below) : seg_cap - 1u - (l0 + (uint32_t)__popcll(lm & below));
        if (slot < seg_cap) { seg_a0[slot] = base + off; seg_nh[slot] = cnt; seg_f[slot] = f; }
      }
      s0 += (uint32_t)__popcll(sm);
      l0 += (uint32_t)__popcll(lm);
    }
  }
  __builtin_amdgcn_wave_barrier();
  // A hit carries the RANK of its hash among the fragment's hashes -- the sketch is in hash order, so that is the number i
  // of the posting list it comes from -- on top of its (contig, window id): the mapping kernel's bound on what a window
  // can share asks which of a window's hits lie below a pivot rank (kHitRankShift; the fragment itself is named by the
  // segment lists).
  // write_all: the batch is about to be ordered as a whole (a repeat family too long for an LDS sort), and that keeps
  // the (fragment, genome) slices in place only when every slot holds its own key with the fragment on top; the rank
  // then rides in the sort's payload.
  for_each_posting(post_cw, [&](uint32_t i, uint64_t cw) {
    const uint32_t at = atomicAdd(&hist[posting_genome(cw)], 1u);
    if (write_all) {
      keys[base + (at & 0x7fffffffu)] = hit_key_of_fragment(f, hit_place(cw));
      vals[base + (at & 0x7fffffffu)] = i;
    } else if (!(at & 0x80000000u)) {
      keys[base + at] = hit_key_of_rank(i, hit_place(cw));
    }
  });
}

// ---- the same for one fragment per WORKGROUP, the hits of the listed pairs staged in LDS ----------------------------
// bucket_hits_kernel above writes every hit of a listed pair with a lone 8-byte store into its genome's slice of the
// fragment's hit range: the eight hits of a 64-byte sector arrive at eight different times from eight posting lists, the
// L2 cannot hold the lines of all fragments in flight until they are full, and the counters show 19.6 written bytes per
// hit against 8 (profiles/r04_pmc_bucket_hits_summary.txt).  Here the eight waves of a workgroup share one fragment:
// they split its posting lists (a step of sixteen lists per wave and turn), count into ONE histogram in LDS, place the
// hits of the LISTED genomes in a compact LDS copy of their slices (21 KB on average at 1 000 genomes: the pairs that
// are not listed -- fewer hits than a run needs -- are not written at all), and then every listed slice leaves as a run
// of consecutive 8-byte stores -- whole sectors but for a slice's two ends.  A fragment whose listed hits do not fit the
// staging area (repeat families) writes them directly, as above.
constexpr int kStageWaves = 8;
__global__ __launch_bounds__(kStageWaves * 64) void bucket_hits_staged_kernel(
    uint32_t n_frags, const uint32_t *__restrict__ q_pos, const uint32_t *__restrict__ q_id,
    const uint32_t *__restrict__ q_s, const uint32_t *__restrict__ hit_off,
    const uint16_t *__restrict__ post_genome, const uint64_t *__restrict__ post_cw, uint32_t n_genomes,
    const uint32_t *__restrict__ tab_min_hits, uint64_t *__restrict__ keys, uint32_t *__restrict__ seg_a0,
    uint32_t *__restrict__ seg_nh, uint32_t *__restrict__ seg_f, uint32_t seg_cap, uint32_t *__restrict__ counters,
    unsigned long long *__restrict__ cursor64, uint32_t ref0, uint32_t ref1, uint32_t stage_cap) {
  extern __shared__ uint64_t st_lds[];
  uint64_t *stage = st_lds;                                           // [stage_cap] the listed slices, one after the other
  uint32_t *hist = reinterpret_cast<uint32_t *>(st_lds + stage_cap);  // [n_genomes] counts, then offsets in the fragment's hit range
  uint32_t *coff = hist + n_genomes;                                  // [n_genomes] cursors into `stage` (listed genomes)
  __shared__ uint32_t s_tot[kStageWaves][2], s_part[kStageWaves][2], s_draw[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t f = blockIdx.x;
  if (f >= n_frags) return;
  const uint32_t s = q_s[f], base = hit_off[f];
  for (uint32_t g = tid; g < n_genomes; g += kStageWaves * 64) hist[g] = 0;
  __syncthreads();
  // sixteen lists per step and wave, 32 lanes' worth of slots each, eight independent posting loads per lane in flight
  constexpr int kLoads = 8;
  auto for_each_posting = [&](const auto *__restrict__ postings, auto &&visit) {
    using Elem = std::remove_cv_t<std::remove_reference_t<decltype(postings[0])>>;
    for (uint32_t i0 = 2u * kLoads * wave; i0 < s; i0 += 2u * kLoads * kStageWaves) {
      uint32_t lo_u[kLoads], n_u[kLoads], longest = 0;
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const uint32_t i = i0 + 2u * (uint32_t)u + (lane >> 5);
        // (loads without a branch -- the row's last slot for a list past the sketch's end, discarded --: all sixteen in flight together)
        lo_u[u] = q_id[(uint64_t)f * kQMax + min(i, (uint32_t)kQMax - 1u)];  // (first posting, length) from query_sketch_kernel
        n_u[u] = q_pos[(uint64_t)f * kQMax + min(i, (uint32_t)kQMax - 1u)];
      }
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const uint32_t i = i0 + 2u * (uint32_t)u + (lane >> 5);
        lo_u[u] = i < s ? lo_u[u] : 0u;
        n_u[u] = i < s ? n_u[u] : 0u;
        longest = max(longest, n_u[u]);
      }
      longest = pa_dev::wave_max_dpp(longest);
      for (uint32_t r = 0; r < longest; r += 32) {
        const uint32_t slot = r + (lane & 31u);
        Elem cw[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) cw[u] = slot < n_u[u] ? postings[lo_u[u] + slot] : Elem(0);
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
          if (slot < n_u[u]) visit(i0 + 2u * (uint32_t)u + (lane >> 5), cw[u]);
      }
    }
  };
  // (The counting pass over the 8-byte postings instead of their 2-byte genomes -- so that the scatter pass finds them in the
  // caches -- was tried in round 6: seeding 70 ms per run against 63.5.)
  for_each_posting(post_genome, [&](uint32_t, uint16_t g) { atomicAdd(&hist[g], 1u); });
  __syncthreads();
  // exclusive scans over the genomes, 512 at a time (a wave per 64 genomes, the waves chained through their totals): of all
  // counts -- the offsets in the fragment's hit range -- and of the listed genomes' counts -- the offsets in `stage`
  const uint32_t mh = s ? tab_min_hits[s] : 0xffffffffu;
  uint32_t carry = 0, ccarry = 0, n_small = 0, n_large = 0, n_big = 0, max_big = 0;
  for (uint32_t g0 = 0; g0 < n_genomes; g0 += kStageWaves * 64) {
    const uint32_t g = g0 + tid;
    const uint32_t cnt = g < n_genomes ? hist[g] : 0u;
    const bool keep = cnt >= mh && g >= ref0 && g < ref1;
    const uint32_t kcnt = keep ? cnt : 0u;
    const uint32_t ex = wave_excl_scan(cnt, lane), wsum = wave_sum(cnt);
    const uint32_t kex = wave_excl_scan(kcnt, lane), kwsum = wave_sum(kcnt);
    if (lane == 0) { s_tot[wave][0] = wsum; s_tot[wave][1] = kwsum; }
    __syncthreads();
    uint32_t before = 0, chunk = 0, kbefore = 0, kchunk = 0;
#pragma unroll
    for (int q = 0; q < kStageWaves; ++q) {
      const uint32_t t = s_tot[q][0], kt = s_tot[q][1];
      before += (uint32_t)q < wave ? t : 0u; chunk += t;
      kbefore += (uint32_t)q < wave ? kt : 0u; kchunk += kt;
    }
    if (g < n_genomes) {
      hist[g] = (carry + before + ex) | (keep ? 0u : 0x80000000u);  // top bit: nobody will read this genome's hits
      coff[g] = ccarry + kbefore + kex;
    }
    const bool small = keep && cnt <= (uint32_t)kHitCapSmall;
    n_small += (uint32_t)__popcll(__ballot(small));
    n_large += (uint32_t)__popcll(__ballot(keep && !small));
    n_big += (uint32_t)__popcll(__ballot(keep && cnt > (uint32_t)kHitCap));
    if (keep && cnt > (uint32_t)kHitCap) max_big = max(max_big, cnt);
    carry += chunk;
    ccarry += kchunk;
    __syncthreads();  // s_tot is written again in the next turn
  }
  const uint32_t total_hits = carry;
  const bool staged = ccarry <= stage_cap;  // the listed hits fit the staging area (uniform over the workgroup)
  if (n_big) max_big = pa_dev::wave_max_dpp(max_big);
  if (lane == 0) {
    s_part[wave][0] = n_small;
    s_part[wave][1] = n_large;
    if (n_big) { atomicAdd(&counters[1], n_big); atomicMax(&counters[2], max_big); }
  }
  __syncthreads();
  if (tid == 0) {  // both list cursors in one 64-bit word: one draw per workgroup
    uint32_t ws = 0, wl = 0;
#pragma unroll
    for (int q = 0; q < kStageWaves; ++q) { ws += s_part[q][0]; wl += s_part[q][1]; }
    unsigned long long got = 0;
    if (ws | wl) got = atomicAdd(cursor64, ((unsigned long long)wl << 32) | ws);
    s_draw[0] = (uint32_t)got;
    s_draw[1] = (uint32_t)(got >> 32);
  }
  __syncthreads();
  uint32_t s0 = s_draw[0], l0 = s_draw[1];
#pragma unroll
  for (int q = 0; q < kStageWaves; ++q)
    if ((uint32_t)q < wave) { s0 += s_part[q][0]; l0 += s_part[q][1]; }
  if (n_small | n_large) {  // (uniform over the wave)
    for (uint32_t g0 = 0; g0 < n_genomes; g0 += kStageWaves * 64) {
      const uint32_t g = g0 + tid;
      uint32_t off = 0, cnt = 0;
      if (g < n_genomes) {
        off = hist[g] & 0x7fffffffu;
        cnt = (g + 1 < n_genomes ? (hist[g + 1] & 0x7fffffffu) : total_hits) - off;
      }
      const bool keep = cnt >= mh && g >= ref0 && g < ref1;
      const bool small = keep && cnt <= (uint32_t)kHitCapSmall, large = keep && !small;
      const uint64_t sm = __ballot(small), lm = __ballot(large);
      if (keep) {
        const uint64_t below = (1ULL << lane) - 1ULL;
        const uint32_t slot = small ? s0 + (uint32_t)__popcll(sm & below) : seg_cap - 1u - (l0 + (uint32_t)__popcll(lm & below));
        if (slot < seg_cap) { seg_a0[slot] = base + off; seg_nh[slot] = cnt; seg_f[slot] = f; }
      }
      s0 += (uint32_t)__popcll(sm);
      l0 += (uint32_t)__popcll(lm);
    }
  }
  // scatter pass.  Staged: a hit of a listed genome draws its place from the genome's cursor into `stage` (the offsets
  // in the hit range stay as they are: the copy below reads them); else from the genome's offset, which moves.
  if (staged) {
    for_each_posting(post_cw, [&](uint32_t i, uint64_t cw) {
      const uint32_t g = posting_genome(cw);
      if (!(hist[g] & 0x80000000u)) stage[atomicAdd(&coff[g], 1u)] = hit_key_of_rank(i, hit_place(cw));
    });
    __syncthreads();
    // the listed slices, from LDS to the hit array: a wave per genome, consecutive lanes consecutive hits.  A genome's
    // cursor stands at the END of its slice in `stage` now; its length is the distance to the next genome's offset.
    for (uint32_t g0 = 0; g0 < n_genomes; g0 += kStageWaves * 64) {
      const uint32_t g = g0 + tid;
      uint32_t off = 0, cnt = 0, cend = 0;
      bool keep = false;
      if (g < n_genomes) {
        const uint32_t v = hist[g];
        keep = !(v & 0x80000000u);
        off = v & 0x7fffffffu;
        cnt = (g + 1 < n_genomes ? (hist[g + 1] & 0x7fffffffu) : total_hits) - off;
        cend = coff[g];
      }
      for (uint64_t todo = __ballot(keep && cnt > 0u); todo; todo &= todo - 1) {
        const int src = __builtin_ctzll(todo);
        const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)off, src), n0 = (uint32_t)__builtin_amdgcn_readlane((int)cnt, src);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cend, src) - n0;
        for (uint32_t i = lane; i < n0; i += 64) keys[base + o0 + i] = stage[c0 + i];
      }
    }
  } else {
    __syncthreads();  // every offset has been read before the scatter pass moves it
    for_each_posting(post_cw, [&](uint32_t i, uint64_t cw) {
      const uint32_t at = atomicAdd(&hist[posting_genome(cw)], 1u);
      if (!(at & 0x80000000u)) keys[base + at] = hit_key_of_rank(i, hit_place(cw));
    });
  }
}

// Chance matches with unrelated genomes still leave millions of listed segments with a handful of hits and
// no valid L1 run.  One THREAD settles each segment of <= 8 hits here (sort its keys in registers, test the
// run condition of map_segments_kernel exactly) so that the mapping kernel does not spend a workgroup
// launch and a dozen dependent loads on it; longer segments pass through.
constexpr uint32_t kTinySegment = 8;
__global__ __launch_bounds__(kThreads) void prefilter_segments_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_a0, const uint32_t *__restrict__ seg_nh,
    const uint32_t *__restrict__ seg_f, uint32_t n_segs, const uint32_t *__restrict__ q_s,
    const uint32_t *__restrict__ tab_min_hits, const uint32_t *__restrict__ q_cut, uint32_t frag_len, uint32_t *__restrict__ out_a0,
    uint32_t *__restrict__ out_nh, uint32_t *__restrict__ out_f, unsigned long long *__restrict__ counter, uint32_t sparse_max) {
  // Kept segments of at most `sparse_max` hits (0: none) whose fragment lost no hash to the frequency cut are listed from
  // the BACK of the out arrays: map_sparse_kernel takes them, map_segments_kernel the ones listed from the front.
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t a0 = 0, nh = 0, f = 0;
  bool keep = false;
  if (i < n_segs) {
    a0 = seg_a0[i];
    nh = seg_nh[i];
    f = seg_f[i];
    if (nh > kTinySegment) {
      keep = true;
    } else {
      uint64_t k[kTinySegment];
#pragma unroll
      for (uint32_t j = 0; j < kTinySegment; ++j) k[j] = keys[a0 + min(j, nh - 1u)];  // (loads without a branch: all in flight together; nh >= 1)
#pragma unroll
      for (uint32_t j = 0; j < kTinySegment; ++j) k[j] = j < nh ? hit_place(k[j]) : ~0ULL;  // (contig, window id)
#pragma unroll
      for (uint32_t pass = 0; pass < kTinySegment; ++pass)  // odd-even transposition sort: 8 passes sort 8 keys
#pragma unroll
        for (uint32_t j = pass & 1u; j + 1 < kTinySegment; j += 2) {
          const uint64_t lo = k[j] < k[j + 1] ? k[j] : k[j + 1], hi = k[j] < k[j + 1] ? k[j + 1] : k[j];
          k[j] = lo;
          k[j + 1] = hi;
        }
      const uint32_t s = q_s[f];
      const uint32_t mh = s ? tab_min_hits[s] : 0xffffffffu;
#pragma unroll
      for (uint32_t a = 0; a < kTinySegment; ++a) {
#pragma unroll
        for (uint32_t z = a; z < kTinySegment; ++z) {  // z = a + mh - 1
          if (z + 1 == a + mh && z < nh && l1_run_valid(hit_contig(k[a]), hit_window(k[a]), hit_contig(k[z]), hit_window(k[z]), frag_len))
            keep = true;
        }
      }
    }
  }
  const bool sparse = keep && nh <= sparse_max && q_cut[f] == 0u;
  // one draw from the two list cursors (one 64-bit word) per workgroup (same-address atomics queue up in the L2, ~11 ns each)
  __shared__ uint32_t s_kept[kThreads / 64][2], s_base[2];
  const uint64_t km = __ballot(keep && !sparse), sm = __ballot(sparse);
  const uint32_t wave = threadIdx.x >> 6;
  if (lane == 0) { s_kept[wave][0] = (uint32_t)__popcll(km); s_kept[wave][1] = (uint32_t)__popcll(sm); }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0, ssum = 0;
#pragma unroll
    for (int q = 0; q < kThreads / 64; ++q) { sum += s_kept[q][0]; ssum += s_kept[q][1]; }
    const unsigned long long got = (sum | ssum) ? atomicAdd(counter, ((unsigned long long)ssum << 32) | sum) : 0ull;
    s_base[0] = (uint32_t)got;
    s_base[1] = (uint32_t)(got >> 32);
  }
  __syncthreads();
  if (keep) {
    uint32_t slot = s_base[sparse ? 1 : 0] + (uint32_t)__popcll((sparse ? sm : km) & ((1ULL << lane) - 1ULL));
#pragma unroll
    for (int q = 0; q < kThreads / 64; ++q)
      if ((uint32_t)q < wave) slot += s_kept[q][sparse ? 1 : 0];
    if (sparse) slot = n_segs - 1u - slot;  // from the back (n_segs slots in all: the two lists cannot meet)
    out_a0[slot] = a0;
    out_nh[slot] = nh;
    out_f[slot] = f;
  }
}

// the listed segments longer than kHitCap, as (start, length) pairs for frag_sort_kernel
__global__ __launch_bounds__(kThreads) void big_segments_kernel(const uint32_t *__restrict__ seg_a0,
                                                                const uint32_t *__restrict__ seg_nh, uint32_t n_segs,
                                                                uint32_t *__restrict__ big_a0,
                                                                uint32_t *__restrict__ big_nh,
                                                                uint32_t *__restrict__ counter) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_segs || seg_nh[i] <= (uint32_t)kHitCap) return;
  const uint32_t slot = atomicAdd(counter, 1u);
  big_a0[slot] = seg_a0[i];
  big_nh[slot] = seg_nh[i];
}

// ---- hits of one fragment, sorted by (contig, window) in LDS --------------------------------------
// fill_hits_kernel leaves the hits of fragment f contiguous at hit_off[f]; they only need ordering
// inside the fragment (the fragment number is the top of the key), so one workgroup sorts one fragment
// in LDS (bitonic on the 64-bit key with its 32-bit payload) instead of 8 radix passes over the
// whole batch.  Used when the busiest fragment has <= kFragSortMax hits.
constexpr uint32_t kFragSortMax = 8192;
constexpr int kFragSortThreads = 256;

__global__ __launch_bounds__(kFragSortThreads) void frag_sort_kernel(uint64_t *__restrict__ keys,
                                                                     uint32_t *__restrict__ vals,
                                                                     const uint32_t *__restrict__ hit_off,
                                                                     const uint32_t *__restrict__ hit_count,
                                                                     uint32_t np2_max, uint32_t rot) {
  // rot: bits the keys are turned left by while they are sorted -- 0 for keys with the fragment on top (one fragment's
  // hits: by contig and window id), 20 for the bucketed hits of one long segment, whose top bits hold the rank of the
  // hit's hash: ordered by (contig, window id) all the same
  extern __shared__ uint64_t fs_key[];
  uint32_t *fs_val = reinterpret_cast<uint32_t *>(fs_key + np2_max);
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  const uint32_t n = hit_count[f];
  if (n < 2) return;
  const uint32_t a0 = hit_off[f];
  uint32_t np2 = 2;
  while (np2 < n) np2 <<= 1;
  for (uint32_t i = tid; i < np2; i += kFragSortThreads) {
    const uint64_t key = i < n ? keys[a0 + i] : 0ULL;
    fs_key[i] = i < n ? (rot ? (key << rot) | (key >> (64u - rot)) : key) : ~0ULL;
    fs_val[i] = i < n ? vals[a0 + i] : 0u;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= np2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < (np2 >> 1); t += kFragSortThreads) {
        const uint32_t i = 2u * t - (t & (j - 1u));
        const uint32_t l = i + j;
        const uint64_t a = fs_key[i], b = fs_key[l];
        const bool up = (i & k) == 0u;
        if ((a > b) == up && a != b) {
          fs_key[i] = b;
          fs_key[l] = a;
          const uint32_t va = fs_val[i];
          fs_val[i] = fs_val[l];
          fs_val[l] = va;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < n; i += kFragSortThreads) {
    const uint64_t key = fs_key[i];
    keys[a0 + i] = rot ? (key >> rot) | (key << (64u - rot)) : key;
    vals[a0 + i] = fs_val[i];
  }
}

// keep the segments that can hold an L1 run at all: at least min_hits(s) seed hits
__global__ __launch_bounds__(kThreads) void segment_keep_kernel(const uint64_t *__restrict__ keys,
                                                                const uint32_t *__restrict__ seg_start, uint32_t n_segs,
                                                                const uint32_t *__restrict__ q_s,
                                                                const uint32_t *__restrict__ tab_min_hits,
                                                                const uint32_t *__restrict__ contig_genome, uint32_t ref0,
                                                                uint32_t ref1, uint32_t *__restrict__ keep) {
  const uint32_t seg = blockIdx.x * kThreads + threadIdx.x;
  if (seg >= n_segs) return;
  const uint32_t a0 = seg_start[seg], nh = seg_start[seg + 1] - a0;
  const uint64_t key = keys[a0];
  const uint32_t s = q_s[hit_fragment(key)];
  const uint32_t g = contig_genome[hit_contig(key)];
  keep[seg] = (s != 0 && nh >= tab_min_hits[s] && g >= ref0 && g < ref1) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void segment_list_kernel(const uint32_t *__restrict__ keep,
                                                                const uint32_t *__restrict__ pos, uint32_t n_segs,
                                                                uint32_t *__restrict__ seg_list) {
  const uint32_t seg = blockIdx.x * kThreads + threadIdx.x;
  if (seg < n_segs && keep[seg]) seg_list[pos[seg]] = seg;
}

// old path: the kept segments of the fully sorted hit list as (start, length) pairs
__global__ __launch_bounds__(kThreads) void segments_from_list_kernel(const uint32_t *__restrict__ seg_start,
                                                                      const uint32_t *__restrict__ seg_list,
                                                                      uint32_t n, uint32_t *__restrict__ seg_a0,
                                                                      uint32_t *__restrict__ seg_nh) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t seg = seg_list[i];
  seg_a0[i] = seg_start[seg];
  seg_nh[i] = seg_start[seg + 1] - seg_start[seg];
}
