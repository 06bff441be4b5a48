// fragani_index.inc -- part of fragani.hip (included there, inside its anonymous namespace: one translation unit): the reference index: minimizers of every contig (one pass, chained scan), dictionary of their hashes, postings, frequency cut; the register sort both later stages use.

// ============================================================== 1. minimizers
constexpr int kPPT = 8;                       // positions per thread
#ifndef PA_MINI_THREADS
#define PA_MINI_THREADS 256
#endif
constexpr int kMiniThreads = PA_MINI_THREADS; // threads of a workgroup of minimizer_kernel
#ifndef PA_MINI_HASH_GROUP
#define PA_MINI_HASH_GROUP 4
#endif
// k-mers hashed side by side before the scheduler may start on the next ones (0: all eight of a thread): the
// compiler interleaves what it is allowed to, and pays in registers -- 102 for eight, 80 for two or four
constexpr int kMiniHashGroup = PA_MINI_HASH_GROUP;
constexpr int kTile = kMiniThreads * kPPT;    // positions per workgroup, of which
constexpr int kHalo = 128;                    // the first 128 are look-back (needs w <= 64)
constexpr int kOwn = kTile - kHalo;

// One pass: every workgroup hashes and winnows its tile once, then learns where its minimizers go from the
// workgroups before it -- a chained scan with look-back (each publishes first the count of its own tile, then, once it
// knows it, the count of everything up to and including itself; a workgroup adds up published tile counts backwards
// until it meets such a running total).  Tiles are handed out by a ticket counter, so a workgroup only ever waits for
// workgroups that started before it.  `look` holds one 64-bit word per tile: state (0 nothing yet, 1 tile count,
// 2 running total) in the top two bits, the count below; `scalars`: [0] ticket (one counter), [1] total, [2] a wait ran out,
// [kTicketStride * (1 + x)] the ticket counter of XCD x (ticket_mode 1).
constexpr uint64_t kLookTile = 1ULL << 62, kLookTotal = 2ULL << 62;
constexpr uint32_t kTicketStride = 32;  // words between the per-XCD ticket counters in `scalars` (128 bytes: a line each), the first at kTicketStride
constexpr uint32_t kMiniScalarBytes = 4u * kTicketStride * 9u;
constexpr uint32_t kLookSpinLimit = 1u << 24;
// (A ticket per RUN of consecutive tiles was tried to take load off the ticket counter -- one address, ~11 ns per
// returning atomic, 2.6 million tiles in the 1 000 x 5 Mb run: a floor of 29 ms under this 58 ms kernel -- and is wrong
// for a chained scan: the first tile of a run waits for the last tile of the run before it, which its workgroup
// reaches last, so the workgroups execute one after the other: 34 s.)

// A k-mer that holds residues other than A, C, G, T: fastANI hashes the characters as they are (upper-cased; the reverse
// complement leaves what it does not know in place), so such a k-mer is a k-mer like any other -- only a k-mer equal to its
// own reverse complement (a run of N, for one) is passed over, as every k-mer whose two strands hash alike is.  The packed
// arena keeps two bits per residue and one "not ACGT" bit: such a residue is 'N' (by far the commonest) unless the arena's
// list of other letters (IUPAC codes, ...) holds its position -- one search per such residue, only here.
// Rare, and off the hot path: the bytes are put together one by one, the two multiplies of MurmurHash3 done in full.
// `codes`: residue j in bits 2j, 2j+1; `bad`: bit j set = residue j is not ACGT; `pos`: arena position of residue 0.
// Returns kSkip when the strands hash alike.
// The residues that are neither ACGT nor N, as the packers list them (pa_fragani_set_ambiguous): ascending arena
// positions and upper-cased bytes.  The letter at arena position `pos`, of a residue whose "not ACGT" bit is set.
struct AmbiguousList {
  const uint64_t *pos;
  const uint8_t *byte;
  uint32_t n;
};
__device__ __forceinline__ uint32_t ambiguous_letter(const AmbiguousList &amb, uint64_t pos) {
  uint32_t lo = 0, hi = amb.n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (amb.pos[mid] < pos) lo = mid + 1; else hi = mid;
  }
  return (lo < amb.n && amb.pos[lo] == pos) ? (uint32_t)amb.byte[lo] : (uint32_t)'N';
}

template <int K>
__device__ __forceinline__ uint32_t hash_kmer_with_unknowns(uint32_t codes, uint32_t bad, uint64_t pos, const AmbiguousList &amb) {
  constexpr int kWords = (K + 7) / 8;
  // the letters of the residues that are not ACGT, four to a word (only when the arena has a list: else every one is N)
  uint32_t letters[(K + 3) / 4];
#pragma unroll
  for (int q = 0; q < (K + 3) / 4; ++q) letters[q] = 0x4e4e4e4eu;  // "NNNN"
  if (amb.n) {
    for (uint32_t rest = bad; rest; rest &= rest - 1u) {
      const int j = __builtin_ctz(rest);
      const uint32_t ch = ambiguous_letter(amb, pos + (uint64_t)j);
#pragma unroll
      for (int q = 0; q < (K + 3) / 4; ++q)
        if ((j >> 2) == q) letters[q] = (letters[q] & ~(0xffu << (8 * (j & 3)))) | (ch << (8 * (j & 3)));
    }
  }
  uint32_t hs[2];
#pragma unroll
  for (int strand = 0; strand < 2; ++strand) {
    uint64_t P[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < kWords; ++q) {
      uint64_t word = 0;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int j = 8 * q + t;  // byte j of the strand's text
        if (j >= K) break;
        const int src = strand ? K - 1 - j : j;
        const uint32_t code = ((codes >> (2 * src)) & 3u) ^ (strand ? 3u : 0u);
        const uint32_t ch = ((bad >> src) & 1u) ? (letters[src >> 2] >> (8 * (src & 3))) & 0xffu : (0x54474341u >> (8 * code)) & 0xffu;  // "ACGT"
        word |= (uint64_t)ch << (8 * t);
      }
      P[q] = word * ((q & 1) ? kC2 : kC1);
    }
    hs[strand] = (uint32_t)murmur3_from_products<K>(P);
  }
  return hs[0] == hs[1] ? kSkip : (hs[0] < hs[1] ? hs[0] : hs[1]);
}

// The contig of every tile's first position, found once, side by side, by a thread per tile: inside minimizer_kernel the
// search through the contigs' starts was ten dependent loads in every tile's life -- a life that is mostly waiting.
__global__ __launch_bounds__(kThreads) void tile_contig_kernel(const uint64_t *__restrict__ contig_start, uint32_t n_contigs,
                                                                uint32_t n_tiles, uint32_t *__restrict__ tile_contig) {
  const uint32_t tile = blockIdx.x * kThreads + threadIdx.x;
  if (tile >= n_tiles) return;
  const int64_t first = (int64_t)tile * kOwn - kHalo;
  tile_contig[tile] = contig_of(contig_start, n_contigs, first > 0 ? (uint64_t)first : 0u);
}

template <int K>
__global__ __launch_bounds__(kMiniThreads) void minimizer_kernel(
    const uint32_t *__restrict__ packed, const uint32_t *__restrict__ mask, uint64_t arena_bases,
    const uint64_t *__restrict__ contig_start, const uint32_t *__restrict__ contig_len, uint32_t n_contigs, int w,
    unsigned long long *__restrict__ look, uint32_t *__restrict__ scalars, uint32_t cap, uint32_t *__restrict__ out_hash,
    uint32_t *__restrict__ out_wpos, uint32_t *__restrict__ out_contig, uint32_t n_tiles, AmbiguousList amb, uint32_t ticket_mode,
    const uint32_t *__restrict__ tile_contig) {
  static_assert(K >= 8 && K <= 16, "both k-mer registers are 32-bit");
  static_assert(kPPT == 8 && kHalo % kPPT == 0, "a thread's eight hashes are two 16-byte LDS accesses; a thread is all look-back or all its own");
  constexpr int kWords = (K + 7) / 8;
  // the first-multiply tables of MurmurHash3 (as kmer_hash.hip): low and high half of a group of eight characters
  __shared__ __attribute__((aligned(16))) unsigned char s_tab_raw[kWords * 256 * 12];
  uint64_t (*s_lo)[256] = reinterpret_cast<uint64_t (*)[256]>(s_tab_raw);
  uint32_t (*s_hi)[256] = reinterpret_cast<uint32_t (*)[256]>(s_tab_raw + kWords * 256 * 8);
  __shared__ __attribute__((aligned(16))) uint32_t s_h[kTile];    // the tile's hashes (kSkip: no k-mer, or both strands alike)
  __shared__ __attribute__((aligned(16))) uint32_t s_suf[kTile];  // position y: the minimum of y .. the end of its thread's group of eight
  __shared__ uint32_t s_scan[kMiniThreads / 64];
  __shared__ uint32_t s_tile, s_before;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    uint32_t t = 0xffffffffu;
    if (ticket_mode == 0u) {
      t = atomicAdd(&scalars[0], 1u);
    } else {
      // One counter per XCD (kTicketStride words apart: a line each), XCD x handing out the tiles x, x + 8, x + 16, ...: the
      // tiles are drawn at eight addresses instead of one (a returning atomic on ONE address is served every ~11 ns
      // chip-wide: 30 ms for the 2.6 million tiles of 1 000 x 5 Mb, under a kernel whose arithmetic takes less).  A workgroup
      // draws from its own XCD's counter and, once that has handed out its last tile, from the others' (as many
      // workgroups as tiles: it finds one).  Every counter hands its tiles out in order and the XCDs are dealt workgroups
      // at the same rate, so the lowest unfinished tile is always some running workgroup's; should a dispatch order ever
      // break that, the look-back's wait runs out, the flag is set and the host repeats the run with one counter.
      uint32_t xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t y = (xcc + i) & 7u;
        const uint32_t share = n_tiles > y ? (n_tiles - y + 7u) / 8u : 0u;
        if (share == 0u) continue;
        const uint32_t got = atomicAdd(&scalars[kTicketStride * (1u + y)], 1u);
        if (got < share) { t = got * 8u + y; break; }
      }
    }
    s_tile = t;
  }
  if (tid < 256u) {
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
      const uint64_t cj = (j & 1) ? kC2 : kC1;
      s_lo[j][tid] = (uint64_t)ascii_group(tid, K - 8 * j) * cj;
      s_hi[j][tid] = (uint32_t)((uint64_t)ascii_group(tid, K - 8 * j - 4) * cj);
    }
  }
  __syncthreads();
  const uint32_t tile = s_tile;
  if (tile == 0xffffffffu) return;  // (as many workgroups as tiles: does not happen)
  const int64_t tile0 = (int64_t)tile * kOwn - kHalo;
  const int64_t p0 = tile0 + (int64_t)tid * kPPT;  // (a multiple of eight)
  const bool in_arena = p0 >= 0 && (uint64_t)p0 < arena_bases;
  constexpr uint32_t kMask = (K == 16) ? 0xffffffffu : (uint32_t)((1ull << (2 * K)) - 1ull);

  // ---- both-strand hashes of the kPPT k-mers starting at p0 .. p0+kPPT-1: every one is hashed, without a branch; the
  // k-mers that hold a residue other than ACGT (or lie past the arena) are sorted out afterwards, by one bit each
  uint32_t own[kPPT];
  uint32_t unknowns = (1u << kPPT) - 1u;  // bit j: the k-mer at p0 + j holds a position that is no usable base
  {
    uint32_t lo = 0, hi = 0;
    if (in_arena) {
      const uint64_t wi = (uint64_t)p0 >> 4, mi = (uint64_t)p0 >> 5;
      const uint64_t nw = arena_bases >> 4, nm = arena_bases >> 5;
      const uint64_t w0 = packed[wi], w1 = wi + 1 < nw ? packed[wi + 1] : 0u;
      const uint64_t bases = ((w1 << 32) | w0) >> (2 * ((uint32_t)p0 & 15u));  // 24 or 32 residues: kPPT + K - 1 <= 23 are used
      lo = (uint32_t)bases;
      hi = (uint32_t)(bases >> 32);
      const uint64_t m0 = mask[mi], m1 = mi + 1 < nm ? mask[mi + 1] : 0xffffffffu;
      uint32_t bad = (uint32_t)(((m1 << 32) | m0) >> ((uint32_t)p0 & 31u));  // bit i: position p0 + i is no usable base (32 positions)
      // bit j of the OR over K consecutive bits from j on: eight by doubling, the rest by one more shift
      bad |= bad >> 1;
      bad |= bad >> 2;
      bad |= bad >> 4;
      if (K > 8) bad |= bad >> (K - 8);
      unknowns = bad & ((1u << kPPT) - 1u);
    }
    // the reverse complement of the first k-mer, LSB-first like the forward one: the 2-bit groups in reverse order, complemented
    uint32_t rc;
    {
      uint32_t r = __brev(lo & kMask);
      r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
      rc = (r >> (32 - 2 * K)) ^ kMask;
    }
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
      const uint32_t fl = alignbit(hi, lo, 2 * j) & kMask;  // residues j .. j+K-1, residue j in the lowest two bits
      if (j) rc = (((rc << 2) | (fl >> (2 * (K - 1)))) ^ 3u) & kMask;  // the new last residue, complemented, becomes the first
      const uint32_t strands[2] = {fl, rc};
      uint32_t hs[2];
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        uint64_t P[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < kWords; ++q) {
          const uint32_t glo = (strands[sidx] >> (16 * q)) & 0xffu, ghi = (strands[sidx] >> (16 * q + 8)) & 0xffu;
          const uint64_t tl = s_lo[q][glo];
          P[q] = u64_of((uint32_t)tl, (uint32_t)(tl >> 32) + s_hi[q][ghi]);
        }
        hs[sidx] = (uint32_t)murmur3_from_products<K>(P);
      }
      own[j] = hs[0] != hs[1] ? min(hs[0], hs[1]) : kSkip;
      if (kMiniHashGroup && j % (kMiniHashGroup ? kMiniHashGroup : 1) == (kMiniHashGroup ? kMiniHashGroup : 1) - 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
  uint32_t c = 0;
  bool have_c = false;
  // the contig of the thread's first position and its bounds, in registers: they change at a contig boundary only
  uint64_t c_beg = 0, c_next = ~0ULL;
  uint32_t c_len = 0;
  if (in_arena) {
    // from the contig of the tile's first position (tile_contig_kernel) on: the thread's own is that one or, rarely, a later one
    c = tile_contig[tile];
    c_next = c + 1 < n_contigs ? contig_start[c + 1] : ~0ULL;
    if (__builtin_expect((uint64_t)p0 >= c_next, 0)) {
      for (int step = 0; step < 4 && (uint64_t)p0 >= c_next; ++step) {
        ++c;
        c_next = c + 1 < n_contigs ? contig_start[c + 1] : ~0ULL;
      }
      if ((uint64_t)p0 >= c_next) {  // many short contigs inside one tile: the search
        c = contig_of(contig_start, n_contigs, (uint64_t)p0);
        c_next = c + 1 < n_contigs ? contig_start[c + 1] : ~0ULL;
      }
    }
    have_c = true;
    c_beg = contig_start[c];
    c_len = contig_len[c];
  }
  // Residues other than ACGT in a k-mer -- or the padding between contigs, marked the same way: a k-mer that starts in it
  // or runs into it is none; one that holds such a residue inside its contig is hashed as fastANI hashes it (the
  // characters as they are).  Few threads ever come here: the residues and mask words are asked for again (they are in
  // the cache) and the k-mer's contig is found by walking on from the thread's.
  if (__builtin_expect(unknowns != 0u, 0)) {
#pragma unroll
    for (int j = 0; j < kPPT; ++j)
      if ((unknowns >> j) & 1u) own[j] = kSkip;
    if (have_c) {
      constexpr uint64_t kBadMask = (1ULL << K) - 1;
      const uint64_t mi = (uint64_t)p0 >> 5, nm = arena_bases >> 5;
      const uint64_t m0 = mask[mi], m1 = mi + 1 < nm ? mask[mi + 1] : 0xffffffffu;
      const uint64_t bad = ((m1 << 32) | m0) >> ((uint32_t)p0 & 31u);  // (bits past the two words: never reached by 8 + 16 residues)
      const uint64_t wi = (uint64_t)p0 >> 4, nw = arena_bases >> 4;
      const uint64_t w0 = packed[wi], w1 = wi + 1 < nw ? packed[wi + 1] : 0u;
      const uint64_t bases = ((w1 << 32) | w0) >> (2 * ((uint32_t)p0 & 15u));
      uint64_t beg = c_beg, next = c_next;
      uint32_t cc = c, len = c_len;
#pragma unroll 1  // one copy of the code, the thread's positions one after the other
      for (uint32_t rest = unknowns; rest; rest &= rest - 1u) {
        const int j = __builtin_ctz(rest);
        const uint64_t pos = (uint64_t)(p0 + j);
        if (pos >= arena_bases) break;
        while (pos >= next) {  // into the next contig
          ++cc;
          beg = next;
          len = contig_len[cc];
          next = cc + 1 < n_contigs ? contig_start[cc + 1] : ~0ULL;
        }
        if (pos - beg + K > len) continue;
        const uint32_t h = hash_kmer_with_unknowns<K>((uint32_t)(bases >> (2 * j)) & kMask, (uint32_t)((bad >> j) & kBadMask), pos, amb);
#pragma unroll
        for (int q = 0; q < kPPT; ++q)
          if (q == j) own[q] = h;
      }
    }
  }
  // the hashes and the suffix minima of the thread's group of eight, 16 bytes at a time
  {
    uint32_t suf[kPPT];
    suf[kPPT - 1] = own[kPPT - 1];
#pragma unroll
    for (int j = kPPT - 2; j >= 0; --j) suf[j] = min(own[j], suf[j + 1]);
    uint4 *h4 = reinterpret_cast<uint4 *>(s_h + tid * kPPT), *s4 = reinterpret_cast<uint4 *>(s_suf + tid * kPPT);
    h4[0] = make_uint4(own[0], own[1], own[2], own[3]);
    h4[1] = make_uint4(own[4], own[5], own[6], own[7]);
    s4[0] = make_uint4(suf[0], suf[1], suf[2], suf[3]);
    s4[1] = make_uint4(suf[4], suf[5], suf[6], suf[7]);
  }
  __syncthreads();

  // ---- winnowing: the window that ends at x holds the positions x - w + 1 .. x, its minimizer is the RIGHTMOST of its
  // smallest hashes; a window is USED when it lies inside one contig and its last k-mer is one (own != kSkip), and a used
  // window records its minimizer when that is another k-mer than the minimizer of the used window before it (none within
  // the w - 1 positions before: always).  Positions of minima are never needed for that.  With `inner` the minimum of the
  // positions the window shares with the window one to the left (x - w + 1 .. x - 1), both used:
  //     the minimizer moves  <=>  own[x] <= inner  (the newcomer takes over, ties included: it is the rightmost)
  //                            or  hash[x - w] < inner  (the one that leaves was the minimizer, strictly: it was the leftmost).
  // inner = the own hashes before x in the thread's group (a running minimum in registers), the whole groups between (their
  // suffix minimum at the group's first position) and the suffix minimum at x - w + 1 in the group the window starts in:
  // for w = 24 two words per thread and two per position from LDS.  What does not fit -- the window before is not used
  // (after a run of N, at a contig's start), the thread's positions do not lie w deep inside one contig, w <= 8 -- takes
  // the plain form: the two minimizers found by going through their windows.
  auto window_minimizer = [&](int x, uint32_t &best) -> int {  // position of the minimizer of the window that ends at x, rightmost of equal ones
    best = s_h[x];
    int mp = x;
#pragma unroll 1
    for (int y = x - 1; y > x - w; --y) {
      const uint32_t hy = s_h[y];
      if (hy < best) { best = hy; mp = y; }
    }
    return mp;
  };
  // x: a used window, loc: its last position inside the contig.  Is its minimizer recorded?
  auto records_plain = [&](int x, uint32_t loc, uint32_t &best) -> bool {
    const int mp = window_minimizer(x, best);
#pragma unroll 1
    for (int y = x - 1; y > x - w; --y) {
      // the window that ends at y lies in the same contig as far as it is one at all: x's window does
      if (s_h[y] != kSkip && loc - (uint32_t)(x - y) + 1u >= (uint32_t)w) {
        uint32_t other;
        return window_minimizer(y, other) != mp;
      }
    }
    return true;
  };
  uint32_t flags = 0, cnt = 0;
  uint32_t besth[kPPT];
#pragma unroll
  for (int j = 0; j < kPPT; ++j) besth[j] = 0;
  const int x0 = (int)tid * kPPT;
  // every position of the thread, and the one before, at least w - 1 deep in the thread's contig and inside it
  const uint64_t loc0 = (uint64_t)p0 - c_beg;  // (garbage without a contig: have_c is asked first)
  const bool deep = have_c && w > kPPT && loc0 >= (uint64_t)w && loc0 + kPPT <= (uint64_t)c_len;
  if (x0 >= kHalo) {
    if (deep) {
      // whole groups between the window's first group and the thread's own: n_full for the positions j < j_switch, one
      // fewer from there on (uniform: w is)
      const int n_full = (w - 1 + 7) / 8 - 1, j_switch = (w - 1) % 8 == 0 ? kPPT : (w - 1) % 8;
      uint32_t c_all = 0xffffffffu, c_less = 0xffffffffu;  // minimum over the n_full groups before the thread's, over n_full - 1 of them
      for (int d = 1; d <= n_full; ++d) {
        c_less = c_all;
        c_all = min(c_all, s_suf[x0 - d * kPPT]);
      }
      uint32_t pre = 0xffffffffu;                 // the own hashes before position j
      uint32_t before = s_h[x0 - 1];              // the hash one position to the left
      uint32_t slow = 0;                          // bit j: a used window whose left neighbour is not
#pragma unroll
      for (int j = 0; j < kPPT; ++j) {
        const int x = x0 + j;
        const uint32_t inner = min(min(pre, j < j_switch ? c_all : c_less), s_suf[x - w + 1]);
        const uint32_t leaves = s_h[x - w];
        const uint32_t hx = own[j];
        besth[j] = min(inner, hx);
        const bool used = hx != kSkip, used_before = before != kSkip;
        const bool moves = (hx <= inner) | (leaves < inner);
        if (used & used_before & moves) { flags |= 1u << j; ++cnt; }
        if (used & !used_before) slow |= 1u << j;
        pre = min(pre, hx);
        before = hx;
      }
      if (__builtin_expect(slow != 0u, 0)) {
#pragma unroll 1
        for (uint32_t rest = slow; rest; rest &= rest - 1u) {
          const int j = __builtin_ctz(rest);
          uint32_t best;
          if (records_plain(x0 + j, (uint32_t)loc0 + (uint32_t)j, best)) { flags |= 1u << j; ++cnt; }
        }
      }
    } else if (have_c) {
      uint64_t beg = c_beg, next = c_next;
      uint32_t cc = c, len = c_len;
#pragma unroll 1
      for (int j = 0; j < kPPT; ++j) {
        const uint64_t pos = (uint64_t)(p0 + j);
        while (pos >= next) {  // into the next contig
          ++cc;
          beg = next;
          len = contig_len[cc];
          next = cc + 1 < n_contigs ? contig_start[cc + 1] : ~0ULL;
        }
        const uint64_t loc = pos - beg;
        if (loc < len && loc + 1 >= (uint64_t)w && s_h[x0 + j] != kSkip) {
          uint32_t best;
          const bool rec = records_plain(x0 + j, (uint32_t)loc, best);
#pragma unroll
          for (int q = 0; q < kPPT; ++q)
            if (q == j) besth[q] = best;
          if (rec) { flags |= 1u << j; ++cnt; }
        }
      }
    }
  }
  // block exclusive scan of cnt
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t wex = wave_excl_scan(cnt, lane);
  if (lane == 63) s_scan[wave] = wex + cnt;
  __syncthreads();
  uint32_t pre = 0, total = 0;
#pragma unroll
  for (int q = 0; q < kMiniThreads / 64; ++q) {
    if ((uint32_t)q < wave) pre += s_scan[q];
    total += s_scan[q];
  }
  // ---- minimizers of all tiles before this one
  if (wave == 0) {
    uint32_t before = 0;
    if (tile == 0) {
      if (lane == 0) __hip_atomic_store(&look[0], kLookTotal | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0) __hip_atomic_store(&look[tile], kLookTile | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int64_t at = (int64_t)tile - 1;  // lane l looks at tile at - l
      uint32_t spins = 0;
      for (;;) {
        const int64_t idx = at - (int64_t)lane;
        const uint64_t v = idx >= 0 ? __hip_atomic_load(&look[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kLookTotal;
        const uint32_t state = (uint32_t)(v >> 62);
        const uint64_t totals = __ballot(state == 2u), missing = __ballot(state == 0u);
        const uint32_t stop = totals ? (uint32_t)__builtin_ctzll(totals) : 64u;  // first lane holding a running total
        const uint64_t needed = stop >= 63u ? ~0ULL : ((2ULL << stop) - 1ULL);
        if (missing & needed) {  // a tile in front has not published yet
          if (++spins > kLookSpinLimit) { if (lane == 0) scalars[2] = 1u; break; }
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        before += wave_sum(lane <= stop ? (uint32_t)v : 0u);
        if (stop < 64u) break;
        at -= 64;
      }
      if (lane == 0)
        __hip_atomic_store(&look[tile], kLookTotal | (uint64_t)(before + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
      s_before = before;
      if (tile == n_tiles - 1) scalars[1] = before + total;
    }
  }
  __syncthreads();
  uint32_t o = s_before + pre + wex;
  if (flags) {
    // where the recorded windows end inside their contigs: the thread's contig, or -- at a contig boundary -- the ones after it
    uint64_t beg = c_beg, next = c_next;
    uint32_t cc = c;
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
      if (!((flags >> j) & 1u)) continue;
      const uint64_t pos = (uint64_t)(p0 + j);
      if (!deep) {
        while (pos >= next) {
          ++cc;
          beg = next;
          next = cc + 1 < n_contigs ? contig_start[cc + 1] : ~0ULL;
        }
      }
      if (o < cap) {  // a run that overflows the estimate is repeated with the exact size
        out_hash[o] = besth[j];
        out_wpos[o] = (uint32_t)(pos - beg) - (uint32_t)w + 1u;
        out_contig[o] = cc;
      }
      ++o;
    }
  }
}

__global__ __launch_bounds__(kThreads) void contig_offsets_kernel(const uint32_t *__restrict__ mini_contig, uint32_t m,
                                                                   uint32_t n_contigs, uint32_t *__restrict__ off) {
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c <= n_contigs) off[c] = lower_bound_u32(mini_contig, 0, m, c);
}

// bucket_first[base_c + b] = first minimizer of contig c with window id >= b*256, b = 0 .. n_buckets_c
__global__ __launch_bounds__(kThreads) void bucket_index_kernel(const uint32_t *__restrict__ mini_wpos,
                                                                const uint32_t *__restrict__ contig_mini_off,
                                                                const uint32_t *__restrict__ contig_bucket_off,
                                                                uint32_t n_contigs, uint32_t total_entries,
                                                                uint32_t *__restrict__ bucket_first) {
  const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= total_entries) return;
  uint32_t lo = 0, hi = n_contigs;  // contig owning entry e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (contig_bucket_off[mid] <= e) lo = mid; else hi = mid;
  }
  const uint32_t c = lo, b = e - contig_bucket_off[c];
  bucket_first[e] = lower_bound_u32(mini_wpos, contig_mini_off[c], contig_mini_off[c + 1], b << kBucketShift);
}

// ============================================================== 2. dictionary of minimizer hashes
// Sort key of a minimizer: its hash in the low word -- the only bits the radix passes look at -- and its window id as a
// passenger in the high word, so that the posting build reads it in posting order instead of gathering it.
// (`base`: the first minimizer the dictionary holds -- those of the reference genomes asked for; values = minimizer indices)
__global__ __launch_bounds__(kThreads) void mini_keys_kernel(const uint32_t *__restrict__ hash, const uint32_t *__restrict__ wpos,
                                                             uint32_t base, uint32_t m, uint64_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < m) { keys[i] = ((uint64_t)wpos[base + i] << 32) | hash[base + i]; vals[i] = base + i; }
}
// Where the dictionary holds the reference range's minimizers only, a query minimizer finds its hash by value: an open
// table of {hash, first posting, postings | mark of the frequency cut << 31, -} entries, 16 bytes each, at least two slots
// per hash, linear probing -- one load per look-up where a search through the sorted hashes and the list bounds were eight
// (19 ms per batch against 1 for 125 of 1 000 genomes).  The slot comes from the hash multiplied by the golden-ratio
// constant: a minimizer's hash is the MINIMUM of a window of hashes, and minima crowd at the low end -- slotted by their top
// bits they filled the table's first tenth and every probe walked through it (28 s for twenty genomes).
__device__ __forceinline__ uint32_t lookup_slot(uint32_t h, uint32_t table_bits) { return (h * 0x9e3779b1u) >> (32u - table_bits); }
__global__ __launch_bounds__(kThreads) void lookup_insert_kernel(const uint32_t *__restrict__ uniq_hash,
                                                                 const uint32_t *__restrict__ post_start,
                                                                 const uint32_t *__restrict__ hash_cut, uint32_t n_ids,
                                                                 uint32_t table_bits, uint4 *__restrict__ table) {
  const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
  if (id >= n_ids) return;
  const uint32_t h = uniq_hash[id], lo = post_start[id], cnt = post_start[id + 1] - lo;
  const uint32_t mark = (hash_cut[id >> 5] >> (id & 31u)) & 1u;
  const uint32_t mask = (1u << table_bits) - 1u;
  unsigned long long *words = reinterpret_cast<unsigned long long *>(table);
  for (uint32_t slot = lookup_slot(h, table_bits);; slot = (slot + 1u) & mask) {
    if (atomicCAS(&words[2ull * slot], ~0ULL, ((unsigned long long)lo << 32) | h) == ~0ULL) {
      table[slot].z = cnt | (mark << 31);
      return;
    }
  }
}
// the contig of the first minimizer of every block of 2^kContigBlockShift minimizers (the minimizers are stored contig by contig)
constexpr uint32_t kContigBlockShift = 10;
__global__ __launch_bounds__(kThreads) void block_contig_kernel(const uint32_t *__restrict__ mini_contig, uint32_t m,
                                                                 uint32_t *__restrict__ block_contig) {
  const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
  if (((uint64_t)b << kContigBlockShift) < m) block_contig[b] = mini_contig[(uint64_t)b << kContigBlockShift];
}
__global__ __launch_bounds__(kThreads) void key_heads_kernel(const uint64_t *__restrict__ keys, uint32_t m,
                                                             uint32_t *__restrict__ flags) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < m) flags[i] = (i == 0 || (uint32_t)keys[i] != (uint32_t)keys[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(kThreads) void postings_kernel(const uint64_t *__restrict__ keys,
                                                            const uint32_t *__restrict__ sorted_idx,
                                                            const uint32_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ pos, uint32_t m, uint32_t n_ids,
                                                            const uint32_t *__restrict__ mini_contig,
                                                            uint32_t *__restrict__ mini_id, uint32_t *__restrict__ post_start,
                                                            int32_t *__restrict__ prev_same,
                                                            const uint32_t *__restrict__ mini_wpos,
                                                            const uint32_t *__restrict__ contig_genome,
                                                            uint64_t *__restrict__ post_cw,
                                                            uint16_t *__restrict__ post_genome,
                                                            const uint32_t *__restrict__ contig_mini_off, uint32_t n_contigs,
                                                            uint32_t *__restrict__ uniq_hash, const uint32_t *__restrict__ block_contig) {
  // the contig of the posting before this one comes from the thread before it (LDS) instead of a second random read
  __shared__ uint32_t s_contig[kThreads];
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool in = i < m;
  uint32_t id = 0, me = 0, mc = 0;
  if (in) {
    id = pos[i] + flags[i] - 1u;
    me = sorted_idx[i];
    // the minimizers are stored contig by contig: the contig of minimizer `me` comes from the contig of its block of 1 024
    // minimizers (block_contig_kernel: a table of 1.5 MB, in the L2) and a step or two through the contigs' first minimizers
    // (a few KB, in the L1) -- two dependent loads where a search through the contigs' first minimizers was ten, and no random
    // 4-byte read from the 1.6 GB of mini_contig
    uint32_t cc = block_contig[me >> kContigBlockShift];
    while (cc + 1u < n_contigs && contig_mini_off[cc + 1u] <= me) ++cc;
    mc = cc;
  }
  s_contig[threadIdx.x] = mc;
  __syncthreads();
  if (!in) return;
  mini_id[me] = id;
  // the posting as the low 44 bits of a hit key, its genome on top so that bucketing needs no second lookup
  const uint32_t pg = contig_genome[mc];
  const uint64_t key = keys[i];
  post_cw[i] = posting_of(pg, place_of(mc, (uint32_t)(key >> 32)));  // the window id rode along in the sort key
  post_genome[i] = (uint16_t)pg;  // (the bucketed seeding and the frequency cut read this; at most 65 535 genomes)
  if (flags[i]) { post_start[id] = i; uniq_hash[id] = (uint32_t)key; }
  if (i == m - 1) post_start[n_ids] = m;
  // "the same hash earlier in this contig": rare (repeats inside a contig), and the array has been filled with -1
  if (i > 0 && (uint32_t)key == (uint32_t)keys[i - 1]) {
    const uint32_t other = sorted_idx[i - 1];  // stable sort: other < me
    const uint32_t oc = threadIdx.x > 0 ? s_contig[threadIdx.x - 1] : mini_contig[other];
    if (oc == mc) prev_same[me] = (int32_t)other;
  }
}

// ---- Mashmap's frequency cut of the seed look-up (fastANI logs it: "ignore minimizers occurring >= N times during
// lookup").  The reference sketch of a fastANI process is ONE genome; the minimizers it holds are counted per hash, and
// the most frequent ones -- as many bars of the histogram of counts, from the top, as stay within 0.001 % of the distinct
// minimizers -- give no seed hits.  Here the postings of a hash are ordered by arena position, so the occurrences of a
// hash in one genome are a RUN of its list: a run of c >= 2 is counted into its genome's histogram (c >= kFreqBins - 1:
// listed exactly instead), the host walks the histograms (a few KB per genome), and the runs at or above their genome's
// threshold are taken out of the posting lists -- everything after the index sees lists that never held them.  The
// minimizers themselves stay where they are: the L2 windows hold every minimizer, as fastANI's do.
constexpr uint32_t kFreqBins = 256;
// The runs are numbered first -- a flag at every run's first posting, their prefix sums, the runs' first postings
// gathered by number -- so that a run's length is a difference of two entries, whoever asks: one thread per POSTING
// everywhere below.  (A thread walking its run cost the run's length in dependent loads, twice per index build: a
// homopolymer or an array of a short unit in a reference is one minimizer per position with one hash, runs of 10^5-10^6
// postings on one lane while the grid idled.)
__global__ __launch_bounds__(kThreads) void posting_run_flags_kernel(const uint32_t *__restrict__ heads,
                                                                     const uint16_t *__restrict__ post_genome, uint32_t m,
                                                                     uint32_t *__restrict__ run_flag) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < m) run_flag[i] = (i == 0 || heads[i] || post_genome[i - 1] != post_genome[i]) ? 1u : 0u;
}
__global__ __launch_bounds__(kThreads) void posting_run_starts_kernel(const uint32_t *__restrict__ run_flag,
                                                                      const uint32_t *__restrict__ runs_before, uint32_t m,
                                                                      uint32_t *__restrict__ run_start) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  if (run_flag[i]) run_start[runs_before[i]] = i;
  if (i == m - 1) run_start[runs_before[i] + run_flag[i]] = m;  // the closing entry
}
__global__ __launch_bounds__(kThreads) void posting_run_hist_kernel(const uint32_t *__restrict__ run_flag,
                                                                    const uint32_t *__restrict__ runs_before,
                                                                    const uint32_t *__restrict__ run_start,
                                                                    const uint16_t *__restrict__ post_genome, uint32_t m,
                                                                    uint32_t *__restrict__ hist /* [genomes][kFreqBins] */,
                                                                    uint32_t *__restrict__ dups /* [genomes] */,
                                                                    uint2 *__restrict__ over, uint32_t over_cap,
                                                                    uint32_t *__restrict__ over_n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m || !run_flag[i]) return;  // a run's first posting speaks for the run
  const uint32_t c = run_start[runs_before[i] + 1u] - i;
  if (c < 2u) return;  // a run of one: the common case, counted by difference
  const uint16_t g = post_genome[i];
  atomicAdd(&dups[g], c - 1u);
  if (c < kFreqBins - 1u) {
    atomicAdd(&hist[(uint64_t)g * kFreqBins + c], 1u);
  } else {
    atomicAdd(&hist[(uint64_t)g * kFreqBins + kFreqBins - 1u], 1u);
    const uint32_t at = atomicAdd(over_n, 1u);
    if (at < over_cap) over[at] = make_uint2(g, c);
  }
}
// keep[i] = 0 for the postings of runs at or above their genome's threshold, 1 for the others.  `keep` is the memory of
// the run flags: a thread reads its own flag before it writes its own entry.
__global__ __launch_bounds__(kThreads) void posting_cut_flags_kernel(const uint32_t *__restrict__ heads,
                                                                     const uint32_t *__restrict__ ids_before,
                                                                     const uint32_t *__restrict__ runs_before,
                                                                     const uint32_t *__restrict__ run_start,
                                                                     const uint16_t *__restrict__ post_genome, uint32_t m,
                                                                     const uint32_t *__restrict__ threshold,
                                                                     uint32_t *__restrict__ keep /* in: run flags */,
                                                                     uint32_t *__restrict__ hash_cut) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t first = keep[i];  // the run flag
  const uint32_t run = runs_before[i] + first - 1u;
  const uint32_t c = run_start[run + 1u] - run_start[run];
  const uint32_t thr = threshold[post_genome[i]];
  const bool cut = thr != 0xffffffffu && c >= thr;
  keep[i] = cut ? 0u : 1u;
  if (cut && first) {
    // the hash has lost seed hits somewhere: its matches in an L2 window are no longer all among the seed hits (the mapping
    // kernel's bounds allow for them).  A bit per hash (dense id: the hashes before this posting's own, plus one where it
    // is its hash's first) says so; mark_cut_minimizers_kernel hands it on to the minimizers.
    const uint32_t id = ids_before[i] + heads[i] - 1u;
    atomicOr(&hash_cut[id >> 5], 1u << (id & 31u));
  }
}
// Every minimizer whose hash lost seed hits -- in whatever genome: it is the QUERY's minimizers that are asked -- carries
// the mark in the top bit of its hash id, which the sketch kernel reads anyway.  One thread per posting.
__global__ __launch_bounds__(kThreads) void mark_cut_minimizers_kernel(const uint32_t *__restrict__ heads,
                                                                       const uint32_t *__restrict__ ids_before,
                                                                       const uint32_t *__restrict__ sorted_idx, uint32_t m,
                                                                       const uint32_t *__restrict__ hash_cut,
                                                                       uint32_t *__restrict__ mini_id) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const uint32_t id = ids_before[i] + heads[i] - 1u;
  if ((hash_cut[id >> 5] >> (id & 31u)) & 1u) mini_id[sorted_idx[i]] |= 0x80000000u;
}
__global__ __launch_bounds__(kThreads) void posting_compact_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ at,
                                                                   const uint64_t *__restrict__ post_cw,
                                                                   const uint16_t *__restrict__ post_genome,
                                                                   const uint32_t *__restrict__ sorted_idx, uint32_t m,
                                                                   uint64_t *__restrict__ cw_out, uint16_t *__restrict__ g_out,
                                                                   uint32_t *__restrict__ idx_out) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < m && keep[i]) { cw_out[at[i]] = post_cw[i]; g_out[at[i]] = post_genome[i]; idx_out[at[i]] = sorted_idx[i]; }
}
__global__ __launch_bounds__(kThreads) void posting_starts_kernel(uint32_t *__restrict__ post_start, uint32_t n_ids,
                                                                  const uint32_t *__restrict__ at, uint32_t m, uint32_t kept) {
  const uint32_t id = blockIdx.x * kThreads + threadIdx.x;
  if (id > n_ids) return;
  const uint32_t old = post_start[id];
  post_start[id] = old < m ? at[old] : kept;
}

// Keys ordered in registers (a segment's hits by (contig, window id) in the mapping kernel, a fragment's minimizers by
// hash below): E keys per lane, element e = lane * E + q, bitonic network over 64 E elements.  Strides of E and more exchange between lanes (ds_bpermute, no LDS memory, no barrier),
// the strides below E between the registers of a lane.  Missing elements are keys above any real one.  Key = uint32_t
// (contig relative to the genome's first in 8 bits | window id in 24) when the segment's contigs allow it -- one
// shuffle, a minimum, a maximum and a select per key and stage --, else uint64_t (20 + 24 bits).
template <typename Key>
__device__ __forceinline__ Key lane_exchange(Key v, int partner_byte_address) {
  if constexpr (sizeof(Key) == 4) {
    return (Key)__builtin_amdgcn_ds_bpermute(partner_byte_address, (int)v);
  } else {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(partner_byte_address, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(partner_byte_address, (int)(uint32_t)(v >> 32));
    return ((Key)hi << 32) | lo;
  }
}
template <int E, int J, typename Key>
__device__ __forceinline__ void bitonic_inside_lane(Key (&k)[E], uint32_t e0, uint32_t span) {
#pragma unroll
  for (int q = 0; q < E; ++q) {
    if ((q & J) == 0) {
      const bool asc = ((e0 + (uint32_t)q) & span) == 0u;
      const Key a = k[q], b = k[q | J];
      const Key lo = a < b ? a : b, hi = a < b ? b : a;
      k[q] = asc ? lo : hi;
      k[q | J] = asc ? hi : lo;
    }
  }
}
template <int E, typename Key>
__device__ __forceinline__ void bitonic_sort_lanes(Key (&k)[E], uint32_t lane) {
  const uint32_t e0 = lane * (uint32_t)E;
  for (uint32_t span = 2; span <= 64u * (uint32_t)E; span <<= 1) {
    for (uint32_t j = span >> 1; j > 0; j >>= 1) {
      if (j >= (uint32_t)E) {
        const uint32_t lj = j / (uint32_t)E;
        const int partner = (int)((lane ^ lj) << 2);  // byte address of the partner lane for ds_bpermute
        // the lower lane of a pair keeps the smaller key in an ascending run: span > j >= E, so the run's direction is a
        // bit of the lane number, the same for all E keys of the lane
        const bool take_min = ((lane & lj) == 0u) == ((lane & (span / (uint32_t)E)) == 0u);
#pragma unroll
        for (int q = 0; q < E; ++q) {
          const Key other = lane_exchange<Key>(k[q], partner);
          if constexpr (sizeof(Key) == 4) {
            const Key lo = min(k[q], other), hi = max(k[q], other);
            k[q] = take_min ? lo : hi;
          } else {
            k[q] = ((other < k[q]) == take_min) ? other : k[q];
          }
        }
      } else if (E > 4 && j == 4u) {
        bitonic_inside_lane<E, (E > 4 ? 4 : 1), Key>(k, e0, span);
      } else if (E > 2 && j == 2u) {
        bitonic_inside_lane<E, (E > 2 ? 2 : 1), Key>(k, e0, span);
      } else if (E > 1) {
        bitonic_inside_lane<E, 1, Key>(k, e0, span);
      }
    }
  }
}
