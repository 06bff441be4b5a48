// pa_internal.h -- shared internals of libpyani_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pyani_hip.h"
#include "pa_carve.h"
#include "pa_launch_geom.h"

// ---- error plumbing -------------------------------------------------------
void pa_set_error(const char *fmt, ...);

#define PA_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t _e = (call);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      pa_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
      return PA_E_HIP;                                                                        \
    }                                                                                         \
  } while (0)

#define PA_TRY(call)          \
  do {                        \
    int _s = (call);          \
    if (_s != PA_OK) return _s; \
  } while (0)

#define PA_REQUIRE(cond, ...)   \
  do {                          \
    if (!(cond)) {              \
      pa_set_error(__VA_ARGS__); \
      return PA_E_INVALID;      \
    }                           \
  } while (0)

// ---- switches for tools and tests ------------------------------------------
// Environment variables that force a rare path, cut a kernel short or select an ablation variant exist in
// libpyani_hip_tools.so only (built with -DPA_TOOLS from the same sources; tools/ and the tests of the rare paths load
// it).  In the product library the look-up is a null constant: the names are not even in the binary, and a stray variable
// in a worker's environment cannot change a result.
#ifdef PA_TOOLS
#include <cstdlib>
#define PA_TOOL_ENV(name) getenv(name)
#else
#define PA_TOOL_ENV(name) static_cast<const char *>(nullptr)
#endif

// ---- growable device buffer owned by the context ---------------------------
// A group of buffers may share a budget: bytes held, the most ever held, and an optional cap (0: none) past which a
// buffer refuses to grow -- with a message that names the sizes -- instead of asking the driver (fragani.hip).
struct DevBudget {
  uint64_t held = 0, peak = 0, cap = 0;
  char what[192] = {0};  // the call the buffers are growing for, for the message
};
struct DevBuf {
  void *p = nullptr;
  uint64_t bytes = 0;
  DevBudget *budget = nullptr;
  int reserve(uint64_t want) {
    if (want <= bytes) return PA_OK;
    // grow geometrically so steady-state calls never allocate
    uint64_t sz = want + want / 4 + 256;
    if (budget && budget->cap && budget->held - bytes + sz > budget->cap) {
      pa_set_error("%s: the workspace would grow to %llu bytes (%llu held; this buffer from %llu to %llu), above the cap of %llu bytes",
                   budget->what[0] ? budget->what : "device workspace", (unsigned long long)(budget->held - bytes + sz),
                   (unsigned long long)budget->held, (unsigned long long)bytes, (unsigned long long)sz, (unsigned long long)budget->cap);
      return PA_E_NOMEM;
    }
    if (p) (void)hipFree(p);
    if (budget) budget->held -= bytes;
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, sz);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // the failure is reported here: the next launch's hipGetLastError must not see it again
      if (budget)
        pa_set_error("%s: hipMalloc(%llu) failed with %llu bytes of workspace held: %s", budget->what[0] ? budget->what : "device workspace",
                     (unsigned long long)sz, (unsigned long long)budget->held, hipGetErrorString(e));
      else
        pa_set_error("hipMalloc(%llu) failed: %s", (unsigned long long)sz, hipGetErrorString(e));
      p = nullptr;
      return PA_E_NOMEM;
    }
    bytes = sz;
    if (budget) {
      budget->held += sz;
      if (budget->held > budget->peak) budget->peak = budget->held;
    }
    return PA_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    if (budget) budget->held -= bytes;
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

// A workspace of several arrays (pa_carve.h): `layout` states the parts once, as take()s on a Carve that assign the caller's pointers.  It runs
// twice: to measure, then on buf.p after reserve(the measured bytes).  A size past 64 bits, a part off its alignment or passes that differ: PA_E_INVALID.
template <class Layout>
int pa_carve(DevBuf &buf, const char *name, Layout &&layout) {
  uint64_t bytes = 0;
  CarveVerdict v = carve_measure(layout, &bytes);
  if (v == CarveVerdict::kOk) PA_TRY(buf.reserve(bytes));
  if (v == CarveVerdict::kOk) v = carve_place(buf.p, bytes, layout);
  PA_REQUIRE(v == CarveVerdict::kOk, "workspace %s, %llu bytes: %s", name, (unsigned long long)bytes, carve_verdict_text(v));
  return PA_OK;
}

struct ProfPhase {
  double total_ms = 0.0;
  uint64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// ---- device scalars ---------------------------------------------------------
// A block of device scalars -- the counters and cursors that kernels are handed -- is divided into named slots:
// (first 32-bit word, words).  A hipMemsetAsync or a read-back stays inside one slot (none covers two).  A block's
// owner lists the slots that are live together in one static_assert(slots_apart(bytes, {...})).
struct ScalarSlot {
  uint32_t word, words;
  constexpr uint32_t bytes() const { return words * 4u; }
  constexpr bool apart_from(ScalarSlot o) const { return word + words <= o.word || o.word + o.words <= word; }
};
// Every slot inside the block's `region_bytes`, slots of whole 64-bit words on an even word, no two overlapping.
constexpr bool slots_apart(uint32_t region_bytes, std::initializer_list<ScalarSlot> slots) {
  for (const ScalarSlot *a = slots.begin(); a != slots.end(); ++a) {
    if ((a->word + a->words) * 4u > region_bytes || (a->words % 2 == 0 && a->word % 2)) return false;
    for (const ScalarSlot *b = a + 1; b != slots.end(); ++b)
      if (!a->apart_from(*b)) return false;
  }
  return true;
}

// The words of pa_ctx::counters (pa_ctx::slot).  A new feature that needs a device scalar adds its slot here.
constexpr uint32_t kCtxScalarBytes = 192;      // what pa_ctx_create reserves
constexpr ScalarSlot kCandCount{0, 2};         // pa_sketch, general path: candidates of the k-mer hash kernel, 64-bit; zeroed and read per attempt
constexpr ScalarSlot kSketchTotal{2, 2};       // pa_build_sketch_csr, pa_sketch_from_regions, pa_sketch_bottom: the 64-bit total of their scan (written, never zeroed)
constexpr ScalarSlot kDenseIds{4, 4};          // pa_dense_ids_sorted, two 64-bit words zeroed as one: [0] OR of the keys, [1] distinct keys (its scan's total)
constexpr uint32_t kDenseOr = 0, kDenseDistinct = 1;  // 64-bit words within kDenseIds
constexpr ScalarSlot kCompactTotal{8, 2};      // pa_classify_edges, pa_runcomp_join: the 64-bit total of their scan (written, never zeroed)
constexpr ScalarSlot kRegionOverflow{12, 1};   // pa_sketch, pa_sketch_streamed: a region was too small; zeroed there, read by pa_sketch_from_regions
constexpr ScalarSlot kNjPick{16, 8};           // pa_nj: the pair a join chose, written by its join kernel and read by its update kernel (NjPick, nj.hip)
constexpr ScalarSlot kDistBad{24, 8};          // pa_check_distance_matrices (pa_nj, pa_gower_center, pa_mantel): per matrix, of up to two, two 64-bit words: [0] cells that break the rule, [1] the first of them
constexpr ScalarSlot kDerepProgress{14, 2};    // pa_derep_select: [0] nodes settled, [1] rounds that had work; zeroed as one, read once per batch of rounds
constexpr ScalarSlot kSubstUndefined{32, 16};  // pa_subst_distances: per matrix, of up to four a launch, two 64-bit words: the pairs without a shared nucleotide column, the saturated pairs; zeroed and read per launch
static_assert(slots_apart(kCtxScalarBytes, {kCandCount, kSketchTotal, kDenseIds, kCompactTotal, kRegionOverflow, kNjPick, kDistBad, kDerepProgress, kSubstUndefined}),
              "two slots of pa_ctx::counters overlap or leave the block");

// The words of pa_ctx::dict_scalars (pa_ctx::dict_slot), the hash dictionary's own block, touched by no other phase
constexpr uint32_t kDictScalarBytes = 64;  // what dict_insert and pa_pairs_bitrow_hash reserve
constexpr ScalarSlot kDictCounters{0, 2};  // dict_insert: [0] id counter (zeroed), [1] id of the key ~0 (set to ~0); read by pa_pairs_bitrow_hash
constexpr uint32_t kDictIdCounter = 0, kDictSpecialId = 1;  // 32-bit words within kDictCounters
constexpr ScalarSlot kDictPreparedFp{2, 4};  // pa_pair_dict_prepare_impl: 128-bit fingerprint of the postings a prepared dictionary was built from
constexpr ScalarSlot kDictTileFp{6, 4};      // pa_pairs_bitrow_hash: the same of the tile that consumes it; zeroed there, read with the one above
static_assert(slots_apart(kDictScalarBytes, {kDictCounters, kDictPreparedFp, kDictTileFp}),
              "two slots of pa_ctx::dict_scalars overlap or leave the block");

constexpr uint32_t kPinnedBytes = 64;  // pa_ctx::h_pinned, the landing place of ReadBack

// The device buffers of the context, each named here and nowhere else: the members of pa_ctx and their release in
// pa_ctx_destroy follow from this list.  ONE(name): a buffer `name`; PAIR(name): two, `name[0]` and `name[1]`.
//   sketch phase: cand_keys / cand_vals, the double-buffered radix sort storage; genome_blk, genome start block index
//   (u32[n+1]); counters, the small device scalars above; hist, the radix sort's histograms and the scratch of pa_minmax_f64,
//   pa_moments_f64, pa_select_f64, pa_kde_gauss_f64 and the uniform histograms (hist.hip); flags, compaction; scan_tmp, the scan's
//   tile sums and the runs of pa_mask_from_runs; region_off and region_cursor, per-genome candidate regions (LDS-sort path);
//   dirty, the dirty-block bitmap for callers that pass none.  A sort reserves hist and, through its scans, scan_tmp, and a
//   reserve may move the buffer: those users of hist hold no pointer into it across a sort (none sorts or scans; pa_kde_gauss_f64
//   cuts hist after its own pa_minmax_f64 is done), nor pa_mask_from_runs one into scan_tmp across a sort or a scan
//   pair phase: dict_keys / dict_vals, ids, post_genome, bitrows; dict_scalars, the hash dictionary's scalars above
//   classify (classify.hip): cls_i, cls_j, cls_score, cls_cov, the edges in (i, j) order, before the sort
//   plot-run's scatter figures (scatter.hip): bin2d, the two edge arrays, then the cells' counts and last indices
//   TETRA-hip (tetra.hip): tetra_tab, the genomes' first blocks and first chunks (u32[2 (n + 1)])
//   tree-run (nj.hip): nj_work, the row sums, the slots' node ids, the scan's candidates and the join table
//   ordinate-run (pcoa.hip): pcoa_work, the thin blocks Q and Y, the chunks' partial sums, the centring's row sums
//   mantel-run-comp (mantel.hip): mantel_work, the moments, the cross sums, a batch's permutations,
//   inverses and row sums
//   dereplicate-run (derep.hip): derep_work, the nodes still open as bits, then a round's new representatives or candidates
//   bootstrap-run (msa_boot.hip) and phylo-run (subst.hip): boot_work, a launch's weights as bytes and as bit planes (msa_boot_dev.h)
#define PA_CTX_BUFFERS(ONE, PAIR)                                                                                   \
  PAIR(cand_keys) PAIR(cand_vals) ONE(genome_blk) ONE(counters) ONE(hist) ONE(flags) ONE(scan_tmp) ONE(region_off) \
  ONE(region_cursor) ONE(dirty) PAIR(dict_keys) PAIR(dict_vals) ONE(ids) ONE(post_genome) ONE(bitrows)             \
  ONE(dict_scalars) ONE(cls_i) ONE(cls_j) ONE(cls_score) ONE(cls_cov) ONE(bin2d) ONE(tetra_tab) ONE(nj_work) ONE(pcoa_work) \
  ONE(mantel_work) ONE(derep_work) ONE(boot_work)

struct pa_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipDeviceProp_t prop;
#define PA_ONE(name) DevBuf name;
#define PA_PAIR(name) DevBuf name[2];
  PA_CTX_BUFFERS(PA_ONE, PA_PAIR)
#undef PA_ONE
#undef PA_PAIR
  template <class Fn>
  void each_buffer(Fn &&fn) {
#define PA_ONE(name) fn(name);
#define PA_PAIR(name) fn(name[0]); fn(name[1]);
    PA_CTX_BUFFERS(PA_ONE, PA_PAIR)
#undef PA_ONE
#undef PA_PAIR
  }
  template <typename T = uint32_t>
  T *slot(ScalarSlot s) const { return reinterpret_cast<T *>(counters.as<uint32_t>() + s.word); }
  template <typename T = uint32_t>
  T *dict_slot(ScalarSlot s) const { return reinterpret_cast<T *>(dict_scalars.as<uint32_t>() + s.word); }
  // dictionary built ahead of the pair phase by pa_pair_dict_prepare (multi-GPU overlap)
  bool dict_prepared = false;
  uint64_t dict_prepared_postings = 0;
  uint32_t dict_prepared_cap = 0;
  hipStream_t copy_stream = nullptr;  // uploads of pa_sketch_streamed, created on first use
  void *frag_work = nullptr;  // fragment-ANI workspace (fragani.hip), created on first use
  // pinned host scalars (kPinnedBytes), written and read through ReadBack only
  uint64_t *h_pinned = nullptr;
  // profiling
  bool prof_on = false;
  ProfPhase prof[PA_PROF_NPHASES];
  std::vector<hipEvent_t> event_pool;
};

// ---- reading device scalars back ---------------------------------------------
// Copies of a few typed values from the device to the host through the context's pinned block, with one wait on the
// context's stream: queue() once per value (or array of `count` values), host work that may overlap the stream, then
// wait(), which fills the callers' variables.  Each copy gets a place of its own in the block and is checked against
// kPinnedBytes; what is copied is exactly what *out receives, so no read is wider than its copy.
class ReadBack {
 public:
  explicit ReadBack(pa_ctx *c) : c_(c) {}
  template <typename T>
  int queue(const T *d_src, T *out, uint32_t count = 1) {
    static_assert(std::is_trivially_copyable<T>::value && alignof(T) <= 8, "ReadBack copies plain scalars");
    const uint64_t bytes = (uint64_t)count * sizeof(T);
    PA_REQUIRE(n_ < kMaxItems && used_ + bytes <= kPinnedBytes, "read-back of %llu bytes behind %u in %u copies exceeds the pinned block of %u bytes",
               (unsigned long long)bytes, used_, n_, kPinnedBytes);
    PA_HIP(hipMemcpyAsync(reinterpret_cast<char *>(c_->h_pinned) + used_, d_src, bytes, hipMemcpyDeviceToHost, c_->stream));
    items_[n_++] = Item{out, used_, (uint32_t)bytes};
    used_ = (used_ + (uint32_t)bytes + 7u) & ~7u;  // the next copy on a 64-bit boundary
    return PA_OK;
  }
  int wait() {
    PA_HIP(hipStreamSynchronize(c_->stream));
    for (uint32_t i = 0; i < n_; ++i) memcpy(items_[i].out, reinterpret_cast<const char *>(c_->h_pinned) + items_[i].at, items_[i].bytes);
    n_ = used_ = 0;
    return PA_OK;
  }

 private:
  static constexpr uint32_t kMaxItems = 4;
  struct Item {
    void *out;
    uint32_t at, bytes;
  };
  pa_ctx *c_;
  Item items_[kMaxItems];
  uint32_t n_ = 0, used_ = 0;
};
// One value (or array): the copy, the wait on c->stream, *out filled.
template <typename T>
int pa_read_back(pa_ctx *c, const T *d_src, T *out, uint32_t count = 1) {
  ReadBack rb(c);
  PA_TRY(rb.queue(d_src, out, count));
  return rb.wait();
}

// RAII-ish phase timer: records events around a group of launches when enabled.
struct ProfScope {
  pa_ctx *c;
  int phase;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ProfScope(pa_ctx *ctx, int ph);
  ~ProfScope();
};

// Bulk copy to the host on the context's stream, and the wait for it.
inline int pa_copy_to_host(pa_ctx *c, void *h_dst, const void *d_src, size_t bytes) {
  PA_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}

// ---- kernel launches ---------------------------------------------------------
// Every kernel is launched through PA_LAUNCH (on the context's stream), PA_LAUNCH_ON (on a stream of the caller's;
// nullptr: the context's) or PA_LAUNCH_RAISE_LDS (the kernel's dynamic LDS limit is raised to this launch's bytes
// first).  grid and block are LaunchDim: a 64-bit count for the 1-D form, LaunchDim(x, y) otherwise.  An empty grid
// launches nothing and is PA_OK; a grid or block beyond the device's limits is PA_E_INVALID; what the runtime refuses
// is PA_E_HIP, reported at once with the kernel's name and sizes.  The launcher keeps no state.
inline int pa_launch_refused(const char *name, LaunchDim g, LaunchDim b, size_t lds_bytes, const char *why, int status) {
  pa_set_error("launch of %s, grid (%llu, %llu, %llu), block (%llu, %llu, %llu), %zu bytes of dynamic LDS: %s", name, (unsigned long long)g.x,
               (unsigned long long)g.y, (unsigned long long)g.z, (unsigned long long)b.x, (unsigned long long)b.y, (unsigned long long)b.z,
               lds_bytes, why);
  return status;
}
template <class... Params, class... Args>
int pa_launch(pa_ctx *c, const char *name, void (*kernel)(Params...), bool raise_lds, LaunchDim grid, LaunchDim block, size_t lds_bytes,
              hipStream_t stream, Args &&...args) {
  const hipDeviceProp_t &p = c->prop;
  const LaunchLimits lim{{(uint64_t)p.maxGridSize[0], (uint64_t)p.maxGridSize[1], (uint64_t)p.maxGridSize[2]},
                         {(uint64_t)p.maxThreadsDim[0], (uint64_t)p.maxThreadsDim[1], (uint64_t)p.maxThreadsDim[2]},
                         (uint64_t)p.maxThreadsPerBlock};
  switch (launch_verdict(grid, block, lim)) {
    case LaunchVerdict::kEmptyGrid: return PA_OK;
    case LaunchVerdict::kOutsideLimits: return pa_launch_refused(name, grid, block, lds_bytes, "beyond the device's limits", PA_E_INVALID);
    case LaunchVerdict::kGo: break;
  }
  if (raise_lds)
    PA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  kernel<<<dim3((uint32_t)grid.x, (uint32_t)grid.y, (uint32_t)grid.z), dim3((uint32_t)block.x, (uint32_t)block.y, (uint32_t)block.z), lds_bytes,
           stream ? stream : c->stream>>>(std::forward<Args>(args)...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PA_OK : pa_launch_refused(name, grid, block, lds_bytes, hipGetErrorString(e), PA_E_HIP);
}
#define PA_LAUNCH_ON(c, stream, kernel, grid, block, lds_bytes, ...) \
  pa_launch(c, #kernel, kernel, false, grid, block, lds_bytes, stream, __VA_ARGS__)
#define PA_LAUNCH(c, kernel, grid, block, lds_bytes, ...) PA_LAUNCH_ON(c, nullptr, kernel, grid, block, lds_bytes, __VA_ARGS__)
#define PA_LAUNCH_RAISE_LDS(c, kernel, grid, block, lds_bytes, ...) \
  pa_launch(c, #kernel, kernel, true, grid, block, lds_bytes, nullptr, __VA_ARGS__)

// ---- device primitives implemented in the .hip files -----------------------
// radix_sort.hip
// Stable LSD radix sort of (u64 key, u32 val) pairs on bits [bit_lo, bit_hi) of the key
// (or of the value when by_val), in passes of one whole 8-bit digit: bit_lo >= 0, bit_hi - bit_lo
// a multiple of 8, bit_hi <= 64 (<= 32 when by_val); anything else is PA_E_INVALID before a launch.
// keys/vals are double buffers: *which says which one holds the input on entry and the result
// on return.  n <= 1 or bit_hi <= bit_lo: nothing to do, nothing is touched.
int pa_radix_sort_pairs(pa_ctx *c, uint64_t *keys[2], uint32_t *vals[2], uint64_t n, int bit_lo,
                        int bit_hi, bool by_val, int *which);
// Exclusive prefix sums of n u32 values, themselves u32: they wrap past 2^32.  The total is
// added up in 64 bits from the tiles' 32-bit sums and goes to *d_total_u64 where that is not null.
int pa_exclusive_scan_u32(pa_ctx *c, const uint32_t *d_in, uint32_t *d_out, uint64_t n,
                          uint64_t *d_total_u64 /*nullable device ptr*/);
// The scan with its total read back: one wait on c->stream, directly after the scan's launches.
inline int pa_scan_total_u32(pa_ctx *c, const uint32_t *d_in, uint32_t *d_out, uint64_t n, uint64_t *d_total_u64, uint64_t *h_total) {
  PA_TRY(pa_exclusive_scan_u32(c, d_in, d_out, n, d_total_u64));
  return pa_read_back(c, d_total_u64, h_total);
}

// distmat.hip
// The check of `count` (1 or 2) n x n distance matrices on the device against distmat_rule.h's rule: one launch each, one
// read-back for all through kDistBad.  PA_OK, or PA_E_INVALID with the message "<who>: <names[m]>[i,j] is ..." for the
// first matrix, in argument order, that breaks it.
int pa_check_distance_matrices(pa_ctx *c, const char *who, const char *const *names, const double *const *d_M, int count, uint32_t n);
// One matrix, named D
inline int pa_check_distance_matrix(pa_ctx *c, const char *who, const double *d_D, uint32_t n) {
  const char *const name = "D";
  return pa_check_distance_matrices(c, who, &name, &d_D, 1, n);
}

// fragani.hip
void pa_fragani_release(pa_ctx *c);

// kmer_hash.hip
// The arena as the hash kernels read it.  dirty: one bit per block, set when the block needs its mask words
// (pa_build_dirty).
struct ArenaView {
  const uint32_t *packed = nullptr, *mask = nullptr;
  const uint64_t *dirty = nullptr;
  uint64_t n_blocks64 = 0;
};
// Where a surviving hash goes.  With region_off != nullptr the survivors of genome g go, unordered, to
// cand_hash[region_off[g] + i), i < cursor[g] (zeroed by the caller), and *overflow is set if a region was too small;
// otherwise (hash, genome) goes to slot atomicAdd(count) of cand_hash / cand_genome while that is below cap.
struct CandSink {
  uint64_t *cand_hash = nullptr;
  uint32_t *cand_genome = nullptr;
  uint64_t cap = 0;
  uint64_t *count = nullptr;
  const uint64_t *region_off = nullptr;
  uint32_t *cursor = nullptr, *overflow = nullptr;
  const uint32_t *genome_blk = nullptr;  // genome g is blocks [genome_blk[g], genome_blk[g + 1])
  uint32_t n_genomes = 0;
};
// One launch: arena blocks [blk0, arena.n_blocks64) on `stream` (default: the context's); blk0 is a multiple of 64.
struct KmerHashArgs {
  ArenaView arena;
  uint32_t k = 0;
  uint64_t max_hash = 0;
  CandSink sink;
  uint64_t blk0 = 0;
  hipStream_t stream = nullptr;
};
int pa_launch_kmer_hash(pa_ctx *c, const KmerHashArgs &a);

// The host plan of a sketch call (pa_sketch, pa_sketch_streamed): what follows from the genome starts alone.
struct SketchPlan {
  std::vector<uint32_t> blk;         // genome g is arena blocks [blk[g], blk[g + 1])
  std::vector<uint64_t> region_off;  // its candidate region is slots [region_off[g], region_off[g + 1])
  uint64_t longest_region = 0;
  double frac = 1.0;  // expected survivors: one window in 2^64/(max_hash+1)
  uint64_t n_blocks = 0;
};
// Checks everything the entry points require of the arena's size, k and the genome starts (`who` begins the messages),
// then fills the plan.  A region is the genome's expected survivors + 25 % + 128 slots.
inline int pa_sketch_plan(const uint64_t *h_genome_start, uint32_t n_genomes, uint64_t arena_bases, uint32_t k, uint64_t max_hash,
                          const char *who, SketchPlan *plan) {
  PA_REQUIRE((arena_bases % PA_ALIGN_BASES) == 0, "%s: arena_bases %llu is not a multiple of %u", who,
             (unsigned long long)arena_bases, PA_ALIGN_BASES);
  PA_REQUIRE(k >= 1 && k <= PA_MAX_K, "%s: k=%u outside [1,%u]", who, k, PA_MAX_K);
  PA_REQUIRE(h_genome_start[n_genomes] == arena_bases, "%s: genome_start[n] must equal arena_bases", who);
  plan->n_blocks = arena_bases / PA_ALIGN_BASES;
  plan->frac = (max_hash == UINT64_MAX) ? 1.0 : ((double)max_hash + 1.0) / 18446744073709551616.0;
  plan->blk.assign((size_t)n_genomes + 1, 0);
  plan->region_off.assign((size_t)n_genomes + 1, 0);
  plan->longest_region = 0;
  for (uint32_t g = 0; g <= n_genomes; ++g) {
    const uint64_t s = h_genome_start[g];
    PA_REQUIRE((s % PA_ALIGN_BASES) == 0 && (g == 0 || s >= h_genome_start[g - 1]) && s <= arena_bases,
               "%s: genome_start[%u]=%llu must be an ascending multiple of %u inside the arena", who, g,
               (unsigned long long)s, PA_ALIGN_BASES);
    plan->blk[g] = (uint32_t)(s / PA_ALIGN_BASES);
    if (g < n_genomes) {
      const uint64_t room = (uint64_t)((double)(h_genome_start[g + 1] - s) * plan->frac * 1.25) + 128;
      plan->longest_region = std::max(plan->longest_region, room);
      plan->region_off[g + 1] = plan->region_off[g] + room;
    }
  }
  PA_REQUIRE(plan->n_blocks < (1ULL << 32), "%s: arena too large", who);
  return PA_OK;
}
// capi.hip.  Region mode begins: the plan's two tables go up to genome_blk and region_off (the caller waits on
// c->stream while the plan is alive), cand_keys[0] holds all regions, the cursors and kRegionOverflow are zeroed.
int pa_regions_begin(pa_ctx *c, const SketchPlan &plan);
CandSink pa_region_sink(pa_ctx *c, uint32_t n_genomes);  // the sink over those buffers
// pa_sketch behind its argument checks: the arena is on the device, the plan made
int pa_sketch_resident(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty_in,
                       const SketchPlan &plan, uint32_t k, uint64_t max_hash, uint64_t *d_hashes, uint64_t cap_hashes,
                       uint64_t *d_off, uint64_t *h_total);

// Dirty bitmap of an arena (sketch_stream.hip): bit b of word w <-> block 64*w + b holds an invalid position, or
// the 32 positions before it do, or it is block 0.  ceil(n_blocks64 / 64) words.
int pa_build_dirty(pa_ctx *c, const uint32_t *d_mask, uint64_t n_blocks64, uint64_t *d_dirty, hipStream_t stream = nullptr);
// The bitmap the caller handed in, or one built into the context's own buffer when it handed in none.
int pa_dirty_or_build(pa_ctx *c, const uint32_t *d_mask, uint64_t n_blocks64, const uint64_t *d_dirty, const uint64_t **out);

// sketch_lds.hip: per-genome regions -> sorted unique CSR sketches, one workgroup and one LDS sort per genome
constexpr uint32_t kLdsSortMax = 16384;  // longest region the LDS sort takes
int pa_sketch_from_regions(pa_ctx *c, uint64_t *d_regions, const uint64_t *d_region_off, const uint32_t *d_cursor,
                           const uint32_t *d_overflow, uint32_t n_genomes, uint32_t longest_region, uint64_t max_hash,
                           uint64_t *d_hashes, uint64_t cap_hashes, uint64_t *d_off, uint64_t *h_total, bool *h_overflow);

// sketch_build.hip
int pa_build_sketch_csr(pa_ctx *c, const uint64_t *d_sorted_hash, const uint32_t *d_sorted_genome,
                        uint64_t n_cand, uint32_t n_genomes, uint64_t *d_hashes, uint64_t cap_hashes,
                        uint64_t *d_off, uint64_t *h_total);

// pairs_bitrow.hip / pairs_merge.hip
int pa_pairs_bitrow(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n, uint64_t total,
                    uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, uint32_t *d_counts);
int pa_dense_ids_sorted(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n, uint64_t P,
                        uint64_t *n_distinct);
int pa_pairs_bitrow_hash(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, const uint64_t *h_off /*nullable*/,
                         uint32_t n, uint64_t total, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1,
                         uint32_t *d_counts);
int pa_pair_dict_prepare_impl(pa_ctx *c, const uint64_t *d_subject_hashes, uint64_t n_postings);
int pa_pairs_merge(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n, uint32_t q0,
                   uint32_t q1, uint32_t s0, uint32_t s1, uint32_t *d_counts);

// ani.hip
int pa_launch_ani(pa_ctx *c, const uint32_t *d_counts, const uint64_t *d_off, uint32_t q0, uint32_t q1,
                  uint32_t s0, uint32_t s1, uint32_t k, double *d_identity, double *d_cov_query);
