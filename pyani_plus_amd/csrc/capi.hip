// capi.hip -- extern "C" entry points of libpyani_hip.so (see include/pyani_hip.h).
#include <algorithm>
#include <cstdarg>
#include <cstring>

#include "pa_internal.h"

// ---- errors -----------------------------------------------------------------
static thread_local char g_err[1024] = "";

void pa_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- profiling ----------------------------------------------------------------
static hipEvent_t take_event(pa_ctx *c) {
  if (!c->event_pool.empty()) {
    hipEvent_t e = c->event_pool.back();
    c->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

ProfScope::ProfScope(pa_ctx *ctx, int ph) : c(ctx), phase(ph) {
  if (!c->prof_on) return;
  e0 = take_event(c);
  e1 = take_event(c);
  if (e0) (void)hipEventRecord(e0, c->stream);
}

ProfScope::~ProfScope() {
  if (!c->prof_on || !e0 || !e1) return;
  (void)hipEventRecord(e1, c->stream);
  c->prof[phase].pending.emplace_back(e0, e1);
}

extern "C" {

int pa_abi_version(void) { return PA_ABI_VERSION; }
const char *pa_last_error(void) { return g_err; }

int pa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pa_ctx_create(int device, pa_ctx **out) {
  PA_REQUIRE(out != nullptr, "pa_ctx_create: out is null");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    pa_set_error("no HIP device available (%s); libpyani_hip has no CPU fallback",
                 e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    return PA_E_NODEVICE;
  }
  PA_REQUIRE(device >= 0 && device < n, "pa_ctx_create: device %d out of range [0,%d)", device, n);
  PA_HIP(hipSetDevice(device));
  pa_ctx *c = new (std::nothrow) pa_ctx();
  if (!c) { pa_set_error("out of host memory"); return PA_E_NOMEM; }
  c->device = device;
  if (hipGetDeviceProperties(&c->prop, device) != hipSuccess) { delete c; pa_set_error("hipGetDeviceProperties failed"); return PA_E_HIP; }
  if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
    pa_set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device, c->prop.gcnArchName);
    delete c;
    return PA_E_NODEVICE;
  }
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; pa_set_error("hipStreamCreate failed"); return PA_E_HIP; }
  c->own_stream = true;
  if (hipHostMalloc(reinterpret_cast<void **>(&c->h_pinned), kPinnedBytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipStreamDestroy(c->stream); delete c; pa_set_error("hipHostMalloc failed"); return PA_E_NOMEM;
  }
  if (c->counters.reserve(kCtxScalarBytes) != PA_OK) { (void)hipHostFree(c->h_pinned); (void)hipStreamDestroy(c->stream); delete c; return PA_E_NOMEM; }
  *out = c;
  return PA_OK;
}

void pa_ctx_destroy(pa_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->each_buffer([](DevBuf &b) { b.release(); });
  pa_fragani_release(c);
  for (auto &ph : c->prof)
    for (auto &pr : ph.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  if (c->h_pinned) (void)hipHostFree(c->h_pinned);
  if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); c->copy_stream = nullptr; }
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int pa_ctx_set_stream(pa_ctx *c, void *hip_stream) {
  PA_REQUIRE(c != nullptr, "null context");
  PA_HIP(hipStreamSynchronize(c->stream));
  // the copy stream of pa_sketch_streamed does not depend on the compute stream: it stays as it is
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  c->stream = reinterpret_cast<hipStream_t>(hip_stream);  // nullptr = the default stream
  c->own_stream = false;
  return PA_OK;
}

int pa_ctx_own_stream(pa_ctx *c) {
  PA_REQUIRE(c != nullptr, "null context");
  if (c->own_stream) return PA_OK;
  PA_HIP(hipStreamSynchronize(c->stream));
  PA_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  return PA_OK;
}

int pa_ctx_sync(pa_ctx *c) {
  PA_REQUIRE(c != nullptr, "null context");
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}

int pa_ctx_device_info(pa_ctx *c, char *name256, int *compute_units, uint64_t *global_mem) {
  PA_REQUIRE(c != nullptr, "null context");
  if (name256) { snprintf(name256, 256, "%s (%s)", c->prop.name, c->prop.gcnArchName); }
  if (compute_units) *compute_units = c->prop.multiProcessorCount;
  if (global_mem) *global_mem = (uint64_t)c->prop.totalGlobalMem;
  return PA_OK;
}

int pa_dev_alloc(pa_ctx *c, uint64_t bytes, void **d_out) {
  PA_REQUIRE(c && d_out, "pa_dev_alloc: null argument");
  PA_HIP(hipSetDevice(c->device));
  hipError_t e = hipMalloc(d_out, bytes ? bytes : 16);
  if (e != hipSuccess) { pa_set_error("hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e)); return PA_E_NOMEM; }
  return PA_OK;
}
int pa_dev_free(pa_ctx *c, void *d_ptr) {
  PA_REQUIRE(c != nullptr, "null context");
  if (d_ptr) { PA_HIP(hipStreamSynchronize(c->stream)); PA_HIP(hipFree(d_ptr)); }
  return PA_OK;
}
int pa_memcpy_h2d(pa_ctx *c, void *d_dst, const void *h_src, uint64_t bytes) {
  PA_REQUIRE(c != nullptr, "null context");
  if (bytes == 0) return PA_OK;
  PA_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}
int pa_memcpy_d2h(pa_ctx *c, void *h_dst, const void *d_src, uint64_t bytes) {
  PA_REQUIRE(c != nullptr, "null context");
  if (bytes == 0) return PA_OK;
  PA_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  PA_HIP(hipStreamSynchronize(c->stream));
  return PA_OK;
}
int pa_memset_d(pa_ctx *c, void *d_dst, int value, uint64_t bytes) {
  PA_REQUIRE(c != nullptr, "null context");
  if (bytes == 0) return PA_OK;
  PA_HIP(hipMemsetAsync(d_dst, value, bytes, c->stream));
  return PA_OK;
}

}  // extern "C"

// ---- sketch -------------------------------------------------------------------
int pa_regions_begin(pa_ctx *c, const SketchPlan &plan) {
  const uint64_t n = plan.blk.size() - 1;
  PA_TRY(c->genome_blk.reserve((n + 1) * sizeof(uint32_t)));
  PA_TRY(c->region_off.reserve((n + 1) * sizeof(uint64_t)));
  PA_TRY(c->region_cursor.reserve(n * sizeof(uint32_t)));
  PA_TRY(c->cand_keys[0].reserve(plan.region_off[n] * sizeof(uint64_t)));
  PA_HIP(hipMemcpyAsync(c->genome_blk.p, plan.blk.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipMemcpyAsync(c->region_off.p, plan.region_off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  PA_HIP(hipMemsetAsync(c->region_cursor.p, 0, n * sizeof(uint32_t), c->stream));
  PA_HIP(hipMemsetAsync(c->slot(kRegionOverflow), 0, kRegionOverflow.bytes(), c->stream));
  return PA_OK;
}

CandSink pa_region_sink(pa_ctx *c, uint32_t n_genomes) {
  CandSink s;
  s.cand_hash = c->cand_keys[0].as<uint64_t>();
  s.region_off = c->region_off.as<uint64_t>();
  s.cursor = c->region_cursor.as<uint32_t>();
  s.overflow = c->slot(kRegionOverflow);
  s.genome_blk = c->genome_blk.as<uint32_t>();
  s.n_genomes = n_genomes;
  return s;
}

int pa_sketch_resident(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty_in,
                       const SketchPlan &plan, uint32_t k, uint64_t max_hash, uint64_t *d_hashes, uint64_t cap_hashes,
                       uint64_t *d_off, uint64_t *h_total) {
  *h_total = 0;
  const uint32_t n_genomes = (uint32_t)plan.blk.size() - 1;
  const uint64_t arena_bases = plan.n_blocks * PA_ALIGN_BASES;
  // When the longest region fits an LDS sort the sketches are finished by sketch_lds.hip; otherwise, or if a region
  // overflows, by the global sort below.
  static const bool force_global = [] {
    const char *v = PA_TOOL_ENV("PA_SKETCH_SORT");
    return v && v[0] == 'g';
  }();
  const bool use_regions = !force_global && n_genomes > 0 && plan.longest_region <= kLdsSortMax;
  if (use_regions) {
    PA_TRY(pa_regions_begin(c, plan));
  } else {  // the global candidate list needs the block table only
    PA_TRY(c->genome_blk.reserve(plan.blk.size() * sizeof(uint32_t)));
    PA_HIP(hipMemcpyAsync(c->genome_blk.p, plan.blk.data(), plan.blk.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  }
  KmerHashArgs hash;
  hash.arena = {d_packed, d_mask, nullptr, plan.n_blocks};
  hash.k = k;
  hash.max_hash = max_hash;
  PA_TRY(pa_dirty_or_build(c, d_mask, plan.n_blocks, d_dirty_in, &hash.arena.dirty));
  PA_HIP(hipStreamSynchronize(c->stream));  // the uploads read the caller's plan

  if (use_regions) {
    hash.sink = pa_region_sink(c, n_genomes);
    {
      ProfScope prof(c, PA_PROF_KMER_HASH);
      PA_TRY(pa_launch_kmer_hash(c, hash));
    }
    bool overflow = false;
    {
      ProfScope prof(c, PA_PROF_SKETCH_SORT);
      const int st = pa_sketch_from_regions(c, hash.sink.cand_hash, hash.sink.region_off, hash.sink.cursor, hash.sink.overflow,
                                            n_genomes, (uint32_t)plan.longest_region, max_hash, d_hashes, cap_hashes, d_off,
                                            h_total, &overflow);
      if (st != PA_OK) return st;
    }
    if (!overflow) return PA_OK;
    *h_total = 0;  // a region was too small (repeats, low-complexity sequence): take the general path
  }
  uint64_t cap = (uint64_t)((double)arena_bases * plan.frac * 1.25) + 65536;
  if (cap > arena_bases) cap = arena_bases;
  uint64_t *d_count = c->slot<uint64_t>(kCandCount);
  uint64_t n_cand = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    for (int b = 0; b < 2; ++b) {
      PA_TRY(c->cand_keys[b].reserve(cap * sizeof(uint64_t)));
      PA_TRY(c->cand_vals[b].reserve(cap * sizeof(uint32_t)));
    }
    PA_HIP(hipMemsetAsync(d_count, 0, kCandCount.bytes(), c->stream));
    hash.sink = CandSink{};
    hash.sink.cand_hash = c->cand_keys[0].as<uint64_t>();
    hash.sink.cand_genome = c->cand_vals[0].as<uint32_t>();
    hash.sink.cap = cap;
    hash.sink.count = d_count;
    hash.sink.genome_blk = c->genome_blk.as<uint32_t>();
    hash.sink.n_genomes = n_genomes;
    {
      ProfScope prof(c, PA_PROF_KMER_HASH);
      PA_TRY(pa_launch_kmer_hash(c, hash));
    }
    PA_TRY(pa_read_back(c, d_count, &n_cand));
    if (n_cand <= cap) break;
    PA_REQUIRE(attempt == 0, "pa_sketch: candidate count changed between runs (%llu > %llu)",
               (unsigned long long)n_cand, (unsigned long long)cap);
    cap = n_cand;  // low-complexity input: rerun with the exact size
  }
  {
    ProfScope prof(c, PA_PROF_SKETCH_SORT);
    uint64_t *keys[2] = {c->cand_keys[0].as<uint64_t>(), c->cand_keys[1].as<uint64_t>()};
    uint32_t *vals[2] = {c->cand_vals[0].as<uint32_t>(), c->cand_vals[1].as<uint32_t>()};
    int which = 0;
    int hash_bits = max_hash ? 64 - __builtin_clzll(max_hash) : 0;
    hash_bits = (hash_bits + 7) & ~7;
    int genome_bits = n_genomes > 1 ? 32 - __builtin_clz(n_genomes - 1) : 0;
    genome_bits = (genome_bits + 7) & ~7;
    // LSD: least significant component (hash) first, then genome -> genome-major, hash-minor
    PA_TRY(pa_radix_sort_pairs(c, keys, vals, n_cand, 0, hash_bits, false, &which));
    PA_TRY(pa_radix_sort_pairs(c, keys, vals, n_cand, 0, genome_bits, true, &which));
    int st = pa_build_sketch_csr(c, keys[which], vals[which], n_cand, n_genomes, d_hashes, cap_hashes, d_off, h_total);
    if (st != PA_OK) return st;
  }
  return PA_OK;
}

extern "C" {

int pa_sketch(pa_ctx *c, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty_in, uint64_t arena_bases,
              const uint64_t *h_genome_start, uint32_t n_genomes, uint32_t k, uint64_t max_hash, uint64_t *d_hashes,
              uint64_t cap_hashes, uint64_t *d_off, uint64_t *h_total) {
  PA_REQUIRE(c && d_off && h_total && h_genome_start, "pa_sketch: null argument");
  PA_REQUIRE(arena_bases == 0 || (d_packed && d_mask), "pa_sketch: null arena");
  SketchPlan plan;
  PA_TRY(pa_sketch_plan(h_genome_start, n_genomes, arena_bases, k, max_hash, "pa_sketch", &plan));
  PA_HIP(hipSetDevice(c->device));
  return pa_sketch_resident(c, d_packed, d_mask, d_dirty_in, plan, k, max_hash, d_hashes, cap_hashes, d_off, h_total);
}

// ---- pairs ----------------------------------------------------------------------
int pa_pair_counts_ex(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, const uint64_t *h_off, uint32_t n,
                      uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, uint32_t *d_counts, int algo) {
  PA_REQUIRE(c && d_off, "pa_pair_counts: null argument");
  PA_REQUIRE(q0 <= q1 && q1 <= n && s0 <= s1 && s1 <= n, "pa_pair_counts: ranges [%u,%u) x [%u,%u) outside [0,%u)", q0,
             q1, s0, s1, n);
  PA_REQUIRE(algo == PA_PAIRS_AUTO || algo == PA_PAIRS_BITROW || algo == PA_PAIRS_MERGE || algo == PA_PAIRS_BITROW_HASH,
             "pa_pair_counts: unknown algo %d", algo);
  PA_HIP(hipSetDevice(c->device));
  if (q0 == q1 || s0 == s1) { c->dict_prepared = false; return PA_OK; }  // empty tile: nothing to write
  PA_REQUIRE(d_counts != nullptr, "pa_pair_counts: null counts buffer");
  uint64_t total = 0;
  if (h_off) {
    total = h_off[n];
  } else {
    PA_TRY(pa_read_back(c, d_off + n, &total));
  }
  PA_REQUIRE(total == 0 || d_hashes, "pa_pair_counts: null hashes");
  if (algo != PA_PAIRS_AUTO && algo != PA_PAIRS_BITROW_HASH) c->dict_prepared = false;
  switch (algo) {
    case PA_PAIRS_AUTO:
    case PA_PAIRS_BITROW_HASH:
      return pa_pairs_bitrow_hash(c, d_hashes, d_off, h_off, n, total, q0, q1, s0, s1, d_counts);
    case PA_PAIRS_BITROW:
      return pa_pairs_bitrow(c, d_hashes, d_off, n, total, q0, q1, s0, s1, d_counts);
    case PA_PAIRS_MERGE:
      return pa_pairs_merge(c, d_hashes, d_off, n, q0, q1, s0, s1, d_counts);
    default:
      pa_set_error("pa_pair_counts: unknown algo %d", algo);
      return PA_E_INVALID;
  }
}

int pa_pair_counts(pa_ctx *c, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n, uint32_t q0, uint32_t q1,
                   uint32_t s0, uint32_t s1, uint32_t *d_counts, int algo) {
  return pa_pair_counts_ex(c, d_hashes, d_off, nullptr, n, q0, q1, s0, s1, d_counts, algo);
}

int pa_pair_dict_prepare(pa_ctx *c, const uint64_t *d_subject_hashes, uint64_t n_postings) {
  PA_REQUIRE(c && (n_postings == 0 || d_subject_hashes), "pa_pair_dict_prepare: null argument");
  PA_HIP(hipSetDevice(c->device));
  return pa_pair_dict_prepare_impl(c, d_subject_hashes, n_postings);
}

int pa_ani(pa_ctx *c, const uint32_t *d_counts, const uint64_t *d_off, uint32_t q0, uint32_t q1, uint32_t s0,
           uint32_t s1, uint32_t k, double *d_identity, double *d_cov_query) {
  PA_REQUIRE(c && d_counts && d_off && d_identity && d_cov_query, "pa_ani: null argument");
  PA_REQUIRE(k >= 1 && q0 <= q1 && s0 <= s1, "pa_ani: bad k or ranges");
  PA_HIP(hipSetDevice(c->device));
  return pa_launch_ani(c, d_counts, d_off, q0, q1, s0, s1, k, d_identity, d_cov_query);
}

// ---- profiling API ----------------------------------------------------------------
int pa_prof_enable(pa_ctx *c, int on) {
  PA_REQUIRE(c != nullptr, "null context");
  c->prof_on = on != 0;
  return PA_OK;
}

static int prof_drain(pa_ctx *c) {
  PA_HIP(hipStreamSynchronize(c->stream));
  for (auto &ph : c->prof) {
    for (auto &pr : ph.pending) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
        ph.total_ms += ms;
        ph.launches += 1;
      }
      c->event_pool.push_back(pr.first);
      c->event_pool.push_back(pr.second);
    }
    ph.pending.clear();
  }
  return PA_OK;
}

int pa_prof_reset(pa_ctx *c) {
  PA_REQUIRE(c != nullptr, "null context");
  PA_TRY(prof_drain(c));
  for (auto &ph : c->prof) { ph.total_ms = 0.0; ph.launches = 0; }
  return PA_OK;
}

int pa_prof_get(pa_ctx *c, int phase, double *total_ms, uint64_t *launches) {
  PA_REQUIRE(c != nullptr && phase >= 0 && phase < PA_PROF_NPHASES, "pa_prof_get: bad phase %d", phase);
  PA_TRY(prof_drain(c));
  if (total_ms) *total_ms = c->prof[phase].total_ms;
  if (launches) *launches = c->prof[phase].launches;
  return PA_OK;
}

#ifdef PA_TOOLS
// ---- probes of the device primitives (tests/test_gpu_sort_scan.py) ---------------
// The argument checks of an entry point, then the primitive of radix_sort.hip itself on c->stream.
int pa_tool_radix_sort_pairs(pa_ctx *c, uint64_t *d_keys0, uint64_t *d_keys1, uint32_t *d_vals0, uint32_t *d_vals1, uint64_t n, int bit_lo,
                             int bit_hi, int by_val, int *which) {
  PA_REQUIRE(c != nullptr && which != nullptr, "pa_tool_radix_sort_pairs: null context or which");
  PA_REQUIRE(*which == 0 || *which == 1, "pa_tool_radix_sort_pairs: *which is %d, not 0 or 1", *which);
  PA_REQUIRE(n == 0 || (d_keys0 && d_keys1 && d_vals0 && d_vals1), "pa_tool_radix_sort_pairs: null buffer for %llu elements",
             (unsigned long long)n);
  PA_HIP(hipSetDevice(c->device));
  uint64_t *keys[2] = {d_keys0, d_keys1};
  uint32_t *vals[2] = {d_vals0, d_vals1};
  return pa_radix_sort_pairs(c, keys, vals, n, bit_lo, bit_hi, by_val != 0, which);
}

int pa_tool_exclusive_scan_u32(pa_ctx *c, const uint32_t *d_in, uint32_t *d_out, uint64_t n, uint64_t *d_total_u64) {
  PA_REQUIRE(c != nullptr, "null context");
  PA_REQUIRE(n == 0 || (d_in && d_out), "pa_tool_exclusive_scan_u32: null buffer for %llu values", (unsigned long long)n);
  PA_HIP(hipSetDevice(c->device));
  return pa_exclusive_scan_u32(c, d_in, d_out, n, d_total_u64);
}
#endif

}  // extern "C"
