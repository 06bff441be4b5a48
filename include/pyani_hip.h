/*
 * pyani_hip.h -- C ABI of libpyani_hip.so, the MI355X (gfx950) compute backend
 * for pyani-plus's all-vs-all sketch -> ANI path.
 *
 * pyani-plus has no FFI of its own: its sourmash method shells out to
 * third-party tools.  Each entry point below therefore
 * replaces one *process launch* on that path, and the Python method module
 * (pyani_plus_amd/methods/sourmash_hip.py) binds them with ctypes exactly as a
 * maintainer would from pyani_plus/methods/ (stub shown in INTEGRATION.md).
 *
 *   pa_pack_fasta / pa_pack_seq   FASTA text -> 2-bit arena
 *        replaces the FASTA reader inside `sourmash scripts singlesketch`
 *        (pyani_plus/methods/sourmash.py:67-83); record/whitespace semantics of
 *        pyani_plus/utils.py:67-90.
 *   pa_sketch                     arena -> FracMinHash sketches (CSR of u64)
 *        replaces `sourmash scripts singlesketch -I DNA -p k=K,scaled=S`
 *        (pyani_plus/methods/sourmash.py:62-84).
 *   pa_pair_counts                sketches -> |Q n S| for a query x subject tile
 *        replaces `sourmash sig collect` x2 + `sourmash scripts manysearch`
 *        (pyani_plus/methods/sourmash.py:162-200).
 *   pa_ani / pa_ani_host          counts -> (identity, cov_query)
 *        replaces the manysearch CSV columns read at
 *        pyani_plus/methods/sourmash.py:107-110 and their mapping at
 *        pyani_plus/private_cli.py:1879-1880.
 *
 * Conventions: plain pointers and sizes only.  `d_` arguments are DEVICE
 * pointers (hipMalloc / torch storage), `h_` are host pointers.  Every function
 * returns 0 on success or a negative pa_status; pa_last_error() gives the
 * message of the calling thread's last failure.  A context is bound to one GPU
 * and one HIP stream and is not thread-safe.  Work is enqueued on the context's
 * stream; functions that return sizes to the host synchronise that stream.
 * There is NO CPU fallback: without a usable HIP device pa_ctx_create fails.
 */
#ifndef PYANI_HIP_H
#define PYANI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 5

/* every entry point below is exported with default visibility */
#define PA_API __attribute__((visibility("default")))

typedef enum pa_status {
  PA_OK = 0,
  PA_E_INVALID = -1,   /* bad argument */
  PA_E_HIP = -2,       /* HIP runtime error (message has the hipError string) */
  PA_E_NOMEM = -3,     /* host or device allocation failed */
  PA_E_CAPACITY = -4,  /* caller buffer too small; required size reported */
  PA_E_NODEVICE = -5,  /* no usable gfx950 device */
  PA_E_IO = -6,        /* database I/O failed (pa_sqlite_insert_comparisons) */
  PA_E_NOCONVERGE = -7 /* an iteration used up its max_iter (pa_symm_top_eigs); nothing partial is returned */
} pa_status;

typedef struct pa_ctx pa_ctx;

/* Arena geometry: every genome starts at a multiple of PA_ALIGN_BASES bases. */
#define PA_ALIGN_BASES 64u
#define PA_MAX_K 64u

/* ---- library / context ---- */
PA_API int pa_abi_version(void);
PA_API const char *pa_last_error(void);
/* number of HIP devices visible (0 if none; never initialises a context) */
PA_API int pa_device_count(void);
PA_API int pa_ctx_create(int device, pa_ctx **out);
PA_API void pa_ctx_destroy(pa_ctx *ctx);
/* Adopt an existing hipStream_t (e.g. torch's current stream).  NULL is HIP's default
 * (null) stream, which is what torch uses unless told otherwise.  A new context starts
 * on a private non-blocking stream; pa_ctx_own_stream() returns to it. */
PA_API int pa_ctx_set_stream(pa_ctx *ctx, void *hip_stream);
PA_API int pa_ctx_own_stream(pa_ctx *ctx);
PA_API int pa_ctx_sync(pa_ctx *ctx);
/* Device properties: name (<=255 chars), CU count, bytes of global memory. */
PA_API int pa_ctx_device_info(pa_ctx *ctx, char *name256, int *compute_units, uint64_t *global_mem);

/* ---- raw device memory, for callers without their own allocator ---- */
PA_API int pa_dev_alloc(pa_ctx *ctx, uint64_t bytes, void **d_out);
PA_API int pa_dev_free(pa_ctx *ctx, void *d_ptr);
PA_API int pa_memcpy_h2d(pa_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
PA_API int pa_memcpy_d2h(pa_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes);
PA_API int pa_memset_d(pa_ctx *ctx, void *d_dst, int value, uint64_t bytes);

/* ---- host side: text -> 2-bit arena (no GPU needed) ----
 * Arena layout (DESIGN.md "Data layout"):
 *   packed: uint32 words, 16 bases/word, base i in bits [2*(i%16), 2*(i%16)+1],
 *           A=0 C=1 G=2 T=3 (case-insensitive); invalid positions hold 0.
 *   mask:   uint32 words, 32 bases/word, bit (i%32) = 1 when position i is NOT
 *           a usable base: non-ACGT residue, the one-position separator written
 *           between FASTA records, or the padding after the last residue.  Every
 *           genome ends with AT LEAST ONE invalid position (then padding up to
 *           PA_ALIGN_BASES) so that no k-mer window can span two genomes; arenas
 *           built by other means must keep that invariant.
 * `packed`/`mask` point at the genome's first word inside the arena; `cap_bases`
 * (multiple of 64) is the room available.  An upper bound for any FASTA text of
 * n bytes is pa_pack_bound(n).
 * Outputs: n_bases = positions written incl. separators and padding (multiple
 * of 64), n_residues = sum of record lengths (the reference's Genome.length,
 * db_orm.py:832-866), n_records, n_invalid = non-ACGT residues.
 * FASTA semantics follow pyani_plus/utils.py:67-90: text before the first '>'
 * is ignored; " \t\r\n" are removed from sequence lines. */
PA_API uint64_t pa_pack_bound(uint64_t n_text_bytes);
PA_API int pa_pack_fasta(const uint8_t *h_text, uint64_t n_text, uint32_t *h_packed, uint32_t *h_mask,
                  uint64_t cap_bases, uint64_t *n_bases, uint64_t *n_residues, uint64_t *n_records,
                  uint64_t *n_invalid);
/* One bare residue string (no FASTA framing) = one record. */
PA_API int pa_pack_seq(const uint8_t *h_seq, uint64_t n_seq, uint32_t *h_packed, uint32_t *h_mask,
                uint64_t cap_bases, uint64_t *n_bases, uint64_t *n_invalid);

/* gzip data (one or more members, zero padding after the last accepted) -> bytes, what Python's gzip module does for
 * the reference (pyani_plus/utils.py:178-196).  decoder 0: the library's own inflate (64-bit bit buffer, two-level
 * tables; every member checked against its CRC-32 and length) with zlib over the same bytes on any failure -- the
 * loader's route; 1: the library's own only; 2: zlib only.  PA_E_CAPACITY with *n_out = bytes needed when cap is
 * too small; PA_E_INVALID for a corrupt or truncated stream. */
PA_API int pa_gunzip(const uint8_t *h_gz, uint64_t n_gz, uint8_t *h_out, uint64_t cap, uint64_t *n_out, int decoder);

/* ---- host side: files -> md5 + length + title + arena, on a pool of host threads ----
 * One pass per file does what the reference does in three (md5 of the decompressed bytes,
 * pyani_plus/utils.py:142-196; length and description, pyani_plus/db_orm.py:832-866; the
 * sketcher's own read, pyani_plus/methods/sourmash.py:67-83): read, gunzip (pa_gunzip's decoder 0), md5 (sixteen
 * files side by side where the CPU has AVX-512), parse, pack (pa_pack_fasta).  threads <= 0: pa_host_cpu_budget().
 * The scratch mappings of a batch (up to three, at most 3 GiB) are kept for the next call; the environment variable
 * PA_HOST_SLAB_CACHE=0 returns them to the system at once.
 * pa_fasta_batch_info returns the file's own status (PA_OK or a negative code with `message`,
 * e.g. "Has .gz ending, but x.fa.gz is NOT gzip compressed", db_orm.py:846-854); strings are
 * owned by the batch.  pa_fasta_batch_copy_arena concatenates the successfully loaded genomes
 * (failed files occupy no space) and writes genome_start[n+1]. */
typedef struct pa_fasta_batch pa_fasta_batch;
PA_API int pa_fasta_batch_load(const char *const *paths, uint32_t n, int threads, pa_fasta_batch **out);
PA_API int pa_fasta_batch_info(const pa_fasta_batch *batch, uint32_t i, char md5hex33[33], uint64_t *n_residues,
                        uint64_t *n_records, uint64_t *n_invalid, uint64_t *n_bases, uint64_t *n_text,
                        const char **description, const char **message, int *was_gzip);
/* FASTA records of file i (start relative to the genome's first position, residues); batch-owned */
PA_API int pa_fasta_batch_records(const pa_fasta_batch *batch, uint32_t i, const uint64_t **rec_start,
                           const uint64_t **rec_len, uint64_t *n_records);
PA_API uint64_t pa_fasta_batch_arena_bases(const pa_fasta_batch *batch);
PA_API int pa_fasta_batch_copy_arena(const pa_fasta_batch *batch, uint32_t *h_packed, uint32_t *h_mask,
                              uint64_t *h_genome_start);
PA_API void pa_fasta_batch_free(pa_fasta_batch *batch);

/* FracMinHash threshold for `scaled` (sourmash max_hash; fixtures pin
 * 61489146912365176 @300 and 18446744073709552 @1000). */
PA_API uint64_t pa_max_hash(uint64_t scaled);

/* ---- the arena's third array: which 64-position blocks need their mask words ----
 * The mask is a third of the arena's bytes and almost all zero; the hash kernel reads it only for the blocks
 * this bitmap flags (bit b of word w <-> block 64*w + b: the block, or the 32 positions before it, hold an
 * invalid position; block 0 always).  ceil(arena_bases / 4096) uint64 words.  Built once per arena (it
 * belongs to the layout like the mask itself); entry points that take `d_dirty` accept NULL and then build
 * it into a buffer of the context on every call, which costs one pass over the mask.  Like the packers above it
 * stands in for the FASTA reader inside `sourmash scripts singlesketch` (pyani_plus/methods/sourmash.py:67-83):
 * where that tool skips k-mers with a non-ACGT residue as it meets them, this says where they can occur at all. */
PA_API int pa_arena_dirty(pa_ctx *ctx, const uint32_t *d_mask, uint64_t arena_bases, uint64_t *d_dirty);

/* ---- sketch: arena -> sorted unique hashes per genome ----
 * d_packed/d_mask/d_dirty: arena of `arena_bases` positions (multiple of 64).
 * h_genome_start[n_genomes+1]: first position of each genome (multiples of 64,
 * ascending; last entry = arena_bases).
 * For every window of k valid bases inside one record: canonical k-mer ->
 * MurmurHash3_x64_128(seed 42).h1; kept when <= max_hash.  k from 1 to 64 (the reference hands any --kmersize to
 * sourmash, pyani_plus/public_cli_args.py:229, and sourmash's third default is 51; 33 to 64 run the 128-bit form of
 * the kernel); PA_E_INVALID beyond.
 * Outputs (device): d_hashes[cap_hashes] genome-major ascending duplicate-free,
 * d_off[n_genomes+1] CSR offsets.  *h_total = total hashes.  If the total
 * exceeds cap_hashes the call returns PA_E_CAPACITY with *h_total = required
 * size and writes nothing to d_hashes. */
PA_API int pa_sketch(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty,
              uint64_t arena_bases, const uint64_t *h_genome_start, uint32_t n_genomes, uint32_t k, uint64_t max_hash,
              uint64_t *d_hashes, uint64_t cap_hashes, uint64_t *d_off, uint64_t *h_total);

/* ---- sketch straight from a host arena, upload hidden behind the hash kernel ----
 * The reference's tools read their FASTA input from disk (pyani_plus/methods/sourmash.py:67-83); here the
 * packed genomes start in host memory.  pa_mask_runs (host) lists the runs of invalid positions of a mask
 * (returns their number; writes at most `cap`), so that the mask -- a third of the arena's bytes, almost all
 * zero -- crosses the bus as a few integers; pa_mask_from_runs rebuilds it in d_mask (arena_bases/8 bytes).
 * pa_sketch_streamed = pa_mask_from_runs + chunked upload of h_packed (page-locked for a truly asynchronous
 * copy) into d_packed (arena_bases/4 bytes) on a second stream while the hash kernel works on the chunks
 * that have arrived + the rest of pa_sketch.  Same outputs and error behaviour as pa_sketch; d_packed,
 * d_mask and d_dirty (NULL: not wanted) hold the complete arena afterwards. */
PA_API int64_t pa_mask_runs(const uint32_t *h_mask, uint64_t arena_bases, uint64_t *h_run_start, uint64_t *h_run_len,
                            uint64_t cap);
PA_API int pa_mask_from_runs(pa_ctx *ctx, const uint64_t *h_run_start, const uint64_t *h_run_len, uint32_t n_runs,
                             uint32_t *d_mask, uint64_t arena_bases);
PA_API int pa_sketch_streamed(pa_ctx *ctx, const uint32_t *h_packed, const uint64_t *h_run_start,
                              const uint64_t *h_run_len, uint32_t n_runs, uint64_t arena_bases,
                              const uint64_t *h_genome_start, uint32_t n_genomes, uint32_t k, uint64_t max_hash,
                              uint32_t *d_packed, uint32_t *d_mask, uint64_t *d_dirty, uint64_t *d_hashes,
                              uint64_t cap_hashes, uint64_t *d_off, uint64_t *h_total);

/* ---- pairs: CSR sketches -> intersection counts ----
 * d_hashes/d_off describe n sketches (any source: pa_sketch, a `.sig` cache,
 * an all-gather).  Computes d_counts[(q-q0)*(s1-s0) + (s-s0)] = |S_q n S_s| for
 * q in [q0,q1), s in [s0,s1).  algo: PA_PAIRS_AUTO, or force one kernel.
 * With the default algorithm an all-vs-all call (q range == s range) over more than one subject tile of 2048
 * columns evaluates only the tile pairs on and above the diagonal and mirrors the rest (|A n B| = |B n A|);
 * the environment variable PA_PAIRS_SYMMETRIC=0 evaluates every tile pair instead. */
#define PA_PAIRS_AUTO 0        /* = PA_PAIRS_BITROW_HASH */
#define PA_PAIRS_BITROW 1      /* dictionary by radix sort + bit-row column sums */
#define PA_PAIRS_MERGE 2       /* per-pair merge-path intersection */
#define PA_PAIRS_BITROW_HASH 3 /* dictionary by hash table (subjects of the tile only) + bit-row column sums */
PA_API int pa_pair_counts(pa_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n,
                   uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, uint32_t *d_counts, int algo);
/* Same, for a caller that already has the CSR offsets on the host (h_off[n+1] == the content of d_off: sketch
 * sizes read from a `.sig` cache, or received with the multi-GPU all-gather).  The default algorithm then runs
 * without any host round trip; with h_off == NULL this is pa_pair_counts. */
PA_API int pa_pair_counts_ex(pa_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_off, const uint64_t *h_off,
                      uint32_t n, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, uint32_t *d_counts, int algo);
/* Multi-GPU overlap: build the hash dictionary of one subject tile from its n_postings hashes (a rank's own
 * sketches, contiguous in device memory) while the sketch all-gather is still in flight -- the exchange that
 * replaces the `.sig` file lists handed to `sourmash sig collect` (pyani_plus/methods/sourmash.py:162-183).
 * The next pa_pair_counts(_ex) with the default algorithm must cover a single subject tile (<= 2048 columns)
 * holding exactly these postings -- the same hashes, wherever they now live: the call compares a fingerprint of the
 * tile's postings with the one taken here and fails with PA_E_INVALID on a mismatch -- and then skips its own
 * insert.  Any other pair call drops the preparation. */
PA_API int pa_pair_dict_prepare(pa_ctx *ctx, const uint64_t *d_subject_hashes, uint64_t n_postings);

/* ---- counts -> ANI ----
 * cov_query = (I/|Q|)^(1/k), identity = max(cov_query, (I/|S|)^(1/k));
 * I == 0 -> NaN in both (the reference's NULL, sourmash.py:141-144).
 * pa_ani runs on the device (f64; <= 1 ulp from libm);
 * pa_ani_host uses the host libm `pow`, which reproduces every reference
 * fixture bit for bit, and is what the JSON/DB boundary uses; rows are split over
 * n_threads host threads (0 = pa_host_cpu_budget(), at most 64), and with `symmetric` != 0 (square
 * block, queries and subjects are the same genomes in the same order) one pow per
 * ordered pair is computed instead of two: (I/|S|)^(1/k) of (q,s) is cov_query of (s,q). */
PA_API int pa_ani(pa_ctx *ctx, const uint32_t *d_counts, const uint64_t *d_off, uint32_t q0, uint32_t q1,
           uint32_t s0, uint32_t s1, uint32_t k, double *d_identity, double *d_cov_query);
PA_API int pa_ani_host(const uint32_t *h_counts, const uint64_t *h_q_sizes, const uint64_t *h_s_sizes,
                uint32_t nq, uint32_t ns, uint32_t k, double *h_identity, double *h_cov_query,
                uint8_t *h_is_null, int symmetric, uint32_t n_threads);

/* ---- bottom-m MinHash + Mash Jaccard (the mode BASELINE.json configs[1] names) ----
 * NOT a reference code path: pyani-plus only ever sketches with `scaled=N`
 * (pyani_plus/methods/sourmash.py:75-76, "num":0 in every fixture), so these three entry points
 * replace nothing and their parity is unpinned (checked against the oracle's restatement of the
 * published Mash estimator).  pa_sketch_bottom: the m smallest distinct hashes per genome, CSR as
 * pa_sketch (cap_hashes >= n*m).  pa_pair_mash: per ordered pair, among the min(m, |A u B|) smallest
 * hashes of the union (= denom) how many are in both (= common).  pa_ani_mash:
 * 1 + ln(2j/(1+j))/k with j = common/denom; NaN when common == 0. */
PA_API int pa_sketch_bottom(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty, uint64_t arena_bases,
                     const uint64_t *h_genome_start, uint32_t n_genomes, uint32_t k, uint32_t m, uint64_t *d_hashes,
                     uint64_t cap_hashes, uint64_t *d_off, uint64_t *h_total);
PA_API int pa_pair_mash(pa_ctx *ctx, const uint64_t *d_hashes, const uint64_t *d_off, uint32_t n, uint32_t q0, uint32_t q1,
                 uint32_t s0, uint32_t s1, uint32_t m, uint32_t *d_common, uint32_t *d_denom);
PA_API int pa_ani_mash(pa_ctx *ctx, const uint32_t *d_common, const uint32_t *d_denom, uint64_t n_pairs, uint32_t k,
                double *d_ani);

/* ---- fastANI-style fragment-mapping ANI (BASELINE configs[3]) ----
 * Replaces one `fastANI --ql queries -r subject --fragLen F -k K --minFraction M` process per subject
 * column (pyani_plus/private_cli.py:1044-1063): all ordered pairs of the arena's genomes in one call.
 * Contigs (FASTA records): h_contig_start[i] = first arena position, h_contig_len[i] = residues,
 * h_contig_genome[i] = owning genome, in arena order (pa_fasta_records / the packers' layout).
 * Outputs (host): h_total_frags[g] = sum over g's contigs of floor(len/fragLen) (the last column of a
 * fastANI line); h_matched[q*n+r] = kept (orthologous) fragments, h_ident_sum[q*n+r] = sum of their
 * identities in percent -- fastANI's own sum: float identities added in a float in (contig, bin) order, widened to
 * double here --, so ANI(q,r) = (float)sum / (float)matched IN FLOAT is the number fastANI prints, reported when
 * matched/total >= minFraction (pyani_plus/methods/fastani.py:98-120 parses exactly these three numbers).
 * Only the reference genomes [ref0, ref1) are mapped against (columns outside stay 0): the reference's worker is
 * called once per subject column (pyani_plus/private_cli.py:976-1063), and a column costs one column: the hash
 * dictionary, the seed-hit arrays and the table of best fragments hold the reference range only.
 * Algorithm and its parity (every fastANI value the reference holds, exactly): oracle/fragani_oracle.c.  k from 8 to 16 (fastANI itself stops at 16); fragLen in
 * [100, 65535]; at most 65535 genomes; contigs listed genome by genome, at most 65535 per genome and 2^20-1 in all;
 * at most 2^20-1 fragments per genome.  The workspace (44 GB as allocated for 1000 x 5 Mb genomes all against all; pa_fragani_workspace
 * reports it, pa_fragani_set_workspace_cap bounds it) stays in the context. */
PA_API int pa_fragani(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
               const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
               uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t frag_len, uint32_t ref0, uint32_t ref1,
               uint32_t *h_total_frags, uint32_t *h_matched, double *h_ident_sum);
/* The same with a query range: only the genomes [qry0, qry1) are mapped (rows outside are left untouched), which is
 * how the reference's worker feeds fastANI -- batches of at most 500 queries per process, the column file rewritten
 * after each (pyani_plus/private_cli.py:1029-1101) -- so that an interrupted worker keeps the finished batches.
 * flags: PA_FRAGANI_REUSE_INDEX = the arena, contigs, k and fragLen are exactly those of the previous pa_fragani(_ex)
 * call on this context and the reference index it built (minimizers, dictionary, postings: about a tenth of a run)
 * is taken over instead of being rebuilt; PA_E_INVALID when there is no such call, or when that call's reference range
 * does not hold this one (the dictionary holds the reference range's minimizers).  fastANI itself rebuilds the
 * reference's index in every process. */
#define PA_FRAGANI_REUSE_INDEX 1u
/* PA_FRAGANI_COLUMNS_ONLY: h_matched and h_ident_sum hold n_genomes rows of (ref1 - ref0) entries -- the columns of the
 * reference range and nothing else --, so that a worker asked for one subject column (the reference's layout: one
 * process per column, pyani_plus/public_cli.py:236-261) keeps O(n) results in host memory instead of an n x n matrix. */
#define PA_FRAGANI_COLUMNS_ONLY 2u
PA_API int pa_fragani_ex(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                  const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
                  uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t frag_len, uint32_t qry0, uint32_t qry1,
                  uint32_t ref0, uint32_t ref1, uint32_t flags, uint32_t *h_total_frags, uint32_t *h_matched,
                  double *h_ident_sum);
/* The fragment-ANI workspace of a context (the reference bounds a worker's memory by handing fastANI at most 500
 * queries per process, pyani_plus/private_cli.py:1029-1033; here the workspace is device memory that stays in the context
 * and only grows).  pa_fragani_workspace: bytes held now, the most ever held (the same, until pa_ctx_destroy), the cap
 * (0: none); any pointer may be null.  pa_fragani_set_workspace_cap: later pa_fragani / pa_fragani_ex / pa_fragani_sketch
 * calls that would take the workspace past cap_bytes end with PA_E_NOMEM and a pa_last_error() message that names the
 * call (genomes, arena residues, query and reference range, fragLen) and the sizes (bytes held, the buffer that wanted to
 * grow, the cap); a call that ends that way (or with the device's own out-of-memory) gives the whole workspace back, so a
 * smaller call in the same context starts from nothing and goes on working.  What a call needs (Memory;
 * as allocated, buffers grow by a quarter when they grow): about 2.3 bytes per arena residue for the minimizers of ALL
 * genomes, their hash ids and links; about 5.2 bytes per residue of the REFERENCE RANGE for its dictionary, postings and
 * the sort's buffers (a range that is not the whole set adds a look-up table of 32-64 bytes per distinct hash); 8 bytes per
 * seed hit of the largest query batch and ~1 GB of per-batch tables.  Measured at 1000 x 5 Mb (bench.py,
 * also.fragment_ani.workspace_device_bytes): 44.1 GB all against all, 19.7 GB an eighth of the columns, 12.9 GB one column. */
PA_API int pa_fragani_workspace(pa_ctx *ctx, uint64_t *held_bytes, uint64_t *peak_bytes, uint64_t *cap_bytes);
PA_API int pa_fragani_set_workspace_cap(pa_ctx *ctx, uint64_t cap_bytes);
/* Residues that are neither ACGT nor N.  The arena keeps two bits per residue and one "not ACGT" bit, which the
 * fragment-ANI kernels read as N; fastANI, which the reference hands the FASTA text itself
 * (pyani_plus/private_cli.py:1044-1063), hashes every upper-cased character as it is, so a k-mer over an IUPAC code
 * (R, Y, K, M, S, W, ...) hashes differently from the same k-mer over N.  The packers list such residues --
 * pa_text_ambiguous for a text packed by pa_pack_fasta / pa_pack_seq (positions relative to the genome's first),
 * pa_fasta_batch_ambiguous for a loaded batch (arena positions) --, and pa_fragani_set_ambiguous hands the list of the
 * arena at d_packed to the context (ascending arena positions, upper-cased bytes; copied; n = 0 forgets it): every later
 * pa_fragani / pa_fragani_ex / pa_fragani_sketch call on that arena hashes those residues as the characters they are.
 * Without a list every residue that is not ACGT is an N.  The sourmash path is not concerned: a window over any such
 * residue is skipped there, whatever the letter. */
PA_API int64_t pa_text_ambiguous(const uint8_t *h_text, uint64_t n_text, int fasta, uint64_t *h_pos, uint8_t *h_byte,
                                 uint64_t cap);
PA_API int64_t pa_fasta_batch_ambiguous(const pa_fasta_batch *batch, uint64_t *h_pos, uint8_t *h_byte, uint64_t cap);
PA_API int pa_fragani_set_ambiguous(pa_ctx *ctx, const uint32_t *d_packed, const uint64_t *h_pos, const uint8_t *h_byte,
                                    uint64_t n);
/* stage 1 alone (testing): the winnowed minimizers of every contig, in arena order */
PA_API int pa_fragani_sketch(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, uint64_t arena_bases,
                      const uint64_t *h_contig_start, const uint32_t *h_contig_len, const uint32_t *h_contig_genome,
                      uint32_t n_contigs, uint32_t n_genomes, uint32_t k, uint32_t window, uint32_t *h_hash,
                      uint32_t *h_wpos, uint32_t *h_contig, uint64_t cap, uint64_t *n_out);
/* parameters derived from (k, fragLen): winnowing window; per sketch size s the L1 seed threshold and
 * the smallest accepted number of shared minimizers; identity (percent) of shared/s */
PA_API int pa_fragani_window(uint32_t k, uint32_t frag_len);
PA_API int pa_fragani_tables(uint32_t k, uint32_t s_max, uint32_t *h_min_hits, uint32_t *h_min_shared);
PA_API double pa_fragani_identity(uint32_t shared, uint32_t s, uint32_t k);
/* record table of a FASTA text as pa_pack_fasta lays it out: start (relative to the genome's first
 * position) and length of each record; returns the number of records (may exceed cap) */
PA_API int64_t pa_fasta_records(const uint8_t *h_text, uint64_t n_text, uint64_t *h_rec_start, uint64_t *h_rec_len,
                         uint64_t cap);

/* ---- bulk writer of sourmash-format `.sig` files (the cache of pyani_plus/methods/sourmash.py:57-66) ----
 * File i = heads[i] + "h0,h1,..." + mids[i] + md5sum + tails[i], where the hashes are
 * h_mins[h_off[i] .. h_off[i+1]) in decimal and md5sum = md5(str(ksize) + concatenated decimals), sourmash's
 * checksum of a sketch.  The three text parts come from the caller (json.dumps of everything around the
 * `mins` list and the `md5sum` value).  Files are written to <path>.<pid>.tmp and renamed; n_threads 0 = pa_host_cpu_budget(). */
PA_API int pa_write_sigs(uint32_t n_files, const char *const *paths, const char *const *heads, const char *const *mids,
                         const char *const *tails, uint32_t ksize, const uint64_t *h_mins, const uint64_t *h_off,
                         uint32_t n_threads);

/* ---- bulk reader of sourmash-format `.sig` files ----
 * Replaces what `sourmash sig collect` + `manysearch` do with the N cached signatures of a column worker
 * (pyani_plus/methods/sourmash.py:160-200): open, JSON-parse and validate every file.  The n files are read on
 * n_threads host threads (0 = pa_host_cpu_budget()).  Per file (pa_sig_batch_info returns its status):
 *   PA_OK             one DNA sketch with this ksize and max_hash, num = 0; its hashes (ascending, duplicate-free)
 *                     are in the batch, and the file's own `md5sum` -- md5(str(ksize) + the decimals, concatenated)
 *                     -- matched them;
 *   PA_SIG_UNHANDLED  a readable signature file in another layout (several sketches, another k, protein, ...):
 *                     the caller parses it with a general JSON reader;
 *   PA_E_IO / PA_E_INVALID  unreadable or damaged (truncated list, non-numeric entry, checksum mismatch); `message`
 *                     says what, and the worker ends the way a failing `sourmash sig collect` ends the reference's
 *                     (pyani_plus/utils.py:262-283).
 * pa_sig_batch_copy writes the hashes of the PA_OK files back to back into h_mins and their CSR offsets into
 * h_off[n+1] (files with another status occupy no room); n_mins of pa_sig_batch_info sizes the buffer. */
#define PA_SIG_UNHANDLED 1
typedef struct pa_sig_batch pa_sig_batch;
PA_API int pa_read_sigs(const char *const *paths, uint32_t n, uint32_t ksize, uint64_t max_hash, uint32_t n_threads,
                        pa_sig_batch **out);
PA_API int pa_sig_batch_info(const pa_sig_batch *batch, uint32_t i, uint64_t *n_mins, const char **message);
PA_API int pa_sig_batch_copy(const pa_sig_batch *batch, uint64_t *h_mins, uint64_t *h_off);
PA_API void pa_sig_batch_free(pa_sig_batch *batch);

/* ---- bulk writer of the reference's JSON column file (pyani_plus/private_cli.py:454-504) ----
 * Writes prefix + rows + suffix, rows byte-identical to json.dumps of
 * {"query_hash", "subject_hash", "identity", "cov_query"} dicts (", " separated, `null` where
 * is_null, floats in Python repr form), query-major over the nq x ns matrices. */
PA_API int pa_write_comparisons_json(const char *path, const char *prefix, const char *suffix,
                              const char *const *q_hashes, uint32_t nq, const char *const *s_hashes, uint32_t ns,
                              const double *h_identity, const double *h_cov_query, const uint8_t *h_is_null);

/* Progressive form: `path` was written by pa_write_comparisons_json (possibly with no rows) and ends with
 * `suffix`; append one more block of rows in front of the suffix (file_has_rows: rows are already there, so a
 * ", " goes first).  The file is a complete JSON document after every call -- an interrupted worker leaves
 * the finished subject tiles behind, as pyani_plus/private_cli.py:1863-1894 does by re-dumping its list. */
PA_API int pa_append_comparisons_json(const char *path, const char *suffix, int file_has_rows,
                               const char *const *q_hashes, uint32_t nq, const char *const *s_hashes, uint32_t ns,
                               const double *h_identity, const double *h_cov_query, const uint8_t *h_is_null);

/* The same with the two proxy columns of the fastANI worker (pyani_plus/private_cli.py:1066-1080): rows become
 * {"query_hash", "subject_hash", "identity", "aln_length", "sim_errors", "cov_query"}, integers in decimal, all four
 * `null` where is_null.  aln_length == sim_errors == NULL: the four-key rows of pa_append_comparisons_json. */
PA_API int pa_append_comparisons_json_ex(const char *path, const char *suffix, int file_has_rows,
                                  const char *const *q_hashes, uint32_t nq, const char *const *s_hashes, uint32_t ns,
                                  const double *h_identity, const double *h_cov_query, const uint8_t *h_is_null,
                                  const int64_t *h_aln_length, const int64_t *h_sim_errors);

/* fastANI writes its identity with six significant digits and the reference parses that text
 * (pyani_plus/methods/fastani.py:98-120): every value -> printf("%.6g") -> value, in place; NaN stays NaN. */
PA_API int pa_round_sig6(double *h_values, uint64_t n);

/* Host threads worth starting: the CPUs the process may run on, capped by the cgroup CPU quota when there is one
 * (the reference sizes its worker pools with len(os.sched_getaffinity(0)), pyani_plus/utils.py:199-214, which
 * counts 256 on a box whose container is allowed 16 CPUs' worth of time).  The default of every n_threads = 0
 * argument in this header. */
PA_API uint32_t pa_host_cpu_budget(void);

/* ---- comparison rows into the run database ----
 * Replaces, for this method, the parent process's import of the column file: parse the JSON back and
 * INSERT OR IGNORE one row per comparison through the ORM (pyani_plus/private_cli.py:507-614,
 * pyani_plus/db_orm.py:1076).  The n_queries x n_subjects matrices (row = query) are bound to one prepared
 * INSERT OR IGNORE INTO comparisons (query_hash, subject_hash, configuration_id, identity, aln_length, sim_errors,
 * cov_query, uname_*) and stepped in query-major order inside one transaction on a connection of the call's own;
 * where is_null, identity and cov_query are NULL; aln_length and sim_errors always are (as in
 * pyani_plus/private_cli.py:1866-1880).  *rows_inserted = rows that were not already present.  The database must
 * exist with the reference's schema and must not be locked by another connection.  Uses the system's
 * libsqlite3.so.0 through dlopen; PA_E_IO if that is missing or any SQLite call fails (nothing is committed). */
PA_API int pa_sqlite_insert_comparisons(const char *database, int64_t configuration_id, const char *uname_system,
                                        const char *uname_release, const char *uname_machine,
                                        const char *const *query_hashes, uint32_t n_queries,
                                        const char *const *subject_hashes, uint32_t n_subjects,
                                        const double *h_identity, const double *h_cov_query, const uint8_t *h_is_null,
                                        uint64_t *rows_inserted);

/* The same with aln_length / sim_errors per comparison (both or neither; NULL where is_null): the fastANI worker's rows. */
PA_API int pa_sqlite_insert_comparisons_ex(const char *database, int64_t configuration_id, const char *uname_system,
                                           const char *uname_release, const char *uname_machine,
                                           const char *const *query_hashes, uint32_t n_queries,
                                           const char *const *subject_hashes, uint32_t n_subjects,
                                           const double *h_identity, const double *h_cov_query, const uint8_t *h_is_null,
                                           const int64_t *h_aln_length, const int64_t *h_sim_errors,
                                           uint64_t *rows_inserted);

/* ---- external alignment (method external-alignment-hip): an MSA -> per-pair counts ----
 * Replaces compute_external_alignment_column (pyani_plus/methods/external_alignment.py:33-156), called per subject
 * column by private_cli.compute_external_alignment (pyani_plus/private_cli.py:1930-2041).
 *
 *   pa_msa_load / _info / _record / _copy_rows / _free   the alignment file, read once
 *        replaces the two fasta_bytes_iterator passes per column (external_alignment.py:63-99, parser
 *        pyani_plus/utils.py:40-90) and file_md5sum of the alignment (private_cli.py:1985-1990).  One pass over the
 *        bytes: the md5 of the raw file on its own thread, the records parsed in parallel (titles = line[1:].rstrip(),
 *        sequence lines rstrip()ed and " \t\r\n" deleted; raw bytes, case-sensitive), a 256-bin histogram of the
 *        residue bytes.  threads <= 0: pa_host_cpu_budget().  pa_msa_copy_rows writes rows [r0, r1) with row_stride
 *        bytes each, a row's tail after its residues filled with '-'.
 *   pa_msa_pack          rows -> bit planes + non-gap counts n_x (device)
 *        d_rows: n_chunk_rows rows of row_stride bytes (a multiple of 32 covering ceil(n_cols / 32) words; 16-byte
 *        aligned), rows row0 .. of an MSA of n_rows rows.  The bytes of a row at or past n_cols, up to the end of its
 *        last 32-byte word, are read and ignored: those columns are gap in every plane whatever the bytes say, so the
 *        padding need not be '-'.  h_code256: byte -> code, '-' -> 0, codes below 2^bits
 *        (1 <= bits <= 8).  d_planes: pa_msa_plane_words(n_rows, n_cols, bits) uint32, word-major
 *        [(w * (bits + 1) + p) * n_pad + row], n_pad = n_rows rounded up to 64, plane `bits` = non-gap.  d_nongap:
 *        n_rows uint32, zero before the first chunk; each chunk adds its rows' non-gap columns.
 *   pa_msa_pair_counts   bit planes -> M (q == s, not gap) and B (neither gap), uint32 [q1 - q0][s1 - s0]
 *        replaces the per-pair numpy passes (external_alignment.py:118-132).  symmetric != 0 (equal ranges): only the
 *        64 x 64 tiles on and above the diagonal are evaluated and the rest mirrored on the device.
 *   pa_msa_metrics       (M, B, n_q, n_s) per pair -> identity, aln_length, sim_errors, cov_query, cov_subject (host)
 *        replaces external_alignment.py:134-156; IEEE divisions of integers below 2^53, bit-identical to the
 *        reference's int / int.  PA_E_INVALID when a row has no residues (the reference divides by zero).
 *   pa_append_msa_json   rows (q_idx[r], s_idx[r]) of the column file with the worker's seven keys
 *        (private_cli.py:2009-2032), in the order given, byte-identical to json.dumps; the progressive form of
 *        pa_append_comparisons_json. */
typedef struct pa_msa pa_msa;
PA_API int pa_msa_load(const char *path, int threads, pa_msa **out);
PA_API int pa_msa_info(const pa_msa *msa, uint32_t *n_records, uint64_t *max_len, char md5hex33[33], uint64_t *h_hist256);
PA_API int pa_msa_record(const pa_msa *msa, uint32_t i, const char **title, uint64_t *title_len, uint64_t *length);
PA_API int pa_msa_copy_rows(const pa_msa *msa, uint32_t r0, uint32_t r1, uint64_t row_stride, uint8_t *h_rows);
PA_API void pa_msa_free(pa_msa *msa);
PA_API uint64_t pa_msa_plane_words(uint32_t n_rows, uint64_t n_cols, uint32_t bits);
PA_API int pa_msa_pack(pa_ctx *ctx, const uint8_t *d_rows, uint64_t row_stride, uint32_t row0, uint32_t n_chunk_rows, uint32_t n_rows,
                       uint64_t n_cols, const uint8_t *h_code256, uint32_t bits, uint32_t *d_planes, uint32_t *d_nongap);
PA_API int pa_msa_pair_counts(pa_ctx *ctx, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, uint32_t bits, uint32_t q0,
                              uint32_t q1, uint32_t s0, uint32_t s1, int symmetric, uint32_t *d_match, uint32_t *d_both);
PA_API int pa_msa_metrics(const uint32_t *h_match, const uint32_t *h_both, const uint64_t *h_nq, const uint64_t *h_ns, uint64_t n_pairs,
                          double *h_identity, int64_t *h_aln_length, int64_t *h_sim_errors, double *h_cov_query,
                          double *h_cov_subject, uint32_t n_threads);
PA_API int pa_append_msa_json(const char *path, const char *suffix, int file_has_rows, const char *const *hashes, uint32_t n_hashes,
                              const uint32_t *q_idx, const uint32_t *s_idx, uint64_t n_rows, const double *identity,
                              const int64_t *aln_length, const int64_t *sim_errors, const double *cov_query, const double *cov_subject);

/* ---- classify: a run's matrices -> its genome cliques ----
 * Replaces construct_graph, find_initial_cliques, find_cliques_recursively and get_unique_cliques
 * (pyani_plus/classify.py:64-207).  Node p is row and column p of the two n x n row-major f64 matrices (rows = query,
 * columns = subject).  For every i < j: coverage = agg_cov(C[j,i], C[i,j]), score = agg_score(S[j,i], S[i,j]) with the
 * reference's argument order and NaN behaviour (Python's min and max keep a NaN first argument and pass over a NaN second
 * one; the mean is NaN for either); the pair is an edge iff neither is NaN and coverage > cov_min.
 *
 *   pa_classify_edges        (device) the edges in removal order: ascending score, equal scores (-0.0 equals 0.0) by
 *        ascending (i, j).  The four outputs are device arrays with room for cap_edges elements; *n_edges = E always.
 *        PA_E_CAPACITY when E > cap_edges (nothing written; n (n - 1) / 2 always suffices); PA_E_INVALID for
 *        n > 65536 (edge positions are 32-bit) or an unknown aggregator.  One host synchronisation (E is read back).
 *   pa_classify_edges_host   the same list from host matrices into host arrays (plain loops, std::stable_sort).
 *   pa_classify_tani_host    score matrix of tANI mode from the Hadamard matrix: NaN stays, 0 -> NaN, else
 *        (-log(h)) * -1 with the host libm log (db_orm.py:588, public_cli.py:1269); -log(1.0) * -1 is +0.0.
 *   pa_classify_cliques      (host) edges in removal order -> rows.  The edges are walked backwards with a union-find
 *        that counts nodes and edges per component; a component is recorded, when an edge of score s joins it to
 *        another one, iff it is a clique, with min_score = s; the components left at the end are recorded with no
 *        min_score if there is one of them or no edge at all, else with the smallest score of all.  Row order: if
 *        more than one component is left, those that are cliques by smallest member; then the component tree in
 *        pre-order (roots and children by smallest member), rows already listed skipped.
 *   pa_cliques_info / _copy / _free   number of rows and of members; n_nodes[R], max_cov[R], min_score[R],
 *        max_score[R], present[R] (bit 0: max_cov, 1: min_score, 2: max_score; an absent value is NaN), member_off[R + 1],
 *        members[member_off[R]] (ascending inside a row). */
#define PA_AGG_MIN 0
#define PA_AGG_MAX 1
#define PA_AGG_MEAN 2
typedef struct pa_cliques pa_cliques;
PA_API int pa_classify_edges(pa_ctx *ctx, const double *d_score, const double *d_cov, uint32_t n, int agg_score, int agg_cov,
                             double cov_min, uint64_t cap_edges, uint32_t *d_i, uint32_t *d_j, double *d_edge_score,
                             double *d_edge_cov, uint64_t *n_edges);
PA_API int pa_classify_edges_host(const double *h_score, const double *h_cov, uint32_t n, int agg_score, int agg_cov, double cov_min,
                                  uint64_t cap_edges, uint32_t *h_i, uint32_t *h_j, double *h_edge_score, double *h_edge_cov,
                                  uint64_t *n_edges);
PA_API int pa_classify_tani_host(const double *h_hadamard, uint64_t n_cells, double *h_score);
PA_API int pa_classify_cliques(uint32_t n, uint64_t n_edges, const uint32_t *h_i, const uint32_t *h_j, const double *h_edge_score,
                               const double *h_edge_cov, pa_cliques **out);
PA_API int pa_cliques_info(const pa_cliques *cl, uint64_t *n_rows, uint64_t *n_members);
PA_API int pa_cliques_copy(const pa_cliques *cl, uint32_t *n_nodes, double *max_cov, double *min_score, double *max_score,
                           uint8_t *present, uint64_t *member_off, uint32_t *members);
PA_API void pa_cliques_free(pa_cliques *cl);

/* ---- plot-run: clustered heatmap order ----
 * Restates what seaborn's clustermap computes with its defaults for the reference's plot-run
 * (pyani_plus/plot_run.py:114-147): scipy's linkage(rows, method="average", metric="euclidean") and the leaves of
 * dendrogram(..., no_plot=True), bit for bit.
 *
 *   pa_rowdist_euclid        (device) x is a row-major n x m f64 matrix in device memory; out receives the condensed
 *        distance vector, n (n - 1) / 2 doubles: out[n i - i (i + 1) / 2 + (j - i - 1)] = sqrt(sum over c = 0 .. m - 1,
 *        in this order, of (x[i,c] - x[j,c])^2) for i < j, the index computed in 64 bits.  One accumulator per pair, the
 *        square rounded before it is added (no FMA), the square root correctly rounded: the same bits as
 *        scipy.spatial.distance.pdist(x, "euclidean").  The inputs must be finite (plot-run fills NaN cells first); with
 *        NaN or infinite cells the result is whatever IEEE arithmetic gives and no order is promised to match.
 *        PA_E_INVALID for n > 65536.  n < 2 writes nothing.  The call allocates no device memory and does not
 *        synchronise; it runs on the context's stream.
 *   pa_rowdist_euclid_host   the same vector from a host matrix into a host array, plain loops on n_threads host
 *        threads (0: as many as the process may use).
 *   pa_linkage_average       (host) condensed distances of n observations -> Z, scipy's (n - 1) x 4 row-major f64
 *        linkage table (the two merged clusters, smaller id first; their distance; the size of the union; merge r is
 *        cluster n + r), and leaves, the n observation indices in the dendrogram's order (pre-order from the last merge,
 *        first child before the second).  Nearest-neighbour chain as in scipy: an empty chain restarts at the lowest
 *        live index, the nearest live cluster is searched in ascending index with a strict <, starting from the
 *        distance to the previous chain element, which therefore wins ties; the n - 1 merges are stable-sorted by
 *        distance and relabelled with a union-find.  The distances are not modified (the call works on a copy).
 *        n = 1: leaves = {0}, Z untouched (scipy raises; a one-genome run still plots); n = 0: nothing.
 *        PA_E_INVALID for n > 65536 and for a distance that is NaN or infinite (finite matrix cells do not rule that
 *        out: cells near 1e200 overflow the sum); PA_E_NOMEM when the copy cannot be made. */
PA_API int pa_rowdist_euclid(pa_ctx *ctx, const double *d_x, uint32_t n, uint32_t m, double *d_out);
PA_API int pa_rowdist_euclid_host(const double *h_x, uint32_t n, uint32_t m, double *h_out, uint32_t n_threads);
PA_API int pa_linkage_average(uint32_t n, const double *h_condensed, double *h_Z, uint32_t *h_leaves);

/* ---- plot-run-comp: two runs joined pair by pair, and the histograms of the joined values ----
 * Replaces the dictionaries keyed by (query_hash, subject_hash), the list comprehensions and the Axes.hist calls of
 * plot_run_comparison (pyani_plus/plot_run.py:404-575).  The reference run R is its n_ref x n_ref row-major f64
 * identity matrix (rows = query, columns = subject, NaN where R has no value); the other run O is one row per
 * comparison, in the caller's order: q and s, the u32 row and column of the comparison's genomes in R's matrix
 * (0xFFFFFFFF: a genome R does not have), and y, O's identity (NaN for NULL).
 *
 *   pa_runcomp_join          (device) a row survives iff q < n_ref, s < n_ref, y is not NaN and ref[q, s] is not NaN (the
 *        cell index q * n_ref + s is computed in 64 bits).  The survivors are written densely and in input order:
 *        x = ref[q, s], y, and diff = y - x (one f64 subtraction), into three device arrays with room for n_rows
 *        elements each; *n_common = their number.  Two passes with a prefix sum between them, no atomics; one host
 *        synchronisation (n_common is read back).  PA_E_INVALID for n_ref > 65536 and n_rows >= 2^32; n_rows = 0 is
 *        valid and writes nothing.
 *   pa_minmax_f64            (device) out[0], out[1] = minimum and maximum of the non-NaN values of d_v[n], *n_valid =
 *        their number; with n_valid = 0 out is untouched.  Compared as values: when -0.0 and 0.0 both occur, which of
 *        them comes back is not defined.  One host synchronisation.
 *   pa_hist_uniform_f64      (device) numpy.histogram's counts for uniform bins: h_edges are bins + 1 ascending finite
 *        doubles from the caller (numpy.linspace(first, last, bins + 1) in the driver, so they have numpy's bits),
 *        h_counts is u64[bins].  v is counted iff v >= edges[0] && v <= edges[bins] (NaN is not).  Its bin is
 *        ((v - edges[0]) / (edges[bins] - edges[0])) * bins truncated -- a correctly rounded division, then the
 *        multiplication, two roundings -- set to bins - 1 where it came out bins, decremented where v < edges[i], then
 *        incremented where v >= edges[i + 1] and i != bins - 1 (numpy/lib/_histograms_impl.py, the uniform-bins branch).
 *        PA_E_INVALID for bins outside 1 .. 1024, an edge that is not finite or lies below the one before it, and
 *        edges[bins] - edges[0] not positive and finite.  One host synchronisation.  The rule is pa_uniform_bin
 *        (csrc/uniform_bins.h), the one statement of it for this function, its wide form and pa_bin2d_f64, on the device
 *        and on the host; the edge check is pa_check_uniform_edges (csrc/hist_host.cpp), the same for all of them; the
 *        kernel and the host loop are csrc/hist.hip and csrc/hist_host.cpp.
 *   pa_runcomp_join_host, pa_minmax_f64_host, pa_hist_uniform_f64_host   the same from host arrays into host arrays,
 *        plain loops, the same bits.
 *   pa_write_pairs_tsv       (host) `header` and a newline, then n lines repr(x) TAB repr(y) with Python's
 *        float.__repr__: what f"{x}\t{y}\n" writes for two Python floats. */
PA_API int pa_runcomp_join(pa_ctx *ctx, const double *d_ref, uint32_t n_ref, const uint32_t *d_q, const uint32_t *d_s, const double *d_y,
                           uint64_t n_rows, double *d_x, double *d_y_out, double *d_diff, uint64_t *n_common);
PA_API int pa_minmax_f64(pa_ctx *ctx, const double *d_v, uint64_t n, double *out, uint64_t *n_valid);
PA_API int pa_hist_uniform_f64(pa_ctx *ctx, const double *d_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts);
PA_API int pa_runcomp_join_host(const double *h_ref, uint32_t n_ref, const uint32_t *h_q, const uint32_t *h_s, const double *h_y,
                                uint64_t n_rows, double *h_x, double *h_y_out, double *h_diff, uint64_t *n_common);
PA_API int pa_minmax_f64_host(const double *h_v, uint64_t n, double *out, uint64_t *n_valid);
PA_API int pa_hist_uniform_f64_host(const double *h_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts);
PA_API int pa_write_pairs_tsv(const char *path, const char *header, const double *h_x, const double *h_y, uint64_t n);

/* ---- plot-run: score distributions ----
 * What the reference's plot_distribution (pyani_plus/plot_run.py:153-215) has seaborn compute from all N^2 cells of a
 * score matrix: the order statistics numpy's automatic bin rule needs, the moments behind Scott's bandwidth, scipy's
 * gaussian_kde on a grid, and numpy.histogram's counts for the many bins the automatic rule can ask for.  v is a
 * vector of n doubles; NaN means no value and is skipped everywhere.
 *
 *   pa_select_f64            (device) h_out[r] = the element at zero-based rank h_ranks[r] of the non-NaN elements of
 *        d_v[n] in ascending order of value, for up to PA_SELECT_MAX_RANKS ranks in any order, repeats allowed: the value
 *        numpy.sort(v)[rank] has (when -0.0 and 0.0 both occur, which of the two comes back is not defined).  An MSB
 *        radix select over order-preserving u64 keys, a byte a pass, all ranks in the same eight passes; integer
 *        counters only, no sort and no copy of the data; one host synchronisation per pass.  PA_E_INVALID for
 *        n_ranks > PA_SELECT_MAX_RANKS, for a rank >= the number of non-NaN elements (so for every rank when there is
 *        none) and for n >= 2^40; n_ranks = 0 is valid and does nothing.
 *   pa_moments_f64           (device) out[0] = the mean of the non-NaN elements, out[1] = the sum of their squared
 *        deviations from it, in two passes (the mean first); without such an element out is untouched.  A fixed
 *        reduction tree whose shape depends on n alone, no floating-point atomics: two runs give the same bits.  The
 *        host twin adds in index order, so the two agree to rounding, not in bits.  One host synchronisation.
 *   pa_kde_gauss_f64         (device) h_density[j] = 1 / (m bw sqrt(2 pi)) * sum over the m non-NaN elements of
 *        exp(-0.5 ((h_grid[j] - v_i) / bw)^2) for n_grid <= 1024 grid points: scipy's gaussian_kde(v)(grid) when bw is
 *        Scott's factor times the standard deviation.  The quotient is the correctly rounded one, the exponent the
 *        library's exp of a double.  A run of at most PA_KDE_CHAIN additions (the c of DESIGN.md section 7e) one after the other, then a fixed binary
 *        tree over the partial sums, no floating-point atomics: the same bits run to run; the terms are non-negative, so
 *        the sum's relative error is at most (PA_KDE_CHAIN + the tree's depth) * 2^-53.  PA_E_INVALID for n_grid outside
 *        1 .. 1024, a grid point that is not finite, bw that is not positive and finite, an infinite element and no
 *        non-NaN element.
 *   pa_hist_uniform_f64_wide (device) pa_hist_uniform_f64 with another limit, 1 .. 2^20 bins: the same function
 *        (csrc/hist.hip), which chooses by the number of bins: edges and counters in LDS up to 1024 bins, counters in
 *        LDS up to PA_HIST_WIDE_LDS_BINS bins, 64-bit integer atomics on the counters in global memory above.  The
 *        same errors as pa_hist_uniform_f64, with this range of bins.
 *   pa_select_f64_host, pa_moments_f64_host, pa_kde_gauss_f64_host, pa_hist_uniform_f64_wide_host   the same from host
 *        arrays, plain loops.  The density's sum is kept in a long double.  The histogram takes 1 .. 2^28 bins. */
#define PA_SELECT_MAX_RANKS 8
#define PA_KDE_CHAIN 2048
#define PA_HIST_WIDE_LDS_BINS 8192
PA_API int pa_select_f64(pa_ctx *ctx, const double *d_v, uint64_t n, const uint64_t *h_ranks, uint32_t n_ranks, double *h_out);
PA_API int pa_moments_f64(pa_ctx *ctx, const double *d_v, uint64_t n, double *out);
PA_API int pa_kde_gauss_f64(pa_ctx *ctx, const double *d_v, uint64_t n, const double *h_grid, uint32_t n_grid, double bw, double *h_density);
PA_API int pa_hist_uniform_f64_wide(pa_ctx *ctx, const double *d_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts);
PA_API int pa_select_f64_host(const double *h_v, uint64_t n, const uint64_t *h_ranks, uint32_t n_ranks, double *h_out);
PA_API int pa_moments_f64_host(const double *h_v, uint64_t n, double *out);
PA_API int pa_kde_gauss_f64_host(const double *h_v, uint64_t n, const double *h_grid, uint32_t n_grid, double bw, double *h_density);
PA_API int pa_hist_uniform_f64_wide_host(const double *h_v, uint64_t n, const double *h_edges, uint32_t bins, uint64_t *h_counts);

/* ---- plot-run: scatter figures ----
 * What the reference's plot_scatter (pyani_plus/plot_run.py:218-299) hands seaborn.jointplot as one marker per
 * comparison, restated as a raster over the joint panel: N^2 points (x[t], y[t]), t = 0 .. n - 1, binned into
 * bins_x x bins_y cells; per cell the number of points and the index of the last one, whose colour an overdrawn stack
 * of markers shows.
 *
 *   pa_bin2d_f64             (device) point t counts iff x[t] >= xedges[0] && x[t] <= xedges[bins_x] and the same holds
 *        for y[t] and the y edges (NaN fails).  Its bin on each axis is exactly pa_hist_uniform_f64's: the correctly
 *        rounded division, the rounded multiplication, the clamp to bins - 1 and the two corrections against the edges.
 *        h_counts and h_last are u64[bins_x * bins_y] with cell (ix, iy) at ix * bins_y + iy, numpy.histogram2d's
 *        layout: h_counts = histogram2d(x, y, (xedges, yedges))[0]; h_last = the largest t among the cell's points,
 *        PA_BIN2D_NONE for an empty cell.  One grid-stride pass; a wave first merges the points that share its leading
 *        cell into one update; grids of up to PA_BIN2D_LDS_CELLS cells are counted wholly in LDS, larger ones through
 *        a direct-mapped cache of PA_BIN2D_SLOTS slots in LDS, the slot of a cell being cell % PA_BIN2D_SLOTS: the
 *        first cell to claim a slot in a workgroup keeps it, the other cells of that slot go to 32-bit integer atomics
 *        in global memory.  Sums and maxima of integers only, no floating-point atomics: the same bits run to run and
 *        as the host twin.  One host synchronisation.  PA_E_INVALID, checked before any array is touched: bins_x or
 *        bins_y outside 1 .. PA_BIN2D_MAX_BINS; n >= 2^32 - 1 (a cell holds t + 1 in 32 bits on the device); on either
 *        axis, named in the message, an edge that is not finite or lies below the one before it, and a last edge minus
 *        the first that is not positive and finite.  n = 0 is valid: every cell empty.
 *   pa_bin2d_f64_host        the same from host arrays, one plain loop, the same bits, the same checks. */
#define PA_BIN2D_MAX_BINS 1024
#define PA_BIN2D_LDS_CELLS 4096
#define PA_BIN2D_SLOTS 2048
#define PA_BIN2D_NONE 0xFFFFFFFFFFFFFFFFULL
PA_API int pa_bin2d_f64(pa_ctx *ctx, const double *d_x, const double *d_y, uint64_t n, const double *h_xedges, uint32_t bins_x,
                        const double *h_yedges, uint32_t bins_y, uint64_t *h_counts, uint64_t *h_last);
PA_API int pa_bin2d_f64_host(const double *h_x, const double *h_y, uint64_t n, const double *h_xedges, uint32_t bins_x,
                             const double *h_yedges, uint32_t bins_y, uint64_t *h_counts, uint64_t *h_last);

/* ---- TETRA-hip: tetranucleotide Z-score correlations of all genome pairs ----
 * Replaces nothing in the reference: pyani-plus has no TETRA method.  The definition below is this project's own
 * contract (after Teeling et al. 2004, the TETRA of pyani and JSpecies); it is pinned by an independent restatement in
 * tests/tetra_cases.py, and no bit parity with pyani or JSpecies is claimed.  DESIGN.md section 7g.
 *
 * Windows and counts.  For k = 2, 3, 4 a window starts at arena position p when the mask bits p .. p + k - 1 are all 0
 * (pa_sketch's rule: k valid bases inside one record; separators, non-ACGT residues and padding end windows); it
 * belongs to genome g when genome_start[g] <= p and p + k <= genome_start[g + 1].  The index of a word is
 * sum b_i 4^(k - 1 - i) with A=0 C=1 G=2 T=3, the first base most significant.  F[g] is PA_TETRA_BINS = 336 u64 per
 * genome, forward strand only: [0, 256) tetra-, [256, 320) tri-, [320, 336) dinucleotides.
 *
 * Z-scores (host, from the integers).  C_k[w] = F_k[w] + F_k[rc_k(w)], rc_k reversing the k digits and replacing each
 * digit d by 3 - d.  For w = n1 n2 n3 n4, each step one IEEE double operation: N = C_4[w], L = C_3[n1 n2 n3],
 * R = C_3[n2 n3 n4], M = C_2[n2 n3]; E = (L * R) / M; V = (E * ((M - L) * (M - R))) / (M * M); Z = (N - E) / sqrt(V);
 * Z = 0.0 when M == 0 or V is not > 0.
 *
 * Unit rows.  mean = (Z[0] + ... + Z[255], added in this order) / 256; d = Z - mean; ss = the sum of d * d in this order,
 * each product rounded before it is added (no FMA); U = d / sqrt(ss).  ss == 0 (a genome without a window, or one
 * like ACGT alone whose every Z is 0): the genome is degenerate and its U is all NaN.
 *
 * Correlation.  acc = acc + U_a[k] * U_b[k] for k = 0 .. 255 ascending, one accumulator per pair, the product rounded
 * before the addition; r = min(1, max(-1, acc)); exactly 1.0 where a and b are the same genome index; NaN where either
 * genome is degenerate.  r(a, b) and r(b, a) have the same bits.
 *
 *   pa_tetra_counts        (device) d_counts[n_genomes][336] from an arena as pa_sketch takes it (d_dirty may be NULL:
 *        the bitmap is then built into a buffer of the context).  One pass over the packed bases; the mask is read only
 *        for the blocks the dirty bitmap flags and for each genome's first and last block.  Integer sums: the same
 *        counts run to run.  Zeroes d_counts itself; one host synchronisation.
 *   pa_tetra_counts_host   the same from a host arena, one rolling loop per genome on n_threads host threads (0: as many
 *        as the process may use).
 *   pa_tetra_zscores_host  h_counts[n][336] -> h_Z[n][256] and h_U[n][256] as above.  There is no device form.
 *   pa_tetra_corr          (device) d_U[n][256] -> d_out[q1 - q0][s1 - s0], r of genome q0 + i with genome s0 + j.
 *        symmetric != 0 needs q0 == s0 and q1 == s1 (PA_E_INVALID otherwise): only the tiles on and above the diagonal
 *        are evaluated and the rest is mirrored.  64 x 64 pairs per workgroup, register-tiled vector arithmetic, no
 *        atomics.  Allocates nothing, does not synchronise, runs on the context's stream.
 *   pa_tetra_corr_host     the same from host arrays, the same bits.
 *   pa_append_identity_json  pa_append_comparisons_json for a method without coverage: the same rows with
 *        "cov_query": null in every one, "identity": null where is_null. */
#define PA_TETRA_BINS 336
#define PA_TETRA_WORDS 256 /* columns of a Z-score row and of a unit row */
PA_API int pa_tetra_counts(pa_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_mask, const uint64_t *d_dirty, uint64_t arena_bases,
                           const uint64_t *h_genome_start, uint32_t n_genomes, uint64_t *d_counts);
PA_API int pa_tetra_counts_host(const uint32_t *h_packed, const uint32_t *h_mask, uint64_t arena_bases, const uint64_t *h_genome_start,
                                uint32_t n_genomes, uint64_t *h_counts, uint32_t n_threads);
PA_API int pa_tetra_zscores_host(const uint64_t *h_counts, uint32_t n_genomes, double *h_Z, double *h_U);
PA_API int pa_tetra_corr(pa_ctx *ctx, const double *d_U, uint32_t n, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, int symmetric,
                         double *d_out);
PA_API int pa_tetra_corr_host(const double *h_U, uint32_t n, uint32_t q0, uint32_t q1, uint32_t s0, uint32_t s1, int symmetric,
                              double *h_out, uint32_t n_threads);
PA_API int pa_append_identity_json(const char *path, const char *suffix, int file_has_rows, const char *const *q_hashes, uint32_t nq,
                                   const char *const *s_hashes, uint32_t ns, const double *identity, const uint8_t *is_null);

/* ---- tree-run: the neighbour-joining tree of a distance matrix ----
 * Replaces nothing in the reference: pyani-plus writes no tree.  The definition below is this project's own contract
 * (canonical neighbour joining, Saitou & Nei 1987 in Studier & Keppler's form); it is pinned by an independent
 * restatement in tests/tree_cases.py, and no parity with any other program is claimed.  DESIGN.md section 7h.
 *
 * Input.  D, n x n f64 row-major: finite, >= 0, bitwise symmetric, zero diagonal; 1 <= n <= 65535.  Otherwise
 * PA_E_INVALID, and pa_last_error() names the first offending cell in row-major order as D[i,j].
 * Node ids.  Leaves 0 .. n - 1; the node made by join t (t = 0, 1, ...) is n + t.
 * Set-up.  r[i] = D[i, 0] + ... + D[i, n - 1], added in this order into one accumulator; m = n live nodes.
 * While m > 2, every step one IEEE double operation (no FMA):
 *   score of a live pair with ids lo < hi   q = ((double)(m - 2) * d(lo, hi) - r[lo]) - r[hi];
 *   choice   the pair with the smallest q; among equal q (== on doubles: -0.0 ties with 0.0) the smallest lo, then the
 *            smallest hi.  Ties go by node id, not by where a node is stored: the storage layout is free;
 *   join     d = d(lo, hi); len_lo = 0.5 * d + (r[lo] - r[hi]) / (2.0 * (double)(m - 2)); len_hi = d - len_lo;
 *            negative lengths are kept as they come; the record of join t is (lo, hi, len_lo, len_hi);
 *   new node u   for every other live k: d(u, k) = 0.5 * ((d(lo, k) + d(hi, k)) - d);
 *            r[k] = ((r[k] - d(lo, k)) - d(hi, k)) + d(u, k); r[u] = 0.5 * ((r[lo] + r[hi]) - (double)m * d); m -= 1.
 * When m = 2 the two remaining nodes a < b and d(a, b) are the last edge.  n = 2: no join, the last edge is
 * (0, 1, D[0, 1]); n = 1: no join and no edge, nothing is written.  Distances so large that a score overflows are
 * outside the contract (every access stays in bounds; the tree is what IEEE arithmetic gives).
 * Outputs (host).  child[2 (n - 2)] u32 and len[2 (n - 2)] f64: join t is child[2t] = lo, child[2t + 1] = hi with
 * len[2t], len[2t + 1]; last[2] = (a, b) and *last_len.
 *
 *   pa_nj        (device) d_D is device memory and is overwritten as workspace; the other workspace is the context's.
 *        Three launches per join on the context's stream (scan of the live pairs, choice and record, update), enqueued
 *        without a host round trip; one read-back for the check's count and one at the end for the join table.  Integer
 *        atomics in the check only, no floating-point atomics: the same bits run to run and as the host twin.
 *   pa_nj_host   the same from a host matrix, which it does not modify (it works on a copy; PA_E_NOMEM when that cannot
 *        be made); the scan runs on n_threads host threads (0: as many as the process may use) and the result does not
 *        depend on their number. */
PA_API int pa_nj(pa_ctx *ctx, double *d_D, uint32_t n, uint32_t *h_child, double *h_len, uint32_t *h_last, double *h_last_len);
PA_API int pa_nj_host(const double *h_D, uint32_t n, uint32_t *h_child, double *h_len, uint32_t *h_last, double *h_last_len,
                      uint32_t n_threads);

/* ---- bootstrap-run: column-bootstrap support of a run's neighbour-joining tree ----
 * Replaces nothing in the reference: pyani-plus writes no tree and no support.  The definitions below are this project's
 * own contract (Felsenstein's bootstrap over the columns of the alignment of an external-alignment-hip run), pinned by an
 * independent restatement in tests/bootstrap_cases.py.  DESIGN.md section 7l.
 *
 * Weights.  fin is the splitmix64 finaliser of mantel-run-comp.  Replicate r of `seed` over L = n_cols columns has
 * base = fin(fin(seed) + r); its draw t = 0 .. L - 1 hits column mulhi64(fin(base + t), L), the high 64 bits of the
 * 128-bit product; w_r[c] is the number of hits on column c, a uint8.
 * Counts.  Per replicate and ordered pair of rows, over the columns c: M = sum of w[c] where q_c == s_c and q_c != '-',
 * B = sum of w[c] where q_c != '-' and s_c != '-'; the diagonal included, so B[i, i] is row i's weighted residue count
 * n_i.  Integers, at most L < 2^32.
 * Distances.  aln = n_i + n_j - B[i, j]; D[i, j] = 1.0 - (double)M[i, j] / (double)aln, `missing` when aln is 0, 0.0 for
 * i == j: one division and one subtraction, no FMA.
 * Support.  A join table (pa_nj) is an unrooted tree.  The clade of an edge is the set of leaves on its side away from
 * leaf 0; it is trivial with fewer than 2 or more than n - 2 leaves.  Node n + t stands for the edge above it: the edge
 * to the node whose join takes it, and the last edge for the last node made.  Its support is the number of replicate
 * trees that have an edge with the same clade (equal as sets); a trivial clade is in every tree, so its support is n_reps.
 *
 *   pa_msa_boot_weights        (host) rows first .. first + count - 1 of the weights of `seed`: count x n_cols uint8.  A
 *        row depends on (seed, n_cols, its number) alone.  PA_E_INVALID, naming the replicate and the column, for a
 *        weight that would pass 255.
 *   pa_msa_boot_counts         (device) d_planes as pa_msa_pack made them for n_rows rows; h_weights: n_reps x n_cols
 *        uint8 on the host, every row adding up to n_cols (else PA_E_INVALID naming the row).  d_match, d_both:
 *        n_reps x n_rows x n_rows uint32, replicate after replicate.  Only the 64 x 64 tiles on and above the diagonal are
 *        evaluated and the rest mirrored.  Up to PA_MSA_BOOT_BATCH replicates go into one launch; a call may hold more.
 *        The call returns when the stream has finished.
 *   pa_msa_boot_counts_host    the same from the rows as bytes (n_rows rows of row_stride >= n_cols bytes, as
 *        pa_msa_copy_rows lays them out) on n_threads host threads (0: as many as the process may use).
 *   pa_msa_boot_distances      (device) counts -> D, n_reps x n x n f64 on the device, replicate after replicate, each
 *        ready for pa_nj as it is.  `missing` finite and >= 0.
 *   pa_msa_boot_distances_host the same on the host, with the same bits.
 *   pa_tree_support            (host) h_ref_child: the child table of the reference tree, 2 (n - 2) uint32;
 *        h_rep_child: those of n_reps replicate trees, one after the other; h_support: n - 2 uint32, entry t for node
 *        n + t.  4 <= n <= 65535.  Day's algorithm: O(n) per tree, exact.  PA_E_INVALID for a table that is no tree. */
#define PA_MSA_BOOT_BATCH 32 /* replicates the device takes per launch; shows in no result */
PA_API int pa_msa_boot_weights(uint64_t seed, uint64_t n_cols, uint64_t first, uint64_t count, uint8_t *h_weights);
PA_API int pa_msa_boot_counts(pa_ctx *ctx, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, uint32_t bits, const uint8_t *h_weights,
                              uint32_t n_reps, uint32_t *d_match, uint32_t *d_both);
PA_API int pa_msa_boot_counts_host(const uint8_t *h_rows, uint64_t row_stride, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights,
                                   uint32_t n_reps, uint32_t *h_match, uint32_t *h_both, uint32_t n_threads);
PA_API int pa_msa_boot_distances(pa_ctx *ctx, const uint32_t *d_match, const uint32_t *d_both, uint32_t n, uint32_t n_reps, double missing,
                                 double *d_D);
PA_API int pa_msa_boot_distances_host(const uint32_t *h_match, const uint32_t *h_both, uint32_t n, uint32_t n_reps, double missing, double *h_D,
                                      uint32_t n_threads);
PA_API int pa_tree_support(uint32_t n, const uint32_t *h_ref_child, uint32_t n_reps, const uint32_t *h_rep_child, uint32_t *h_support);

/* ---- phylo-run: substitution distances (p, JC69, K80) of an alignment's rows, their tree and its bootstrap ----
 * Replaces nothing in the reference: pyani-plus has no substitution distance.  The definitions below are this project's
 * own contract, pinned by an independent restatement in tests/subst_cases.py.  DESIGN.md section 7m.
 *
 * Code.  A a -> 4, G g -> 5, C c -> 6, T t U u -> 7, every other byte ('-' and the IUPAC letters included) -> 0: bit 2
 * "is a nucleotide", bit 1 the class (0 purine, 1 pyrimidine), bit 0 the base within the class.  pa_subst_code writes
 * the 256 codes; pa_msa_pack takes them with bits = PA_SUBST_BITS.
 * Counts.  For rows i, j and column weights w_c (all 1 without weights): V = sum of w_c over the columns where both
 * rows are nucleotides, S = the sum over those of them where the classes are equal and the bases differ (transitions),
 * T = the sum over those where the classes differ (transversions).  Symmetric; V[i, i] is row i's weighted nucleotide
 * count and S = T = 0 there.  uint32: n_cols < 2^32 and a replicate's weights add up to n_cols.
 * Distance (csrc/subst_rule.h, every operation rounded on its own, no FMA).  i == j: 0.0.  V == 0: `missing`.
 * S + T == 0: +0.0.  p: (double)(S + T) / (double)V.  jc69: a = 1.0 - (4.0 * (double)(S + T)) / (3.0 * (double)V);
 * d = -0.75 * L(a).  k80: P = (double)S / (double)V; Q = (double)T / (double)V; a = (1.0 - 2.0 * P) - Q;
 * b = 1.0 - 2.0 * Q; d = -0.5 * L(a) - 0.25 * L(b).  a <= 0 or b <= 0: `missing` (the pair is saturated).  L is the
 * natural logarithm written out from + - * / and integer operations on the exponent: the same bits on host and device,
 * within 1 ulp of the correctly rounded logarithm on the samples of tests/test_subst_host.py.
 *
 *   pa_subst_code            (host) h_code256[b] = the code of byte b.
 *   pa_msa_subst_counts      (device) d_planes as pa_msa_pack made them from pa_subst_code's table at PA_SUBST_BITS for
 *        n_rows <= 65535 rows.  h_weights NULL: every column once, n_reps must be 1; otherwise n_reps x n_cols uint8 on
 *        the host, every row adding up to n_cols (else PA_E_INVALID naming the row), up to PA_MSA_BOOT_BATCH replicates
 *        a launch.  d_valid, d_ts, d_tv: n_reps x n_rows x n_rows uint32, replicate after replicate.  Only the 64 x 64
 *        tiles on and above the diagonal are evaluated and the rest mirrored.  n_cols == 0: all counts zero.  The call
 *        returns when the stream has finished.
 *   pa_msa_subst_counts_host the same from the rows as bytes (n_rows rows of row_stride >= n_cols bytes) on n_threads
 *        host threads (0: as many as the process may use).
 *   pa_subst_distances       (device) counts -> D, n_reps x n x n f64 on the device, each ready for pa_nj as it is;
 *        h_undefined: per matrix two uint64 on the host, the unordered pairs that are `missing` for V == 0 and those
 *        that are for saturation.  model: PA_SUBST_MODEL_*; `missing` finite and >= 0.
 *   pa_subst_distances_host  the same on the host, with the same bits.
 *   pa_subst_log_host        h_out[i] = L(h_x[i]), for the accuracy test. */
#define PA_SUBST_BITS 3
#define PA_SUBST_MODEL_P 0
#define PA_SUBST_MODEL_JC69 1
#define PA_SUBST_MODEL_K80 2
PA_API int pa_subst_code(uint8_t *h_code256);
PA_API int pa_msa_subst_counts(pa_ctx *ctx, const uint32_t *d_planes, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights, uint32_t n_reps,
                               uint32_t *d_valid, uint32_t *d_ts, uint32_t *d_tv);
PA_API int pa_msa_subst_counts_host(const uint8_t *h_rows, uint64_t row_stride, uint32_t n_rows, uint64_t n_cols, const uint8_t *h_weights,
                                    uint32_t n_reps, uint32_t *h_valid, uint32_t *h_ts, uint32_t *h_tv, uint32_t n_threads);
PA_API int pa_subst_distances(pa_ctx *ctx, const uint32_t *d_valid, const uint32_t *d_ts, const uint32_t *d_tv, uint32_t n, uint32_t n_reps,
                              int model, double missing, double *d_D, uint64_t *h_undefined);
PA_API int pa_subst_distances_host(const uint32_t *h_valid, const uint32_t *h_ts, const uint32_t *h_tv, uint32_t n, uint32_t n_reps, int model,
                                   double missing, double *h_D, uint64_t *h_undefined, uint32_t n_threads);
PA_API int pa_subst_log_host(const double *h_x, uint64_t n, double *h_out);

/* ---- ordinate-run: principal coordinates (classical scaling) of a distance matrix ----
 * Replaces nothing in the reference: pyani-plus writes no ordination.  The definitions below are this project's own
 * contract, pinned by an independent restatement in tests/pcoa_cases.py; no parity with any other program is claimed.
 * DESIGN.md section 7i.  Every step is one IEEE double operation (no FMA), no floating-point atomics: a device entry
 * point gives the same bits run to run and the same bits as its host twin, and a host twin's result does not depend on
 * n_threads (0: as many as the process may use).  pcoa_rule.h states the constants and formulas once for both.
 *
 *   pa_mul_tall_f64   Y = A Q.  A is n x n, Q and Y are n x p, all f64 row-major; 1 <= n <= 65535, 1 <= p <= 32
 *        (PA_E_INVALID otherwise).  The order of the additions is part of the contract.  The columns j of a row are cut
 *        into chunks of pcoa::kChunk = 256 (pcoa_rule.h states it; the last chunk may be short).  Within chunk b,
 *        s_b = ((A[i,j0] Q[j0,c] + A[i,j0+1] Q[j0+1,c]) + ...) in ascending j, every product rounded, one accumulator
 *        that starts from the first product; Y[i,c] = ((s_0 + s_1) + ...) in ascending b, starting from s_0.
 *        Device: d_A, d_Q, d_Y are device memory, none overlapping; one launch over (128-row tile x chunk) writes the
 *        partial sums to the context's workspace (n p ceil(n / 256) doubles), a second adds them; a lane owns its
 *        outputs, so the tiling does not show in a sum.  No host synchronisation.
 *   pa_gower_center   B = the doubly centred matrix of the squared distances.  D as for pa_nj: n x n f64, finite,
 *        >= 0, bitwise symmetric, zero diagonal, 1 <= n <= 65535; otherwise PA_E_INVALID and pa_last_error() names the
 *        first offending cell in row-major order as D[i,j].  a[i,j] = D[i,j] * D[i,j];
 *        r[i] = (a[i,0] + ... + a[i,n-1]) / n, added in ascending order into one accumulator that starts from a[i,0];
 *        g = (r[0] + ... + r[n-1]) / n likewise; B[i,j] = -0.5 * ((a[i,j] - (r[i] + r[j])) + g), which makes B bitwise
 *        symmetric; *h_trace = B[0,0] + B[1,1] + ...; *h_fro2 = the sum over ascending i of the rows' sums over
 *        ascending j of B[i,j] * B[i,j].  d_B (n x n) must not overlap d_D.  Two host synchronisations (the check, the
 *        two scalars).
 *   pa_symm_top_eigs  the k algebraically largest eigenvalues of the symmetric n x n matrix B, 1 <= k <= min(n, 24), in
 *        descending order (h_values[k]), their unit eigenvectors as the columns of h_vectors (n x k row-major), each
 *        pair's residual norm ||B v - lambda v||_2 (h_residuals[k]) and h_info[3] = (iterations of phase 1, iterations
 *        in all, the shift used).  Block subspace iteration with Rayleigh-Ritz, block width
 *        p = min(n, max(2k, k + 8), 32): the product's limit caps it, which at k = 24 still leaves k + 8 columns.
 *        The start block is pcoa::start_value(i * p + c) (a fixed 64-bit integer mix mapped to (-1, 1)),
 *        orthonormalised.  An iteration: Y = B Q by pa_mul_tall_f64, Y += sigma Q; H = Q^T Y, symmetrised as
 *        0.5 (H + H^T); its eigen-decomposition H = S diag(theta) S^T by cyclic Jacobi; theta sorted descending,
 *        lambda = theta - sigma; X = Q S; R = Y S - X diag(theta).  A pair has converged when
 *        ||R_c||_2 <= tol * max|lambda|, the maximum over the p Ritz values.  The next Q is Y orthonormalised by
 *        twice-applied modified Gram-Schmidt (a column that vanishes is replaced by a fresh one).
 *        Phase 1 runs with sigma = 0 until the first k pairs have converged, 200 iterations at most.  With
 *        rho = sqrt(max(fro2 - sum of lambda_c^2 over the converged pairs among the first k, 0)) every other eigenvalue
 *        of B has magnitude <= rho: when all k have converged and lambda_k > rho the result is certified and returned
 *        (shift 0).  Otherwise phase 2 goes on with sigma = rho (B + sigma I has no negative eigenvalue outside the
 *        converged pairs, so the largest in magnitude are the largest) until the first k pairs have converged: from
 *        the current block when phase 1 ended at its cap; when it ended with all k converged the block spans an
 *        invariant subspace, which no product leads out of, so its first k Ritz vectors are kept and the other
 *        p - k columns start again from fresh start values.  fro2 is the squared Frobenius norm of B (pa_gower_center's).  After max_iter iterations in
 *        all (>= 1) without convergence the call returns PA_E_NOCONVERGE, the message names the iteration count and the
 *        worst residual, and the outputs are left untouched.  Sign: each vector is scaled by +-1 so that its entry of
 *        largest magnitude, the first such in index order, is positive.  tol must be finite and > 0 (1e-10 is the
 *        callers' default).
 *        Everything but the product is p-wide algebra on one host thread, the same compiled code for both entry
 *        points.  Device: d_B is device memory and is only read; Q goes up and Y comes down once per iteration.  Host
 *        twin: the product runs on n_threads. */
#define PA_MUL_TALL_MAX_P 32 /* pa_mul_tall_f64: columns of the thin block, at most */
#define PA_EIGS_MAX_K 24     /* pa_symm_top_eigs: eigenpairs, at most */
PA_API int pa_mul_tall_f64(pa_ctx *ctx, const double *d_A, uint32_t n, const double *d_Q, uint32_t p, double *d_Y);
PA_API int pa_mul_tall_f64_host(const double *h_A, uint32_t n, const double *h_Q, uint32_t p, double *h_Y, uint32_t n_threads);
PA_API int pa_gower_center(pa_ctx *ctx, const double *d_D, uint32_t n, double *d_B, double *h_trace, double *h_fro2);
PA_API int pa_gower_center_host(const double *h_D, uint32_t n, double *h_B, double *h_trace, double *h_fro2, uint32_t n_threads);
PA_API int pa_symm_top_eigs(pa_ctx *ctx, const double *d_B, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2,
                            double *h_values, double *h_vectors, double *h_residuals, double *h_info);
PA_API int pa_symm_top_eigs_host(const double *h_B, uint32_t n, uint32_t k, double tol, uint32_t max_iter, double fro2, double *h_values,
                                 double *h_vectors, double *h_residuals, double *h_info, uint32_t n_threads);

/* ---- mantel-run-comp: Mantel's permutation test between two distance matrices ----
 * Replaces nothing in the reference: pyani-plus compares runs with figures only.  The definitions below are this
 * project's own contract, pinned by an independent restatement in tests/mantel_cases.py.  DESIGN.md section 7j.  Every
 * step is one IEEE double operation (no FMA), no floating-point atomics: pa_mantel gives the same bits run to run and the
 * same bits as pa_mantel_host, whose result does not depend on n_threads (0: as many as the process may use); neither
 * depends on how the permutations are batched or on how many a call brings.  mantel_rule.h states the constants and
 * formulas once for both.
 *
 *   Inputs.  X and Y are n x n f64 row-major, each as for pa_nj: finite, >= 0, bitwise symmetric, zero diagonal;
 *        3 <= n <= PA_MANTEL_MAX_N (a row of 128 KB, which the device holds in the LDS of one CU; the host twin has the
 *        same limit).  h_perms is n_perms x n u32, every row a permutation of 0 .. n - 1: row q pairs row i of X with
 *        row h_perms[q n + i] of Y.  n_perms = 0 is valid.  Nothing is modified.
 *   tri(T), the sum of the terms T[i,j], j > i.  Row i has PA_MANTEL_LANES = 64 accumulators; a_l takes the terms with
 *        j % 64 == l, j > i, in ascending j, and starts at -0.0 (so the first term enters unchanged and an accumulator
 *        without terms is -0.0).  Then for w = 32, 16, 8, 4, 2, 1: a_l = a_l + a_{l+w} for l < w.  The row's sum is
 *        rho_i = a_0.  tri = (((-0.0 + rho_0) + rho_1) + ...) + rho_{n-1}, one accumulator, ascending i.
 *   Moments.  m = n (n - 1) / 2 as a double; mean_x = tri(X) / m; x[i,j] = X[i,j] - mean_x for i != j;
 *        ss_x = tri(x x), each square rounded.  The same for y.  h_stats[4] = mean_x, mean_y, ss_x, ss_y.
 *   Cross sums.  cross(pi) = tri(T) with T[i,j] = x[i,j] * y[pi[i],pi[j]], each product rounded.  h_cross[n_perms + 1]:
 *        entry 0 is the identity's, entry 1 + q that of row q of h_perms.  Mantel's r of a permutation is
 *        cross / sqrt(ss_x ss_y), which the callers compute.
 *   Checks, in this order, the same code for both entry points: null arguments; the range of n (before anything is
 *        read); every row of h_perms (PA_E_INVALID names the row and the position of the first value that is out of
 *        range or repeated); X, then Y (PA_E_INVALID names the matrix and the first offending cell in row-major order,
 *        "pa_mantel: Y[3,1] ...").  The permutations are checked on the host before the first launch: that is what keeps
 *        the kernel's LDS index inside the row.  A refused call leaves the context usable.
 *   Device: d_X and d_Y are device memory, h_* host memory.  A workgroup holds one centred row of Y in LDS and its waves
 *        gather from it at pi[j] while row pi^-1[r] of X streams past; the identity and the permutations go through the
 *        context's workspace PA_MANTEL_BATCH at a time.  Two host synchronisations (the check, the results).
 *   pa_mantel_permutations  rows first .. first + count - 1 of the permutations of seed `seed` (h_perms: count x n u32,
 *        1 <= n <= PA_MANTEL_MAX_N).  fin(v) is the splitmix64 finaliser: z = v + 0x9E3779B97F4A7C15,
 *        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z ^ (z >> 31), all mod 2^64.
 *        Row q: base = fin(fin(seed) + q); start from 0 .. n - 1; for t = n - 1 down to 1, k = fin(base + t) mod (t + 1),
 *        swap entries t and k.  The modulo prefers small remainders by less than 2^-48; nothing is rejected.  Row q
 *        depends on (seed, n, q) alone.  seed 1, n 5: rows 0, 1, 2 are [2,1,3,4,0], [0,1,2,4,3], [0,1,4,3,2]. */
#define PA_MANTEL_MAX_N 16384
#define PA_MANTEL_LANES 64
#define PA_MANTEL_BATCH 256 /* cross sums the device makes per launch; shows in no result */
PA_API int pa_mantel_permutations(uint64_t seed, uint32_t n, uint64_t first, uint64_t count, uint32_t *h_perms);
PA_API int pa_mantel(pa_ctx *ctx, const double *d_X, const double *d_Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, double *h_stats,
                     double *h_cross);
PA_API int pa_mantel_host(const double *h_X, const double *h_Y, uint32_t n, const uint32_t *h_perms, uint64_t n_perms, double *h_stats,
                          double *h_cross, uint32_t n_threads);

/* ---- dereplicate-run: one representative genome per group of a run's threshold graph ----
 * Replaces nothing in the reference, which has no such command.  The definitions below are this project's own contract,
 * pinned by an independent restatement in tests/derep_cases.py.  DESIGN.md section 7k.  Everything but the scores is
 * integer work and every score is classify's aggregate of two cells, so each device entry point gives the same bits run
 * to run and the same bits as its _host twin, whose result does not depend on n_threads (0: as many as the process may
 * use).  derep_rule.h states the rules once for both.
 *
 *   Nodes.  Node p is row and column p of S (score) and C (query coverage), n x n f64 row-major, rows the query;
 *        1 <= n <= 65535.  A lower index is a preferred genome: the callers order the genomes, this layer knows no other
 *        priority.  Nothing is modified.
 *   Edge.  For lo < hi: score = agg_score(S[hi,lo], S[lo,hi]), cov = agg_cov(C[hi,lo], C[lo,hi]) with the argument order
 *        and NaN behaviour of pa_classify_edges (PA_AGG_MIN, PA_AGG_MAX keep the first argument unless the comparison
 *        with the second holds; PA_AGG_MEAN is (a + b) / 2).  lo and hi are adjacent iff neither value is NaN,
 *        cov > cov_min and score >= min_score: the graph classify has at the moment its min_score column reads that
 *        value.  Every node is adjacent to itself, whatever the diagonal holds.
 *   Bits.  W = ceil(n / 64) uint64_t words per row, row-major: bit b of word w of row a is adjacency(a, 64 w + b).
 *        Symmetric, the diagonal set, the padding bits zero.
 *   pa_derep_select, PA_DEREP_GREEDY: for p = 0 .. n - 1 in order, p is a representative iff no earlier representative
 *        is adjacent to it (the lexicographically first maximal independent set).  PA_DEREP_COVER: start with every node
 *        uncovered; while one is, gain(p) = uncovered nodes in p's closed neighbourhood; choose the largest gain, among
 *        equal gains a p that is itself uncovered, then the smaller p; its closed neighbourhood is covered.  (Once the
 *        largest gain is 1, exactly the nodes still uncovered become representatives.)  is_rep[n] is 1 or 0,
 *        *n_reps their number.  The device runs rounds of small launches, PA_DEREP_BATCH of them between two looks at a
 *        device scalar that makes the rest return at once when nothing is left; *n_rounds (nullable, device entry only)
 *        is the number of rounds that had work: a diagnostic, not part of the contract.
 *   pa_derep_assign.  rep[p] = p for a representative; otherwise the adjacent representative with the largest
 *        score(p, r), equal scores (== on doubles) to the smaller r; rep_score[p] is that score, for a representative the
 *        score of the pair (p, p) by the same formula.  Both modes guarantee an adjacent representative; with an is_rep
 *        that offers none (or only NaN scores) rep[p] = PA_DEREP_NONE and rep_score[p] = NaN.  Bits of is_rep at or past
 *        n are never read.
 *   Checks, the same code and messages for both forms: n = 0 or n > 65535; null arguments; an unknown aggregator or
 *        mode; a NaN min_score or cov_min: PA_E_INVALID.
 *   Device: every pointer but n_reps and n_rounds is device memory.  No grid-wide barrier, no floating-point atomics;
 *        one read-back per batch of rounds. */
#define PA_DEREP_GREEDY 0
#define PA_DEREP_COVER 1
#define PA_DEREP_BATCH 64 /* rounds the device enqueues between two read-backs; shows in no result */
#define PA_DEREP_NONE 0xFFFFFFFFu
PA_API int pa_derep_adjacency(pa_ctx *ctx, const double *d_S, const double *d_C, uint32_t n, int agg_score, int agg_cov, double min_score,
                              double cov_min, uint64_t *d_bits);
PA_API int pa_derep_adjacency_host(const double *h_S, const double *h_C, uint32_t n, int agg_score, int agg_cov, double min_score, double cov_min,
                                   uint64_t *h_bits, uint32_t n_threads);
PA_API int pa_derep_select(pa_ctx *ctx, const uint64_t *d_bits, uint32_t n, int mode, uint8_t *d_is_rep, uint32_t *n_reps, uint32_t *n_rounds);
PA_API int pa_derep_select_host(const uint64_t *h_bits, uint32_t n, int mode, uint8_t *h_is_rep, uint32_t *n_reps);
PA_API int pa_derep_assign(pa_ctx *ctx, const double *d_S, uint32_t n, int agg_score, const uint64_t *d_bits, const uint8_t *d_is_rep,
                           uint32_t *d_rep, double *d_rep_score);
PA_API int pa_derep_assign_host(const double *h_S, uint32_t n, int agg_score, const uint64_t *h_bits, const uint8_t *h_is_rep, uint32_t *h_rep,
                                double *h_rep_score, uint32_t n_threads);

/* ---- search-run: for new genomes, the nearest genomes of a run ----
 * Replaces nothing in the reference, which has no such command.  The definitions below are this project's own contract,
 * pinned by an independent restatement in tests/search_cases.py.  DESIGN.md section 7n.  Integer work only: the device
 * entry point gives the same bits run to run and the same bits as its _host twin, whose result does not depend on
 * n_threads (0: as many as the process may use).  hits_rule.h states the order once for both.
 *
 *   Input.  counts[q * ld + c] = I = |S_q n S_s| of query q < nq and column c < ns of this tile of subjects, the layout
 *        pa_pair_counts writes (ld = the tile's width there, ld >= ns); q_size[nq] and s_size[ns] the sketch sizes,
 *        1 to 2^32 - 1 each (the twin refuses a 0, the device call does not look).  Column c is subject s_base + c;
 *        s_base + ns < PA_HITS_NONE.  Nothing of the input is modified.
 *   Hit.  A column with I > 0 (I = 0 is the reference's NULL, no hit), with the denominator m = min(|Q|, |S|) under
 *        PA_HITS_RANK_IDENTITY -- (I / m)^(1/k) is the larger of the two containments, the sourmash identity -- and
 *        m = |Q| under PA_HITS_RANK_CONTAINMENT.
 *   Order.  Hit a comes before hit b when I_a m_b > I_b m_a as exact 64-bit products; when these are equal, I_a > I_b;
 *        then the lower subject index.  A strict total order: a query's `top` best hits are unique and do not depend on
 *        how the subjects are cut into tiles.
 *   Output.  Three arrays of nq x top, best first: the subject's index, I and m; a missing rank holds PA_HITS_NONE, 0, 0.
 *        With accumulate != 0 the three arrays are inputs as well: the lists so far compete with this tile's columns under
 *        the same order (the stored m is what makes that possible without the earlier tiles' sizes).  The tiles of one
 *        accumulation must not overlap; this is not checked.  nq == 0 or ns == 0 is a valid call: without accumulate it
 *        writes the empty lists.
 *   Checks, the same code and messages for both forms, PA_E_INVALID: top outside 1 .. PA_HITS_MAX_TOP; an unknown rank;
 *        ld < ns; index overflow (s_base + ns, or nq * ld * 4 bytes past 64 bits); a null pointer to an array that has
 *        elements, named in the message.
 *   Device: every pointer is device memory; one launch on the context's stream, no synchronisation, no workspace. */
#define PA_HITS_MAX_TOP 64
#define PA_HITS_NONE 0xFFFFFFFFu
#define PA_HITS_RANK_IDENTITY 0
#define PA_HITS_RANK_CONTAINMENT 1
PA_API int pa_best_hits(pa_ctx *ctx, const uint32_t *d_counts, uint32_t nq, uint32_t ns, uint64_t ld, const uint32_t *d_q_size,
                        const uint32_t *d_s_size, uint32_t s_base, int rank, uint32_t top, int accumulate, uint32_t *d_hit_subject,
                        uint32_t *d_hit_shared, uint32_t *d_hit_denom);
PA_API int pa_best_hits_host(const uint32_t *h_counts, uint32_t nq, uint32_t ns, uint64_t ld, const uint32_t *h_q_size,
                             const uint32_t *h_s_size, uint32_t s_base, int rank, uint32_t top, int accumulate, uint32_t *h_hit_subject,
                             uint32_t *h_hit_shared, uint32_t *h_hit_denom, uint32_t n_threads);

/* ---- in-library HIP-event timing of the kernels (bench.py roofline) ----
 * Phases are timed with hipEvents on the context's stream when enabled. */
#define PA_PROF_KMER_HASH 0   /* k-mer hash + threshold filter kernel */
#define PA_PROF_SKETCH_SORT 1 /* radix sort + unique of candidates */
#define PA_PROF_PAIR_DICT 2   /* dictionary sort + ids + bit-row build */
#define PA_PROF_PAIR_COUNT 3  /* bit-row column-sum / merge kernel */
#define PA_PROF_ANI 4
#define PA_PROF_FRAG_INDEX 5 /* fragment ANI: minimizers, hash dictionary, postings */
#define PA_PROF_FRAG_SEED 6  /* fragment ANI: fragment sketches, seed hits bucketed by reference genome */
#define PA_PROF_FRAG_MAP 7   /* fragment ANI: prefilter + map_segments_kernel + per-pair reduction */
#define PA_PROF_MSA_PACK 8    /* external alignment: rows -> bit planes (msa_pack_kernel) */
#define PA_PROF_MSA_PAIRS 9   /* external alignment: pair counts M, B (msa_pairs_kernel, mirror); phylo-run: the counts V, S, T, weighted or not (subst_pairs_kernel, subst_boot_pairs_kernel, mirror) */
#define PA_PROF_CLS_EDGES 10  /* classify: pair evaluation, counts, scan, compaction (cls_edges_kernel) */
#define PA_PROF_CLS_SORT 11   /* classify: radix sort of the edges by score + gather */
#define PA_PROF_ROWDIST 12   /* plot-run: all-pairs row distances (rowdist_euclid_kernel) */
#define PA_PROF_NJ_SCAN 13   /* tree-run: the scan of the live pairs before each join (nj_scan_kernel) */
#define PA_PROF_NJ_JOIN 14   /* tree-run: the choice among the tiles' candidates and the record (nj_join_kernel) */
#define PA_PROF_NJ_UPDATE 15 /* tree-run: the new node's row and column, the row sums, the swap-remove (nj_update_kernel) */
#define PA_PROF_MSA_BOOT 16      /* bootstrap-run: weight planes, weighted pair counts, mirror (msa_boot_pairs_kernel) */
#define PA_PROF_MSA_BOOT_DIST 17 /* bootstrap-run: counts -> distances (msa_boot_distances_kernel); phylo-run: the same (subst_distances_kernel) */
#define PA_PROF_NPHASES 18
PA_API int pa_prof_enable(pa_ctx *ctx, int on);
PA_API int pa_prof_reset(pa_ctx *ctx);
/* total milliseconds and number of timed launches of a phase (syncs the stream) */
PA_API int pa_prof_get(pa_ctx *ctx, int phase, double *total_ms, uint64_t *launches);

/* ---- probes of the internal device primitives: libpyani_hip_tools.so (-DPA_TOOLS) only ----
 * Not part of the ABI (PA_ABI_VERSION does not count them) and absent from libpyani_hip.so: they let
 * tests/test_gpu_sort_scan.py call the radix sort and the exclusive scan of radix_sort.hip -- the one object both
 * libraries link -- directly, on the context's stream, without waiting for it.
 *   pa_tool_radix_sort_pairs   stable LSD radix sort of n (u64 key, u32 value) pairs on bits [bit_lo, bit_hi) of the
 *        key, or of the value with by_val != 0.  keys0/keys1 and vals0/vals1 are the two halves of the double
 *        buffers, n elements each; *which (0 or 1) names the half that holds the input on entry and the result on
 *        return.  bit_lo >= 0, bit_hi - bit_lo a multiple of 8, bit_hi <= 64 (<= 32 with by_val): anything else is
 *        PA_E_INVALID before a launch.  n <= 1 or bit_hi <= bit_lo: nothing is touched.
 *   pa_tool_exclusive_scan_u32 d_out[i] = (d_in[0] + ... + d_in[i - 1]) mod 2^32; d_out may be d_in.  The exact
 *        64-bit sum of all n values goes to *d_total_u64 where that is not null (0 for n = 0). */
#ifdef PA_TOOLS
#define PA_TOOL_API __attribute__((visibility("default")))
PA_TOOL_API int pa_tool_radix_sort_pairs(pa_ctx *ctx, uint64_t *d_keys0, uint64_t *d_keys1, uint32_t *d_vals0,
                                         uint32_t *d_vals1, uint64_t n, int bit_lo, int bit_hi, int by_val, int *which);
PA_TOOL_API int pa_tool_exclusive_scan_u32(pa_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint64_t n,
                                           uint64_t *d_total_u64);
#endif

#ifdef __cplusplus
}
#endif
#endif /* PYANI_HIP_H */
