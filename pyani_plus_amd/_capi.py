"""ctypes binding of ``libpyani_hip.so`` (declared in ``include/pyani_hip.h``).

This is the only route from Python into the compute path.  There is no CPU
fallback: if the shared library is missing, or no gfx950 device is usable,
the calls raise ``HipBackendError``.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "_lib" / "libpyani_hip.so"
# The same sources built with -DPA_TOOLS: the environment switches that force a rare path, cut a kernel short or select an
# ablation variant (PA_MAP_CUT, PA_FRAGANI_*, PA_KMER_*, PA_PAIRS_SYMMETRIC, ...) exist in this build only.  tools/ and
# the tests of those paths load it (``HipEngine(tools=True)``); nothing else does.
TOOLS_LIB_PATH = _PKG / "_lib" / "libpyani_hip_tools.so"

ABI_VERSION = 5
PA_OK = 0
PA_E_INVALID = -1
PA_E_NOMEM = -3
PA_E_CAPACITY = -4
PA_E_IO = -6
PA_E_NOCONVERGE = -7  # pa_symm_top_eigs used up its max_iter
PA_MUL_TALL_MAX_P = 32  # pa_mul_tall_f64: columns of the thin block, at most
PA_EIGS_MAX_K = 24  # pa_symm_top_eigs: eigenpairs, at most
PA_MANTEL_MAX_N = 16384  # pa_mantel, pa_mantel_host: genomes, at most (a 128 KB row)
PA_MANTEL_LANES = 64  # ... accumulators of a row's sum
PA_MANTEL_BATCH = 256  # ... cross sums the device makes per launch; shows in no result
PA_MSA_BOOT_BATCH = 32  # pa_msa_boot_counts: replicates the device takes per launch; shows in no result
PA_DEREP_GREEDY, PA_DEREP_COVER = 0, 1  # pa_derep_select: the modes
PA_DEREP_MODE = {"greedy": PA_DEREP_GREEDY, "cover": PA_DEREP_COVER}
PA_DEREP_BATCH = 64  # ... rounds the device enqueues between two read-backs; shows in no result
PA_DEREP_NONE = 0xFFFFFFFF  # pa_derep_assign: the representative of a node that is adjacent to none
PA_SIG_UNHANDLED = 1
PA_FRAGANI_REUSE_INDEX = 1
PA_FRAGANI_COLUMNS_ONLY = 2
PA_PAIRS_AUTO, PA_PAIRS_BITROW, PA_PAIRS_MERGE, PA_PAIRS_BITROW_HASH = 0, 1, 2, 3
PA_ALIGN_BASES = 64
PA_SELECT_MAX_RANKS = 8
PA_KDE_CHAIN = 2048  # the longest run of sequential additions of pa_kde_gauss_f64 (the c of DESIGN.md section 7e)
PA_HIST_WIDE_LDS_BINS = 8192  # pa_hist_uniform_f64_wide counts in LDS up to this many bins
PA_BIN2D_MAX_BINS = 1024  # pa_bin2d_f64: bins per axis, at most
PA_BIN2D_LDS_CELLS = 4096  # ... counts grids of up to this many cells wholly in LDS
PA_BIN2D_SLOTS = 2048  # ... and larger ones through this many direct-mapped slots: the slot of a cell is cell % PA_BIN2D_SLOTS
PA_BIN2D_NONE = 0xFFFFFFFFFFFFFFFF  # the `last` of an empty cell
PA_TETRA_BINS = 336  # pa_tetra_counts: u64 per genome, 256 tetra-, 64 tri- and 16 dinucleotides
PA_TETRA_WORDS = 256  # columns of a Z-score row and of a unit row
PROF_PHASES = {"kmer_hash": 0, "sketch_sort": 1, "pair_dict": 2, "pair_count": 3, "ani": 4, "frag_index": 5, "frag_seed": 6, "frag_map": 7,
               "msa_pack": 8, "msa_pairs": 9, "cls_edges": 10, "cls_sort": 11, "rowdist": 12, "nj_scan": 13, "nj_join": 14, "nj_update": 15,
               "msa_boot": 16, "msa_boot_dist": 17}
PA_AGG = {"min": 0, "max": 1, "mean": 2}

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); mirrors include/pyani_hip.h one to one
SIGNATURES: dict[str, tuple] = {
    "pa_abi_version": (C.c_int, []),
    "pa_last_error": (C.c_char_p, []),
    "pa_device_count": (C.c_int, []),
    "pa_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "pa_ctx_destroy": (None, [_vp]),
    "pa_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "pa_ctx_own_stream": (C.c_int, [_vp]),
    "pa_ctx_sync": (C.c_int, [_vp]),
    "pa_ctx_device_info": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_int), _u64p]),
    "pa_dev_alloc": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp)]),
    "pa_dev_free": (C.c_int, [_vp, _vp]),
    "pa_memcpy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "pa_memcpy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "pa_memset_d": (C.c_int, [_vp, _vp, C.c_int, C.c_uint64]),
    "pa_pack_bound": (C.c_uint64, [C.c_uint64]),
    "pa_pack_fasta": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, _u64p, _u64p, _u64p]),
    "pa_pack_seq": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, _u64p, _u64p]),
    "pa_max_hash": (C.c_uint64, [C.c_uint64]),
    "pa_fasta_batch_load": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.POINTER(_vp)]),
    "pa_fasta_batch_info": (
        C.c_int,
        [_vp, C.c_uint32, C.c_char_p, _u64p, _u64p, _u64p, _u64p, _u64p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int)],
    ),
    "pa_fasta_batch_records": (C.c_int, [_vp, C.c_uint32, C.POINTER(_u64p), C.POINTER(_u64p), _u64p]),
    "pa_fasta_batch_arena_bases": (C.c_uint64, [_vp]),
    "pa_fasta_batch_copy_arena": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pa_fasta_batch_free": (None, [_vp]),
    "pa_arena_dirty": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "pa_sketch": (
        C.c_int,
        [_vp, _vp, _vp, _vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, C.c_uint64, _vp, C.c_uint64, _vp, _u64p],
    ),
    "pa_read_sigs": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "pa_sig_batch_info": (C.c_int, [_vp, C.c_uint32, _u64p, C.POINTER(C.c_char_p)]),
    "pa_sig_batch_copy": (C.c_int, [_vp, _vp, _vp]),
    "pa_sig_batch_free": (None, [_vp]),
    "pa_write_sigs": (C.c_int, [C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32]),
    "pa_mask_runs": (C.c_int64, [_vp, C.c_uint64, _vp, _vp, C.c_uint64]),
    "pa_mask_from_runs": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64]),
    "pa_sketch_streamed": (
        C.c_int,
        [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _u64p],
    ),
    "pa_pair_counts": (
        C.c_int,
        [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_int],
    ),
    "pa_pair_counts_ex": (
        C.c_int,
        [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_int],
    ),
    "pa_pair_dict_prepare": (C.c_int, [_vp, _vp, C.c_uint64]),
    "pa_ani": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "pa_ani_host": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_int, C.c_uint32]),
    "pa_sketch_bottom": (
        C.c_int,
        [_vp, _vp, _vp, _vp, C.c_uint64, _u64p, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _vp, _u64p],
    ),
    "pa_pair_mash": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    "pa_ani_mash": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp]),
    "pa_fragani": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "pa_fragani_ex": (
        C.c_int,
        [_vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
         C.c_uint32, C.c_uint32, _vp, _vp, _vp],
    ),
    "pa_fragani_sketch": (
        C.c_int,
        [_vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _u64p],
    ),
    "pa_text_ambiguous": (C.c_int64, [_vp, C.c_uint64, C.c_int, _vp, _vp, C.c_uint64]),
    "pa_fasta_batch_ambiguous": (C.c_int64, [_vp, _vp, _vp, C.c_uint64]),
    "pa_fragani_set_ambiguous": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64]),
    "pa_fragani_window": (C.c_int, [C.c_uint32, C.c_uint32]),
    "pa_fragani_workspace": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "pa_fragani_set_workspace_cap": (C.c_int, [_vp, C.c_uint64]),
    "pa_fragani_tables": (C.c_int, [C.c_uint32, C.c_uint32, _vp, _vp]),
    "pa_fragani_identity": (C.c_double, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "pa_fasta_records": (C.c_int64, [_vp, C.c_uint64, _vp, _vp, C.c_uint64]),
    "pa_write_comparisons_json": (
        C.c_int,
        [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, _vp],
    ),
    "pa_append_comparisons_json": (
        C.c_int,
        [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, _vp],
    ),
    "pa_append_comparisons_json_ex": (
        C.c_int,
        [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, _vp, _vp, _vp],
    ),
    "pa_round_sig6": (C.c_int, [_vp, C.c_uint64]),
    "pa_host_cpu_budget": (C.c_uint32, []),
    "pa_gunzip": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, _u64p, C.c_int]),
    "pa_sqlite_insert_comparisons": (
        C.c_int,
        [C.c_char_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, _vp, _u64p],
    ),
    "pa_sqlite_insert_comparisons_ex": (
        C.c_int,
        [C.c_char_p, C.c_int64, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, _vp,
         _vp, _vp, _u64p],
    ),
    "pa_msa_load": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "pa_msa_info": (C.c_int, [_vp, _u32p, _u64p, C.c_char_p, _u64p]),
    "pa_msa_record": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_char_p), _u64p, _u64p]),
    "pa_msa_copy_rows": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint64, _vp]),
    "pa_msa_free": (None, [_vp]),
    "pa_msa_plane_words": (C.c_uint64, [C.c_uint32, C.c_uint64, C.c_uint32]),
    "pa_msa_pack": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp]),
    "pa_msa_pair_counts": (
        C.c_int,
        [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp],
    ),
    "pa_msa_metrics": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.c_uint32]),
    "pa_append_msa_json": (
        C.c_int,
        [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp, _vp],
    ),
    "pa_classify_edges": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_int, C.c_int, C.c_double, C.c_uint64, _vp, _vp, _vp, _vp, _u64p]),
    "pa_classify_edges_host": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int, C.c_int, C.c_double, C.c_uint64, _vp, _vp, _vp, _vp, _u64p]),
    "pa_classify_tani_host": (C.c_int, [_vp, C.c_uint64, _vp]),
    "pa_classify_cliques": (C.c_int, [C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pa_cliques_info": (C.c_int, [_vp, _u64p, _u64p]),
    "pa_cliques_copy": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pa_cliques_free": (None, [_vp]),
    "pa_rowdist_euclid": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, _vp]),
    "pa_rowdist_euclid_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32]),
    "pa_linkage_average": (C.c_int, [C.c_uint32, _vp, _vp, _vp]),
    "pa_runcomp_join": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _u64p]),
    "pa_minmax_f64": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _u64p]),
    "pa_hist_uniform_f64": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_runcomp_join_host": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _u64p]),
    "pa_minmax_f64_host": (C.c_int, [_vp, C.c_uint64, _vp, _u64p]),
    "pa_hist_uniform_f64_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_write_pairs_tsv": (C.c_int, [C.c_char_p, C.c_char_p, _vp, _vp, C.c_uint64]),
    "pa_select_f64": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_moments_f64": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "pa_kde_gauss_f64": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_double, _vp]),
    "pa_hist_uniform_f64_wide": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_select_f64_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_moments_f64_host": (C.c_int, [_vp, C.c_uint64, _vp]),
    "pa_kde_gauss_f64_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, C.c_double, _vp]),
    "pa_hist_uniform_f64_wide_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_bin2d_f64": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "pa_bin2d_f64_host": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "pa_tetra_counts": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp]),
    "pa_tetra_counts_host": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint32]),
    "pa_tetra_zscores_host": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),
    "pa_tetra_corr": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _vp]),
    "pa_tetra_corr_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _vp, C.c_uint32]),
    "pa_nj": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "pa_nj_host": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp, C.c_uint32]),
    "pa_mul_tall_f64": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    "pa_mul_tall_f64_host": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, _vp, C.c_uint32]),
    "pa_gower_center": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "pa_gower_center_host": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32]),
    "pa_symm_top_eigs": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_double, _vp, _vp, _vp, _vp]),
    "pa_symm_top_eigs_host": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_double, _vp, _vp, _vp, _vp, C.c_uint32]),
    "pa_mantel_permutations": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    "pa_mantel": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp]),
    "pa_mantel_host": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, C.c_uint32]),
    "pa_msa_boot_weights": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _vp]),
    "pa_msa_boot_counts": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "pa_msa_boot_counts_host": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, C.c_uint32]),
    "pa_msa_boot_distances": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_double, _vp]),
    "pa_msa_boot_distances_host": (C.c_int, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_double, _vp, C.c_uint32]),
    "pa_tree_support": (C.c_int, [C.c_uint32, _vp, C.c_uint32, _vp, _vp]),
    "pa_derep_adjacency": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_int, C.c_int, C.c_double, C.c_double, _vp]),
    "pa_derep_adjacency_host": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int, C.c_int, C.c_double, C.c_double, _vp, C.c_uint32]),
    "pa_derep_select": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int, _vp, _u32p, _u32p]),
    "pa_derep_select_host": (C.c_int, [_vp, C.c_uint32, C.c_int, _vp, _u32p]),
    "pa_derep_assign": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp]),
    "pa_derep_assign_host": (C.c_int, [_vp, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, C.c_uint32]),
    "pa_append_identity_json": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, _vp, _vp]),
    "pa_prof_enable": (C.c_int, [_vp, C.c_int]),
    "pa_prof_reset": (C.c_int, [_vp]),
    "pa_prof_get": (C.c_int, [_vp, C.c_int, _f64p, _u64p]),
}

# The probes of the internal radix sort and exclusive scan (csrc/radix_sort.hip): libpyani_hip_tools.so alone exports
# them, for tests/test_gpu_sort_scan.py; load_library(tools=True) types them as well.  Not part of the ABI version.
TOOL_SIGNATURES: dict[str, tuple] = {
    "pa_tool_radix_sort_pairs": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "pa_tool_exclusive_scan_u32": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp]),
}


class HipBackendError(RuntimeError):
    """The HIP extension is missing, failed to load, or a call into it failed."""


_libs: dict[bool, C.CDLL] = {}


def build_library(force: bool = False) -> Path:
    """Compile ``libpyani_hip.so`` and ``libpyani_hip_tools.so`` for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcdir = _PKG / "csrc"
    cmd = ["make", "-C", str(srcdir), "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        cmd.append("-B")
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0 or not LIB_PATH.is_file() or not TOOLS_LIB_PATH.is_file():
        raise HipBackendError(f"building libpyani_hip.so failed:\n{proc.stdout}\n{proc.stderr}")
    return LIB_PATH


def load_library(tools: bool = False) -> C.CDLL:
    """Load the shared library (``tools``: the -DPA_TOOLS build, with its probes) and type every symbol of the header; raise loudly if absent."""
    if tools in _libs:
        return _libs[tools]
    path = TOOLS_LIB_PATH if tools else LIB_PATH
    if not path.is_file():
        raise HipBackendError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pyani_plus_amd/csrc`).  There is no CPU fallback for the compute path."
        )
    # PyTorch's ROCm wheel bundles its own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one
    # process cannot both own the GPU, so torch goes first and this library (same soname,
    # libamdhip64.so.7) binds to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - plain ROCm install without torch
        pass
    try:
        lib = C.CDLL(str(path))
    except OSError as err:  # missing ROCm runtime, wrong arch, ...
        raise HipBackendError(f"cannot load {path}: {err}") from err
    for name, (restype, argtypes) in {**SIGNATURES, **(TOOL_SIGNATURES if tools else {})}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as err:
            raise HipBackendError(f"{path} does not export {name}") from err
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.pa_abi_version() != ABI_VERSION:
        raise HipBackendError(f"ABI version mismatch: library reports {lib.pa_abi_version()}, binding expects {ABI_VERSION}")
    _libs[tools] = lib
    return lib


def last_error(lib: C.CDLL | None = None) -> str:
    return ((lib or load_library()).pa_last_error() or b"").decode(errors="replace")


def check(status: int, what: str, lib: C.CDLL | None = None) -> None:
    if status != PA_OK:
        err = HipBackendError(f"{what} failed with status {status}: {last_error(lib)}")
        err.status = status  # the library's code (PA_E_*), for callers that tell failures apart
        raise err
