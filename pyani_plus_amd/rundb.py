"""Run drivers for the four methods ``sourmash-hip``, ``fastANI-hip``, ``external-alignment-hip`` and ``TETRA-hip``,
``resume``, ``search_run`` (new genomes looked up in a ``sourmash-hip`` run: it sketches, so it lives with the
drivers), and the command line of the drivers and of the run reports.

The reference's Python (Typer CLI, SQLAlchemy ORM, snakemake) does not travel to the GPU box, so this module is the
build's own counterpart of ``cli_sourmash`` / ``fastani`` / ``external_alignment`` + ``start_and_run_method`` +
``run_method`` minus snakemake (pyani_plus/public_cli.py:115-329, 502-554, 598-699) and of ``resume`` (702-828); a
second file with the md5 of an earlier one aborts the run (public_cli.py:165-171).

Every run takes the same steps: register the genomes, record the run, find what the database lacks
(``_begin_missing``), compute it (the method's ``_compute_missing_<method>``, listed in ``_METHODS``) and finish
(``_finish_run``); ``_RunState`` carries what the steps share.

The database layer is ``run_store`` and the eight reports of a recorded run (``export_run``, ``classify``, ``plot_run``,
``plot_run_comp``, ``tree_run``, ``bootstrap_run``, ``phylo_run``, ``ordinate_run``, ``mantel_run_comp``, ``dereplicate_run``) are ``reports``.  This module imports ``reports``, which
imports ``run_store``, never the other way round, and re-exports both: ``rundb.<name>`` is the public face of all three.
"""

from __future__ import annotations

import argparse
import contextlib
import enum
import hashlib
import importlib
import logging
import os
import sqlite3
import sys
import tempfile
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import launch, reports, wire
from . import classify as classify_mod
from . import dereplicate as dereplicate_mod
from . import scatter as scatter_mod
from . import search as search_mod
from . import substitution as substitution_mod
from . import tree as tree_mod
from ._capi import HipBackendError
from .distributed import shard_bounds_by_cost
from .engine import HipEngine, load_fasta_files, max_hash_for_scaled
from .methods import external_alignment_hip, fastani_hip, sourmash_hip, tetra_hip
from .methods.external_alignment_hip import filename_stem  # noqa: F401  (reached as ``rundb.filename_stem``)
from .reports import _require_database, bootstrap_run, classify, dereplicate_run, export_run, mantel_run_comp, ordinate_run, phylo_run, plot_run, plot_run_comp, tree_run  # noqa: F401
from .run_store import (FASTA_EXTENSIONS, INSERT_COMPARISON, SCHEMA, Configuration, Run, RunGenomeAssociation, Session, _load_tile,  # noqa: F401
                        _open_run, _select_run_comparisons, _store_matrix_cache, add_run, cache_comparisons, cache_matrices, check_fasta,
                        connect_to_db, count_run_comparisons, db_configuration, db_genome, fasta_length_and_description,
                        format_matrix_cache, import_json_comparisons, import_tile, ingest_matrices, ingest_matrices_native, load_run)  # fmt: skip


# ------------------------------------------------------------------ what the steps of a run share
def _phase_clock(timings: dict | None):
    marks = {"start": time.perf_counter()}

    def mark(name: str) -> None:
        marks[name] = time.perf_counter()
        if timings is not None:
            prev = list(marks)[-2]
            timings[name] = marks[name] - marks[prev]

    return mark


@dataclass
class _RunState:
    """What the steps of one run share: built once by ``run_*_hip`` / ``resume``."""

    logger: logging.Logger
    conn: sqlite3.Connection
    tmp_dir: Path
    cache_dir: Path | None  # sourmash-hip's signature cache as the caller named it (None: a temporary one)
    engine: object
    gpus: int
    engine_factory: str | None
    ingest: str
    mark: object  # ``_phase_clock``'s
    run: Run | None = None  # set by ``_record_run`` (sourmash-hip's workers read the files before there is a run)
    session: Session | None = None


class _MatrixCache(enum.Enum):
    """Where ``_finish_run`` takes the five ``runs.df_*`` strings of a directly ingested run from."""

    FORMATTED = enum.auto()  # ``_DirectResult.formatted`` holds them
    TOO_BIG = enum.auto()  # beyond a SQLite value (``_matrix_cache_too_big``): the columns stay NULL
    REBUILD = enum.auto()  # a resumed run, only some columns in memory: read the table back


@dataclass
class _DirectResult:
    """What ``_ingest_direct`` leaves for ``_finish_run``: the rows the table holds now and the matrices in memory."""

    rows: int
    hashes: list[str]
    identity: np.ndarray
    cov_query: np.ndarray
    is_null: np.ndarray
    matrix_cache: _MatrixCache
    formatted: dict[str, str] | None = None


def _work_dir(path: Path | None, prefix: str = "pyani_hip_") -> Path:
    """The directory the caller named, or a fresh temporary one; it exists afterwards."""
    path = Path(path) if path else Path(tempfile.mkdtemp(prefix=prefix))
    path.mkdir(parents=True, exist_ok=True)
    return path


def _record_genome(logger, conn, md5_to_filename: dict[str, Path], filename: Path, md5: str, length: int, description: str) -> None:
    """One input file into ``genomes``; a second file with the same content ends the run
    (pyani_plus/public_cli.py:165-171)."""
    if md5 in md5_to_filename:
        dups = "\n" + "\n".join(sorted({str(md5_to_filename[md5]), str(filename)}))
        sourmash_hip.log_sys_exit(logger, f"Multiple genomes with same MD5 checksum {md5}:{dups}")
    md5_to_filename[md5] = filename
    db_genome(conn, filename, md5, length, description)


def _register_genomes(logger, conn, fasta_names: list[Path], mark) -> dict[str, Path]:
    """Checksum, length and title of every file into ``genomes``, on host threads only (this process touches no GPU);
    returns checksum -> file, in file order."""
    infos, _arena = load_fasta_files(fasta_names)
    md5_to_filename: dict[str, Path] = {}
    for filename, info in zip(fasta_names, infos):
        if info.status != 0:
            sourmash_hip.log_sys_exit(logger, info.message)
        _record_genome(logger, conn, md5_to_filename, filename, info.md5, info.length, info.description)
    del _arena
    mark("register_genomes")
    return md5_to_filename


def _record_run(state: _RunState, config: Configuration, fasta: Path, status: str, name: str | None, md5_to_filename: dict[str, Path]) -> None:
    """The new run (``name`` None: "N genomes using <method>"), its genomes in file order, and the session that
    persists its status."""
    filename_to_md5 = {filename: md5 for md5, filename in md5_to_filename.items()}
    if name is None:
        name = f"{len(filename_to_md5)} genomes using {config.method}"
    state.run = add_run(state.conn, config, " ".join(sys.argv), fasta, status, name, filename_to_md5)
    state.session = Session(state.conn, state.run)


def _incomplete_columns(conn, run: Run) -> list[str]:
    """Subject genomes of the run with fewer than N comparisons recorded (the columns the reference's ``resume``
    recomputes, pyani_plus/public_cli.py:243-261)."""
    n = len(run.fasta_hashes)
    have = dict(_select_run_comparisons(conn, run, "c.subject_hash, COUNT(*)", "GROUP BY c.subject_hash"))
    return sorted(a.genome_hash for a in run.fasta_hashes if have.get(a.genome_hash, 0) < n)


def _begin_missing(state: _RunState) -> tuple[int, list[str] | None] | None:
    """What the database does not hold yet, for a new run (all of it) or a resumed one (the incomplete subject columns
    only: rows that are there are never recomputed, nor -- INSERT OR IGNORE -- written twice).  Returns (rows there,
    those columns or None for all) with the run marked "Running"; None when nothing is missing."""
    run, method = state.run, state.run.configuration.method
    n = len(run.fasta_hashes)
    done = count_run_comparisons(state.conn, run)
    if done == n * n:
        state.logger.info("Database already has all %d=%d^2 %s comparisons", n * n, n, method)
        return None
    state.logger.info("Database already has %d of %d^2=%d %s comparisons, %d needed", done, n, n * n, method, n * n - done)
    columns = None if done == 0 else _incomplete_columns(state.conn, run)
    run.status = "Running"
    state.session.commit()
    return done, columns


def _genome_lengths(state: _RunState) -> dict[str, int]:
    """The column workers' ``query_hashes``: every genome of the run with its length."""
    lengths = dict(state.conn.execute("SELECT genome_hash, length FROM genomes"))
    return {a.genome_hash: lengths[a.genome_hash] for a in state.run.fasta_hashes}


def _column_worker(state: _RunState, compute, json_file: Path, query_hashes: dict[str, int], subject: str, **kwargs) -> None:
    """One call of a method's column worker, with the ten positional arguments the reference gives its own
    (pyani_plus/private_cli.py:956-968); a return code ends the run."""
    run = state.run
    hash_to_filename = {a.genome_hash: a.fasta_filename for a in run.fasta_hashes}
    status = compute(
        state.logger, state.tmp_dir, state.session, run, json_file, Path(run.fasta_directory), hash_to_filename,
        {v: k for k, v in hash_to_filename.items()}, query_hashes, subject, engine=state.engine, **kwargs,
    )  # fmt: skip
    if status:
        sourmash_hip.log_sys_exit(state.logger, f"Column worker failed with return code {status}")


def _json_columns(state: _RunState, compute, query_hashes: dict[str, int], columns: list[str] | None, **kwargs) -> None:
    """The reference's route: one column file per subject of ``columns`` (None: one file with all columns), each
    imported as soon as it is written; an interrupted worker's partial file is the last."""
    run = state.run
    for c, subject in enumerate([""] if columns is None else columns):
        json_file = state.tmp_dir / f"{run.configuration.method}.run_{run.run_id}.column_{c if subject else 0}.json"
        _column_worker(state, compute, json_file, query_hashes, subject, **kwargs)
        state.mark("pairs_and_column_file")
        import_json_comparisons(state.logger, state.conn, json_file)
        state.mark("import_column_file")
        if run.status == "Worker interrupted":
            break


def _launch_workers(logger, gpus: int, spec: dict, work_dir: Path, engine_factory: str | None) -> list[dict]:
    """``gpus`` worker processes on ``spec`` -> their reports; a failing rank's message ends the run."""
    if engine_factory:
        spec["engine_factory"] = engine_factory
    try:
        return launch.launch_workers(gpus, spec, work_dir)
    except launch.WorkerFailure as err:
        sourmash_hip.log_sys_exit(logger, str(err))


def _place_blocks(hashes: list[str], blocks, out) -> int:
    """Blocks ``(queries, subjects, one array per matrix of out)`` into the square matrices ``out`` (rows and columns in
    ``hashes`` order): the blocks arrive in their makers' order, so every one is placed by checksum.  Returns the
    number of cells placed."""
    pos = {h: i for i, h in enumerate(hashes)}
    cells = 0
    for queries, subjects, *arrays in blocks:
        at = np.ix_([pos[q] for q in queries], [pos[x] for x in subjects])
        for matrix, block in zip(out, arrays):
            matrix[at] = block
        cells += len(queries) * len(subjects)
    return cells


def _ingest_direct(state: _RunState, hashes: list[str], cols: list[str], ident, cov, null, *, aln_length=None, sim_errors=None) -> _DirectResult:
    """Matrices in host memory (rows = ``hashes``, columns = ``cols``, both sorted) -> comparison rows in index order,
    the five cached matrices formatted on a second thread meanwhile (when the block is the whole square)."""
    conn, run = state.conn, state.run
    # synchronous=NORMAL for the bulk insert: a handful of fsyncs per transaction instead of one per page group, and
    # -- unlike OFF -- no way for a crash of the machine to corrupt the user's multi-run database
    conn.execute("PRAGMA synchronous=NORMAL")
    conn.execute("PRAGMA cache_size=-1048576")
    square = cols == hashes
    with ThreadPoolExecutor(max_workers=1) as side:
        formatting = side.submit(format_matrix_cache, hashes, ident, cov, null, aln_length=aln_length, sim_errors=sim_errors) if square else None
        ingest_matrices(conn, run, hashes, cols, ident, cov, null, aln_length=aln_length, sim_errors=sim_errors)
        formatted = formatting.result() if formatting is not None else None
    conn.execute("PRAGMA synchronous=FULL")
    state.mark("insert_rows")
    if not square:
        matrix_cache = _MatrixCache.REBUILD
    else:
        matrix_cache = _MatrixCache.TOO_BIG if formatted is None else _MatrixCache.FORMATTED
    # what is in the database now, not what was handed to the insert (INSERT OR IGNORE reports nothing per row)
    return _DirectResult(count_run_comparisons(conn, run), hashes, ident, cov, null, matrix_cache, formatted)


def _finish_run(state: _RunState, result: _DirectResult | None) -> Run:
    """Completion test, matrix cache, status "Done" (pyani_plus/public_cli.py:302-324).  ``result``: None after the
    JSON route (and whenever the rows went in piecewise)."""
    logger, conn, run = state.logger, state.conn, state.run
    n = len(run.fasta_hashes)
    done = count_run_comparisons(conn, run) if result is None else result.rows
    if done != n * n and run.status == "Worker interrupted":
        # the reference's worker ends with return code 0 after an interrupt, its partial results recorded and the run
        # marked (pyani_plus/private_cli.py:1889-1902); ``resume`` completes such a run
        logger.warning("Interrupted: %d of %d^2=%d %s comparisons recorded; the run can be resumed", done, n, n * n, run.configuration.method)
        state.session.commit()
        conn.close()
        return run
    if done != n * n:
        sourmash_hip.log_sys_exit(logger, f"Only have {done} of {n}^2={n * n} {run.configuration.method} comparisons needed")
    if result is None or result.matrix_cache is _MatrixCache.REBUILD:
        cache_comparisons(conn, run)
    elif result.matrix_cache is _MatrixCache.TOO_BIG:
        _store_matrix_cache(conn, run, None)
    else:
        cache_matrices(conn, run, result.hashes, result.identity, result.cov_query, result.is_null, formatted=result.formatted)
    state.mark("matrix_cache")
    run.status = "Done"
    state.session.commit()
    conn.close()
    return run


# ------------------------------------------------------------------ sourmash-hip (pyani_plus/public_cli.py:115-329)
def _compute_direct(state: _RunState, *, subjects: list[str] | None = None) -> _DirectResult:
    """Subject tiles -> binary column files + matrices in host memory -> rows inserted in index order.
    ``subjects``: only these subject columns (resuming a partial run); the matrices then hold those columns."""
    logger, run = state.logger, state.run
    config = run.configuration
    hashes = sorted(a.genome_hash for a in run.fasta_hashes)
    cols = hashes if subjects is None else sorted(subjects)
    n, nc = len(hashes), len(cols)
    ident = np.empty((n, nc), dtype=np.float64)
    cov = np.empty((n, nc), dtype=np.float64)
    null = np.empty((n, nc), dtype=bool)
    sig_cache = sourmash_hip.sig_cache_dir(state.cache_dir, config.kmersize, config.extra)
    col = 0
    try:
        for t, (queries, tile, t_cov, t_ident, t_null) in enumerate(
            sourmash_hip.iter_sourmash_tiles(
                logger, cols, hashes, sig_cache, kmersize=config.kmersize, scaled=sourmash_hip.parse_scaled(config.extra), engine=state.engine
            )
        ):
            assert queries == hashes and tile == cols[col : col + len(tile)]
            wire.save_tile(state.tmp_dir / f"{sourmash_hip.METHOD}.run_{run.run_id}.tile_{t}.npz", config, queries, tile, t_ident, t_cov, t_null)
            ident[:, col : col + len(tile)] = t_ident
            cov[:, col : col + len(tile)] = t_cov
            null[:, col : col + len(tile)] = t_null
            col += len(tile)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, f"{sourmash_hip.METHOD} comparison", err)
    state.mark("pairs_and_tile_files")
    return _ingest_direct(state, hashes, cols, ident, cov, null)


def _file_cost(path: Path) -> int:
    """Bases a FASTA file is expected to hold, from its size (gzip: about a quarter of the text)."""
    try:
        size = path.stat().st_size
    except OSError:
        return 0
    return 4 * size if path.name.endswith(".gz") else size


def _sharded_sourmash_tiles(state: _RunState, config: Configuration, fasta: Path, fasta_names: list[Path], gpus: int,
                            columns: list[str] | None = None):
    """The multi-GPU form of "sketch everything, compare everything" (DESIGN.md section 6): ``gpus`` fresh worker
    processes (``launch.launch_workers`` -- started before this process has touched a GPU), each sketching a
    length-balanced share of the files, ONE all-gather of the sketches, each rank evaluating all queries against its
    own genomes as subject columns (``columns``, checksums: only those of them -- what a resumed run still needs).
    Returns (metadata per file in file order, the ranks' tile files); None when the ranks were interrupted (their
    columns need every rank's sketches: there is nothing partial to keep)."""
    shards = shard_bounds_by_cost([max(1, _file_cost(p)) for p in fasta_names], gpus)
    work_dir = state.tmp_dir / f"{sourmash_hip.METHOD}.workers"
    spec = {
        "task": "sourmash", "fasta_dir": str(fasta), "fasta_files": [str(p) for p in fasta_names], "shards": shards,
        "configuration": {k: getattr(config, k) for k in wire.CONFIG_FIELDS}, "cache": str(state.cache_dir), "work_dir": str(work_dir),
    }  # fmt: skip
    if columns is not None:
        spec["columns"] = list(columns)
    results = _launch_workers(state.logger, gpus, spec, work_dir, state.engine_factory)
    if any(r.get("interrupted") for r in results):
        return None
    meta = [m for r in results for m in r["meta"]]
    assert [m["path"] for m in meta] == [str(p) for p in fasta_names]
    return meta, [Path(r["tile"]) for r in results if r.get("tile")]


def _run_sourmash_sharded(state: _RunState, config: Configuration, fasta: Path, fasta_names: list[Path], name: str | None) -> Run:
    """A new run on worker processes.  The genomes' checksums come from the ranks, so the run is recorded after their
    work, and the ranks' tiles -- all N^2 comparisons -- go in as one square."""
    logger, mark = state.logger, state.mark
    sharded = _sharded_sourmash_tiles(state, config, fasta, fasta_names, state.gpus)
    if sharded is None:
        sourmash_hip.log_sys_exit(logger, "Interrupted before the sketches were exchanged; no run was recorded")
    meta, tile_files = sharded
    md5_to_filename: dict[str, Path] = {}
    for filename, m in zip(fasta_names, meta):
        _record_genome(logger, state.conn, md5_to_filename, filename, m["md5"], m["length"], m["description"])
    mark("workers_front_end_sketch_and_pairs")
    _record_run(state, config, fasta, "Running", name, md5_to_filename)
    hashes = sorted(md5_to_filename)
    n = len(hashes)
    ident = np.empty((n, n), dtype=np.float64)
    cov = np.empty((n, n), dtype=np.float64)
    null = np.empty((n, n), dtype=bool)
    tiles = (_load_tile(logger, tile_file, config) for tile_file in tile_files)  # one in memory at a time
    filled = _place_blocks(hashes, tiles, (ident, cov, null))  # every tile holds all n queries
    if filled != n * n:
        sourmash_hip.log_sys_exit(logger, f"The workers returned {filled // n} of {n} subject columns")
    mark("assemble_tiles")
    return _finish_run(state, _ingest_direct(state, hashes, hashes, ident, cov, null))


def _resume_sourmash_sharded(state: _RunState, gpus: int) -> None:
    """The missing columns of a recorded run through the same executor as the run itself (pyani_plus/public_cli.py:243-261
    re-runs the missing columns through the workflow they came from): worker processes, one all-gather, and each rank's
    tile cut down to the missing columns."""
    logger, run = state.logger, state.run
    fasta = Path(run.fasta_directory)
    columns = _incomplete_columns(state.conn, run)
    logger.info("%d subject columns to compute on %d worker processes", len(columns), gpus)
    run.status = "Running"
    state.session.commit()
    names = [fasta / a.fasta_filename for a in sorted(run.fasta_hashes, key=lambda a: a.fasta_filename)]
    sharded = _sharded_sourmash_tiles(state, run.configuration, fasta, names, gpus, columns=columns)
    if sharded is None:
        run.status = "Worker interrupted"
        return
    meta, tile_files = sharded
    recorded = {a.fasta_filename: a.genome_hash for a in run.fasta_hashes}
    for m in meta:  # the files must still be the ones the run was made from
        if recorded[Path(m["path"]).name] != m["md5"]:
            sourmash_hip.log_sys_exit(
                logger, f"run-id {run.run_id} used {m['path']} with MD5 {recorded[Path(m['path']).name]} but the file now has MD5 {m['md5']}"
            )
    for tile_file in tile_files:
        import_tile(logger, state.conn, run, tile_file)


def _compute_missing_sourmash(state: _RunState, *, presketched=None) -> _DirectResult | None:
    """The comparisons of a ``sourmash-hip`` run that the database does not hold yet: in this process through the
    column worker's JSON files or directly from the tiles (``state.ingest``), or -- a resumed run with ``gpus`` > 1 --
    on worker processes."""
    conn, run = state.conn, state.run
    n = len(run.fasta_hashes)
    state.cache_dir = _work_dir(state.cache_dir, "pyani_hip_cache_")
    gpus = max(1, min(int(state.gpus), n))
    if gpus > 1 and count_run_comparisons(conn, run) != n * n:
        _resume_sourmash_sharded(state, gpus)
        return None
    missing = _begin_missing(state)
    if missing is None:
        return None
    _done, columns = missing
    # the genomes were sketched while their checksums were taken: only the signature files remain to be written
    for _ in sourmash_hip.prepare_genomes(state.logger, run, state.cache_dir, engine=state.engine, presketched=presketched):
        pass
    state.mark("signature_files")
    if state.ingest == "direct":
        return _compute_direct(state, subjects=columns)
    _json_columns(state, sourmash_hip.compute_sourmash_hip, _genome_lengths(state), columns, cache=state.cache_dir)
    return None


def run_sourmash_hip(  # noqa: PLR0913
    fasta: Path,
    database: Path | str,
    *,
    cache: Path | None = None,
    name: str | None = None,
    kmersize: int = sourmash_hip.KMER_SIZE,
    scaled: int = sourmash_hip.SCALED,
    temp: Path | None = None,
    logger: logging.Logger | None = None,
    engine=None,
    ingest: str = "json",
    timings: dict | None = None,
    gpus: int = 1,
    engine_factory: str | None = None,
) -> Run:
    """FASTA directory -> database with all N^2 comparisons and cached matrices.

    Counterpart of ``pyani-plus sourmash <fasta> -d <db> --create-db`` (call stack in
    SURVEY.md section 3.1) with the snakemake layer replaced by one in-process call.

    ``ingest="json"`` goes through the reference's column file (worker -> JSON -> importer), what two
    processes of the reference would do.  ``ingest="direct"`` keeps the subject tiles as binary column
    files (``wire.save_tile``) plus in-memory matrices, inserts the rows in index order straight from them and
    writes the matrix cache from memory: the form that stays feasible at N = 10^4 (10^8 rows).
    ``gpus`` > 1: the sketching and the comparisons are spread over that many worker processes, one per GPU
    (``_run_sourmash_sharded``; the caller must not have initialised the GPU in this process); results always take
    the direct route.  ``timings`` (a dict) receives the wall seconds of the phases."""
    mark = _phase_clock(timings)
    logger = logger or logging.getLogger("pyani_plus_amd")
    fasta = Path(fasta)
    if not 1 <= int(kmersize) <= 64:  # before any file is read
        sourmash_hip.log_sys_exit(logger, f"{sourmash_hip.METHOD} supports k-mer sizes 1 to 64, not {kmersize}")
    if int(scaled) < 1:
        sourmash_hip.log_sys_exit(logger, f"scaled must be a positive integer, not {scaled}")
    if ingest not in {"json", "direct"}:
        sourmash_hip.log_sys_exit(logger, f"ingest must be 'json' or 'direct', not {ingest!r}")
    if int(gpus) < 1:
        sourmash_hip.log_sys_exit(logger, f"gpus must be a positive integer, not {gpus}")
    fasta_names = check_fasta(logger, fasta)
    tool = sourmash_hip.get_sourmash_hip()
    conn = connect_to_db(database)
    config = db_configuration(
        conn, sourmash_hip.METHOD, tool.exe_path.stem, tool.version, kmersize=kmersize, extra=f"scaled={scaled}"
    )
    gpus = min(int(gpus), len(fasta_names))
    state = _RunState(logger, conn, _work_dir(temp), _work_dir(cache, "pyani_hip_cache_"), engine, gpus, engine_factory, ingest, mark)
    # PYANI_HIP_FORCE_WORKERS=1 sends even one GPU's worth of work through a worker process (RCCL with world size 1):
    # the multi-GPU code path on a single-GPU box
    if gpus > 1 or os.environ.get("PYANI_HIP_FORCE_WORKERS") == "1":
        return _run_sourmash_sharded(state, config, fasta, fasta_names, name)
    # One pass over the files: md5 of the decompressed bytes, length, first title AND the sketches -- the host
    # front-end of the next batch of files runs while the device hashes the current one (sketch_fasta_batches).
    sig_dir = sourmash_hip.sig_cache_dir(state.cache_dir, kmersize, f"scaled={scaled}")
    md5_to_filename: dict[str, Path] = {}
    presketched: dict[str, np.ndarray] = {}
    try:
        for batch_paths, infos, sketches in sourmash_hip.sketch_fasta_batches(
            logger, fasta_names, kmersize=kmersize, scaled=scaled, engine=engine, needed=lambda info: not (sig_dir / f"{info.md5}.sig").is_file()
        ):
            for filename, info, mins in zip(batch_paths, infos, sketches):
                _record_genome(logger, conn, md5_to_filename, filename, info.md5, info.length, info.description)
                if mins is not None:
                    presketched[info.md5] = mins
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, f"{sourmash_hip.METHOD} sketching", err)
    mark("fasta_front_end_and_sketch")
    _record_run(state, config, fasta, "Initialising", name, md5_to_filename)
    return _finish_run(state, _compute_missing_sourmash(state, presketched=presketched))


# ------------------------------------------------------------------ fastANI-hip (pyani_plus/public_cli.py:502-554)
def _fastani_workers(state: _RunState, hashes: list[str], column_runs: list[tuple[int, int]], query_hashes: dict[str, int], gpus: int,
                     query_batch: int | None) -> list[tuple]:
    """The missing columns as reference ranges of ``pa_fragani`` spread over ``gpus`` worker processes.  Every rank
    writes the reference's JSON column file, imported here on the JSON route; on the direct route the ranks' binary
    tile files come back as blocks."""
    logger, run = state.logger, state.run
    direct = state.ingest == "direct"
    # every rank maps all queries; what differs is the reference range, whose cost follows the subjects' lengths
    pieces = [(a + i, a + i + 1) for a, b in column_runs for i in range(b - a)]
    bounds = shard_bounds_by_cost([max(1, query_hashes[hashes[a]]) for a, _ in pieces], gpus)
    column_ranges = []
    for a, b in bounds:
        if a == b:
            column_ranges.append((0, 0))
            continue
        lo, hi = pieces[a][0], pieces[b - 1][1]
        if hi - lo != b - a:  # the rank's share is not one range (scattered missing columns): widen it, rows are idempotent
            logger.debug("rank share %s widened to columns %d..%d", (a, b), lo, hi)
        column_ranges.append((lo, hi))
    work_dir = state.tmp_dir / f"{fastani_hip.METHOD}.run_{run.run_id}.workers"
    spec = {
        "task": "fastani", "run_id": run.run_id, "fasta_dir": str(Path(run.fasta_directory)),
        "hash_to_filename": {a.genome_hash: a.fasta_filename for a in run.fasta_hashes},
        "query_hashes": query_hashes, "column_ranges": column_ranges, "work_dir": str(work_dir), "tiles": direct,
        "configuration": {**{k: getattr(run.configuration, k) for k in wire.CONFIG_FIELDS}, "configuration_id": run.configuration_id},
    }  # fmt: skip
    if query_batch:
        spec["query_batch"] = int(query_batch)
    results = _launch_workers(logger, gpus, spec, work_dir, state.engine_factory)
    state.mark("workers")
    blocks: list[tuple] = []
    for rank, r in enumerate(results):
        if r.get("interrupted"):
            run.status = "Worker interrupted"
        if direct:
            for tile in r.get("tiles") or sorted(str(t) for t in work_dir.glob(f"{fastani_hip.METHOD}.rank_{rank}.tile_*.npz")):
                try:
                    _cfg, queries, subjects, ident, cov, null, aln, sim = wire.load_tile(Path(tile), with_proxies=True)
                except (ValueError, OSError, KeyError, zipfile.BadZipFile) as err:
                    # tiles are written under another name and renamed: a rank that ended while it wrote (interrupted, or
                    # ended by this process) may leave an unreadable one, and the other ranks' batches still go in; from
                    # a rank that reported success it is damage, and the run must not end quietly incomplete
                    if not r.get("interrupted"):
                        raise
                    logger.warning("Skipping unreadable tile file %s of rank %d: %s", tile, rank, err)
                    continue
                blocks.append((queries, subjects, ident, aln, sim, cov, null))
        else:
            # the rank's column file: a complete JSON document after every finished query batch, also when the rank
            # was interrupted (or ended by this process while it waited) and reported nothing about it
            c0, c1 = column_ranges[rank]
            json_file = Path(r["json"]) if r.get("json") else work_dir / f"{fastani_hip.METHOD}.run_{run.run_id}.columns_{c0 + 1}_{c1}.json"
            if c0 != c1 and json_file.is_file():
                try:
                    import_json_comparisons(logger, state.conn, json_file)
                except (ValueError, OSError) as err:  # a column file cut short by the end of its rank (it is rewritten whole after every batch)
                    if not r.get("interrupted"):
                        raise
                    logger.warning("Skipping unreadable column file %s of rank %d: %s", json_file, rank, err)
    if run.status == "Worker interrupted":
        state.session.commit()
    return blocks


def _fastani_in_process(state: _RunState, column_runs: list[tuple[int, int]], query_hashes: dict[str, int], query_batch: int | None) -> list[tuple]:
    """The missing columns in this process: one call of the column worker per run of them.  Its JSON column file is
    imported on the JSON route; on the direct route its batches are collected as blocks."""
    run = state.run
    direct = state.ingest == "direct"
    if state.engine is None and state.engine_factory:  # the workers' engine, when their work has shrunk to one process's worth
        module, _, attr = state.engine_factory.partition(":")
        state.engine = getattr(importlib.import_module(module), attr)()
    blocks: list[tuple] = []
    for a, b in column_runs:
        json_file = state.tmp_dir / f"{fastani_hip.METHOD}.run_{run.run_id}.columns_{a + 1}_{b}.json"
        _column_worker(
            state, fastani_hip.compute_fastani_hip, json_file, query_hashes, "", subject_range=(a, b),
            on_block=(lambda *blk: blocks.append(blk)) if direct else None, **({"query_batch": int(query_batch)} if query_batch else {}),
        )  # fmt: skip
        if not direct:
            import_json_comparisons(state.logger, state.conn, json_file)
        if run.status == "Worker interrupted":
            break
    state.mark("worker")
    return blocks


def _ingest_fastani_blocks(state: _RunState, hashes: list[str], blocks: list[tuple], new_run: bool) -> _DirectResult | None:
    """Blocks ``(queries, subjects, identity, aln_length, sim_errors, cov_query, is_null)`` -> comparison rows.  All of a
    new run: one square, rows in index order, matrix cache from memory; otherwise block by block."""
    conn, run = state.conn, state.run
    n = len(hashes)
    if new_run and run.status != "Worker interrupted" and sum(len(b[0]) * len(b[1]) for b in blocks) == n * n:
        ident = np.full((n, n), np.nan)
        cov = np.full((n, n), np.nan)
        null = np.ones((n, n), dtype=bool)
        aln = np.zeros((n, n), dtype=np.int64)
        sim = np.zeros((n, n), dtype=np.int64)
        _place_blocks(hashes, blocks, (ident, aln, sim, cov, null))
        return _ingest_direct(state, hashes, hashes, ident, cov, null, aln_length=aln, sim_errors=sim)
    for queries, subjects, ident, aln, sim, cov, null in blocks:
        ingest_matrices(conn, run, queries, subjects, ident, cov, null, aln_length=aln, sim_errors=sim)
    if run.status != "Worker interrupted":  # whatever blocks of an interrupted run arrived are in; the run stays partial
        state.mark("insert_rows")
    return None


def _compute_missing_fastani(state: _RunState, *, query_batch: int | None = None) -> _DirectResult | None:
    """The incomplete subject columns of a ``fastANI-hip`` run: in this process (one call per run of missing columns; a
    new run is one call for all of them), or as reference ranges of ``pa_fragani`` spread over ``gpus`` worker
    processes -- the reference's own one-process-per-column layout (pyani_plus/public_cli.py:236-261) with a GPU per
    process and no exchange between them.  Every worker writes the reference's JSON column file.  ``ingest="json"``:
    this process imports those files, what the reference's parent does (pyani_plus/workflows/__init__.py:75-87);
    ``"direct"``: the rows go from the result arrays (binary tile files between processes) straight into the table.
    Returns ``_ingest_direct``'s result when a new run went in directly (matrix cache from memory), else None."""
    missing = _begin_missing(state)
    if missing is None:
        return None
    done, columns = missing
    hashes = sorted(a.genome_hash for a in state.run.fasta_hashes)
    pos = {h: i for i, h in enumerate(hashes)}
    # contiguous runs of missing columns; a new run is one run of all columns
    column_runs: list[tuple[int, int]] = []
    for i in (pos[c] for c in (hashes if columns is None else columns)):
        if column_runs and column_runs[-1][1] == i:
            column_runs[-1] = (column_runs[-1][0], i + 1)
        else:
            column_runs.append((i, i + 1))
    query_hashes = _genome_lengths(state)
    gpus = max(1, min(int(state.gpus), len(hashes if columns is None else columns)))
    if gpus > 1:
        blocks = _fastani_workers(state, hashes, column_runs, query_hashes, gpus, query_batch)
    else:
        blocks = _fastani_in_process(state, column_runs, query_hashes, query_batch)
    if state.ingest != "direct":
        state.mark("import_column_files")
        return None
    return _ingest_fastani_blocks(state, hashes, blocks, new_run=done == 0)


def run_fastani_hip(  # noqa: PLR0913
    fasta: Path,
    database: Path | str,
    *,
    name: str | None = None,
    kmersize: int | None = None,
    fragsize: int | None = None,
    minmatch: float | None = None,
    temp: Path | None = None,
    logger: logging.Logger | None = None,
    engine=None,
    gpus: int = 1,
    engine_factory: str | None = None,
    timings: dict | None = None,
    ingest: str = "json",
    query_batch: int | None = None,
) -> Run:
    """FASTA directory -> database with all N^2 fragment-ANI comparisons and cached matrices: counterpart of
    ``pyani-plus fastani <fasta> -d <db> --create-db`` (pyani_plus/public_cli.py:502-554) with one in-process call --
    or ``gpus`` worker processes, each mapping all queries against its own range of subject columns -- in place of the
    snakemake jobs.  Defaults as pyani_plus/methods/fastani.py:27-30.  The registration pass (checksum, length and
    title of every file) runs on host threads only, so this process never touches a GPU when ``gpus`` > 1."""
    mark = _phase_clock(timings)
    logger = logger or logging.getLogger("pyani_plus_amd")
    kmersize = fastani_hip.KMER_SIZE if kmersize is None else int(kmersize)
    fragsize = fastani_hip.FRAG_LEN if fragsize is None else int(fragsize)
    minmatch = fastani_hip.MIN_FRACTION if minmatch is None else float(minmatch)
    fasta = Path(fasta)
    fasta_names = check_fasta(logger, fasta)
    tool = fastani_hip.get_fastani_hip()
    conn = connect_to_db(database)
    config = db_configuration(conn, fastani_hip.METHOD, tool.exe_path.stem, tool.version, fragsize=fragsize, kmersize=kmersize, minmatch=minmatch)
    md5_to_filename = _register_genomes(logger, conn, fasta_names, mark)
    state = _RunState(logger, conn, _work_dir(temp), None, engine, gpus, engine_factory, ingest, mark)
    _record_run(state, config, fasta, "Initialising", name, md5_to_filename)
    if ingest not in {"json", "direct"}:
        sourmash_hip.log_sys_exit(logger, f"ingest must be 'json' or 'direct', not {ingest!r}")
    return _finish_run(state, _compute_missing_fastani(state, query_batch=query_batch))


# ------------------------------------------------------------------ external-alignment-hip (pyani_plus/public_cli.py:642-699)
def _one_gpu_only(logger, gpus: int) -> None:
    if int(gpus) != 1:
        sourmash_hip.log_sys_exit(logger, f"{external_alignment_hip.METHOD} runs on one GPU; --gpus {gpus} is not supported")


def _compute_missing_external_alignment(state: _RunState) -> None:
    """The subject columns the database does not complete yet, through the column worker and its JSON file: all of them
    in one device call for a new run, the incomplete ones (one call each, as the reference's resume) otherwise."""
    _one_gpu_only(state.logger, state.gpus)
    missing = _begin_missing(state)
    if missing is not None:
        query_hashes = {a.genome_hash: 0 for a in state.run.fasta_hashes}
        _json_columns(state, external_alignment_hip.compute_external_alignment_hip, query_hashes, missing[1])


def run_external_alignment_hip(  # noqa: PLR0913
    fasta: Path,
    database: Path | str,
    *,
    alignment: Path,
    label: str = "stem",
    name: str | None = None,
    temp: Path | None = None,
    logger: logging.Logger | None = None,
    engine=None,
    gpus: int = 1,
    timings: dict | None = None,
) -> Run:
    """FASTA directory + its MSA -> database with all N^2 external-alignment comparisons and cached matrices: counterpart
    of ``pyani-plus external-alignment <fasta> -d <db> --alignment <msa> --label <label> --create-db``
    (pyani_plus/public_cli.py:642-699).  As there, the configuration records the MSA's md5 and its file name only: the
    worker looks for the file next to the database.  One GPU: ``gpus`` > 1 is refused."""
    mark = _phase_clock(timings)
    logger = logger or logging.getLogger("pyani_plus_amd")
    _one_gpu_only(logger, gpus)
    if label not in {"md5", "filename", "stem"}:
        sourmash_hip.log_sys_exit(logger, f"label must be md5, filename or stem, not {label!r}")
    alignment = Path(alignment)
    if not alignment.is_file():
        sourmash_hip.log_sys_exit(logger, f"Missing alignment file {alignment}")
    fasta = Path(fasta)
    fasta_names = check_fasta(logger, fasta)
    tool = external_alignment_hip.get_external_alignment_hip()
    with alignment.open("rb") as handle:
        aln_md5 = hashlib.file_digest(handle, "md5").hexdigest() if hasattr(hashlib, "file_digest") else hashlib.md5(handle.read()).hexdigest()
    conn = connect_to_db(database)
    config = db_configuration(conn, external_alignment_hip.METHOD, tool.exe_path.stem, tool.version,
                              extra=external_alignment_hip.make_extra(aln_md5, label, alignment))  # fmt: skip
    md5_to_filename = _register_genomes(logger, conn, fasta_names, mark)
    state = _RunState(logger, conn, _work_dir(temp), None, engine, gpus, None, "json", mark)
    _record_run(state, config, fasta, "Initialising", f"Import of {alignment.name}" if name is None else name, md5_to_filename)
    return _finish_run(state, _compute_missing_external_alignment(state))


# ------------------------------------------------------------------ TETRA-hip (no counterpart in the reference)
def _tetra_one_gpu_only(logger, gpus: int) -> None:
    if int(gpus) != 1:
        sourmash_hip.log_sys_exit(logger, f"{tetra_hip.METHOD} runs on the host or on one GPU; --gpus {gpus} is not supported")


def _compute_missing_tetra(state: _RunState, *, precounted: dict | None = None) -> None:
    """The subject columns the database does not complete yet, through the column worker and its JSON file: the count
    files first (only those the cache lacks), then all columns in one file for a new run, the incomplete ones otherwise."""
    _tetra_one_gpu_only(state.logger, state.gpus)
    missing = _begin_missing(state)
    if missing is None:
        return
    state.cache_dir = _work_dir(state.cache_dir, "pyani_hip_cache_")
    for _ in tetra_hip.prepare_genomes(state.logger, state.run, state.cache_dir, engine=state.engine, precounted=precounted):
        pass
    state.mark("count_files")
    query_hashes = {a.genome_hash: 0 for a in state.run.fasta_hashes}
    _json_columns(state, tetra_hip.compute_tetra_hip, query_hashes, missing[1], cache=state.cache_dir)


def run_tetra_hip(  # noqa: PLR0913
    fasta: Path,
    database: Path | str,
    *,
    cache: Path | None = None,
    name: str | None = None,
    temp: Path | None = None,
    logger: logging.Logger | None = None,
    engine=None,
    timings: dict | None = None,
    gpus: int = 1,
) -> Run:
    """FASTA directory -> database with all N^2 TETRA-hip comparisons and cached matrices.  The reference has no such
    command; the method's definition is this project's own (``methods/tetra_hip.py``).  ``engine`` None computes on the
    host, a ``HipEngine`` on its device, with the same rows.  The configuration records method, program and version
    only; every row has an identity (NULL for a degenerate genome) and NULL coverage.  ``gpus`` > 1 is refused."""
    mark = _phase_clock(timings)
    logger = logger or logging.getLogger("pyani_plus_amd")
    _tetra_one_gpu_only(logger, gpus)
    fasta = Path(fasta)
    fasta_names = check_fasta(logger, fasta)
    tool = tetra_hip.get_tetra_hip()
    conn = connect_to_db(database)
    config = db_configuration(conn, tetra_hip.METHOD, tool.exe_path.stem, tool.version)
    # one pass over the files: checksum, length, title and -- from the same arena -- the counts
    infos, arena = load_fasta_files(fasta_names)
    md5_to_filename: dict[str, Path] = {}
    for filename, info in zip(fasta_names, infos):
        if info.status != 0:
            sourmash_hip.log_sys_exit(logger, info.message)
        _record_genome(logger, conn, md5_to_filename, filename, info.md5, info.length, info.description)
    mark("register_genomes")
    try:
        counts = tetra_hip.count_arena(arena, engine)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, f"{tetra_hip.METHOD} counting", err)
    del arena
    mark("counts")
    state = _RunState(logger, conn, _work_dir(temp), _work_dir(cache, "pyani_hip_cache_"), engine, gpus, None, "json", mark)
    _record_run(state, config, fasta, "Initialising", name, md5_to_filename)
    return _finish_run(state, _compute_missing_tetra(state, precounted={info.md5: row for info, row in zip(infos, counts)}))


_METHODS = {  # method name -> (its tool, its "compute what is missing"): what ``resume`` needs to know of a method
    sourmash_hip.METHOD: (sourmash_hip.get_sourmash_hip, _compute_missing_sourmash),
    fastani_hip.METHOD: (fastani_hip.get_fastani_hip, _compute_missing_fastani),
    external_alignment_hip.METHOD: (external_alignment_hip.get_external_alignment_hip, _compute_missing_external_alignment),
    tetra_hip.METHOD: (tetra_hip.get_tetra_hip, _compute_missing_tetra),
}


# ------------------------------------------------------------------ resume (pyani_plus/public_cli.py:702-828)
def resume(database: Path | str, *, run_id: int | None = None, cache: Path | None = None, temp: Path | None = None,
           logger: logging.Logger | None = None, engine=None, ingest: str = "json", gpus: int = 1,
           engine_factory: str | None = None) -> Run:
    """Complete a partial run of this backend: the missing subject columns are computed, the run is marked done.

    Same checks and messages as the reference's ``resume``: the database and the run must exist, the tool recorded
    with the run must be the one at hand (``We have ... but run-id N used ... instead``), the FASTA directory and
    every file of the run must still be there.  A complete run is left as it is."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    conn, run = _open_run(logger, database, run_id, "Resuming")
    run_id, config = run.run_id, run.configuration
    n = len(run.fasta_hashes)
    logger.info("This is a %s run on %d genomes, using %s version %s", config.method, n, config.program, config.version)
    if not n:
        sourmash_hip.log_sys_exit(logger, f"No genomes recorded for run-id {run_id}, cannot resume.")
    if config.method not in _METHODS:
        sourmash_hip.log_sys_exit(logger, f"Unknown method {config.method} for run-id {run_id} in {database}")
    get_tool, compute_missing = _METHODS[config.method]
    tool = get_tool()
    if tool.exe_path.stem != config.program or tool.version != config.version:
        sourmash_hip.log_sys_exit(
            logger,
            f"We have {tool.exe_path.stem} version {tool.version}, but run-id {run_id} used {config.program} version {config.version} instead.",
        )
    fasta = Path(run.fasta_directory)
    if not fasta.is_dir():
        sourmash_hip.log_sys_exit(logger, f"run-id {run_id} used input folder {fasta}, but that is not a directory (now).")
    for link in run.fasta_hashes:
        if not (fasta / link.fasta_filename).is_file():
            sourmash_hip.log_sys_exit(
                logger, f"run-id {run_id} used {fasta / link.fasta_filename} with MD5 {link.genome_hash} but this FASTA file no longer exists"
            )
    session = Session(conn, run)
    run.status = "Resuming"
    session.commit()
    state = _RunState(logger, conn, _work_dir(temp), cache, engine, gpus, engine_factory, ingest, _phase_clock(None), run, session)
    return _finish_run(state, compute_missing(state))


# ------------------------------------------------------------------ search-run (this project's own: the reference answers no such question)
def search_run(query_fasta: Path, database: Path | str, outdir: Path, *, run_id: int | None = None, cache: Path | None = None,  # noqa: PLR0913
               label: str = "stem", top: int = search_mod.TOP, rank: str = "identity", min_identity: float = 0.0, cov_min: float = 0.0,
               temp: Path | None = None, engine=None, engine_factory: str | None = None, logger: logging.Logger | None = None) -> list[Path]:
    """For every genome of the directory ``query_fasta``, the ``top`` (1 to 64) nearest genomes of a ``sourmash-hip``
    run (``search.search``), without adding it to the run: nothing is written to the database.
    The run (``run_id``; None: the last one) need not be complete: only its genomes, k-mer size and ``scaled`` are used.
    Its sketches come from the ``.sig`` cache ``cache`` (``prepare_genomes`` writes what it lacks from the run's FASTA
    directory; None: a temporary one under ``temp``, so every subject is sketched again); the queries are sketched with
    the run's parameters, in file-name order, and are neither recorded nor cached.  ``rank`` "identity" orders a query's
    subjects by the sourmash identity the run stores, the larger of the two containments; "containment" by how much of
    the query is contained, the right key for an incomplete or contaminated query.  Equal values go to the subject that
    shares more hashes, then to the one whose md5 sorts first.

    * ``<method>_search_hits.tsv``: ``#query subject rank identity query_cov shared_hashes query_hashes subject_hashes``,
      a row per hit among a query's ``top`` with identity >= ``min_identity`` and query_cov >= ``cov_min`` (the
      thresholds filter the top hits; they do not look further down the ranking); ``rank`` is the hit's rank before that;
    * ``<method>_search_queries.tsv``: ``#query md5 length hashes best_subject best_identity best_query_cov hits``, a row
      per query; ``best_*`` is rank 1 whatever the thresholds say, ``NA`` when the query shares no hash with any subject.

    Subjects are labelled by ``label``, queries by their file stem; floats as ``repr``.  Like ``run_sourmash_hip`` this
    needs the device for sketching (``engine``, or ``engine_factory`` "module:callable", else the process's own).
    Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= search_mod.MAX_TOP:
        sourmash_hip.log_sys_exit(logger, f"Expected 1 to {search_mod.MAX_TOP} hits a query, not {top!r}")
    if rank not in search_mod.RANKS:
        sourmash_hip.log_sys_exit(logger, f"Unknown rank {rank!r}: expected one of {', '.join(search_mod.RANKS)}")
    for value, what in ((min_identity, "identity"), (cov_min, "query coverage")):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0 <= value <= 1:  # a NaN fails the comparison
            sourmash_hip.log_sys_exit(logger, f"The minimum {what} must be a number from 0 to 1, not {value!r}")
    query_names = check_fasta(logger, query_fasta)
    outdir = reports._make_outdir(logger, outdir)
    conn, run = _open_run(logger, database, run_id, "Searching")
    config = run.configuration
    if config.method != sourmash_hip.METHOD:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run.run_id} is a {config.method} run: search-run needs the sketches of a {sourmash_hip.METHOD} run")
    reports._require_genomes(logger, run)
    mapping = reports._label_mapping(logger, run, label)
    reports._require_distinct_stems(logger, label, mapping)
    conn.close()
    if engine is None and engine_factory:
        module, _, attr = engine_factory.partition(":")
        engine = getattr(importlib.import_module(module), attr)()
    cache_dir = _work_dir(Path(tempfile.mkdtemp(prefix="pyani_hip_cache_", dir=_work_dir(temp))) if temp and not cache else cache, "pyani_hip_cache_")
    for _ in sourmash_hip.prepare_genomes(logger, run, cache_dir, engine=engine):
        pass
    kmersize, scaled = int(config.kmersize), sourmash_hip.parse_scaled(config.extra)
    subjects = sorted(a.genome_hash for a in run.fasta_hashes)  # a subject's index: its place among the run's md5, as in the run's matrices
    sig_dir = sourmash_hip.sig_cache_dir(cache_dir, config.kmersize, config.extra)
    subject_sketches = sourmash_hip.read_cached_sketches(logger, [sig_dir / f"{h}.sig" for h in subjects], kmersize, max_hash_for_scaled(scaled))
    queries: list[tuple[str, str, int, np.ndarray]] = []  # stem, md5, length, sketch
    try:
        for batch_paths, infos, sketches in sourmash_hip.sketch_fasta_batches(logger, query_names, kmersize=kmersize, scaled=scaled, engine=engine):
            queries += [(filename_stem(path.name), info.md5, info.length, mins) for path, info, mins in zip(batch_paths, infos, sketches)]
        hits = search_mod.search(subject_sketches, [q[3] for q in queries], kmersize, top=top, rank=rank, engine=engine)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "search-run", err)
    except ValueError as err:  # a genome too short for a single hash
        sourmash_hip.log_sys_exit(logger, f"search-run: {err}")
    written = search_mod.write_tables(outdir, config.method, hits, [q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries],
                                      [mapping[h] for h in subjects], min_identity=float(min_identity), cov_min=float(cov_min))  # fmt: skip
    logger.info("Wrote the hits of %d queries among %d genomes of run-id %d to %s", len(queries), len(subjects), run.run_id, outdir)
    return written


# ------------------------------------------------------------------ the driver as a process
_LABEL_OPTION = dict(choices=("md5", "filename", "stem"), default="stem")  # noqa: C408  every ``--label``
_MISSING_OPTION = ("--missing", {"type": float, "default": 1.0, "help": "distance of a pair with no identity in either direction (default 1.0)"})


def _device_option(p, what: str) -> None:
    p.add_argument("--device", type=int, default=None, help=f"{what} on this GPU (default: on the host)")


def _report_parser(sub, name: str, help_: str, *, run_id: bool = True, label: bool = True, own=(), formats=None, more=(), device=None) -> None:  # noqa: PLR0913
    """The subparser of a report command, its options in the order ``--help`` lists them: database, output directory,
    ``--run-id``, ``--label``, its ``own`` options (pairs of a flag and ``add_argument``'s keywords), ``--formats`` (given
    as what ``tsv`` and what an image format write), ``more`` of its own, ``--device`` (given as what then runs on the GPU)."""
    p = sub.add_parser(name, help=help_)
    p.add_argument("--database", "-d", required=True, type=Path)
    p.add_argument("--outdir", "-o", required=True, type=Path)
    if run_id:
        p.add_argument("--run-id", type=int, default=None)
    if label:
        p.add_argument("--label", **_LABEL_OPTION)
    for flag, keywords in own:
        p.add_argument(flag, **keywords)
    if formats:
        p.add_argument("--formats", type=lambda text: tuple(f for f in text.split(",") if f), default="tsv",
                       help=f"comma separated: tsv for {formats[0]}, png, pdf, svg or jpg for {formats[1]} (matplotlib)")  # fmt: skip
    for flag, keywords in more:
        p.add_argument(flag, **keywords)
    if device:
        _device_option(p, device)
    p.add_argument("--verbose", "-v", action="store_true")


@contextlib.contextmanager
def _device_engine(device: int | None):
    """A ``HipEngine`` on GPU ``device`` (None: none), closed on the way out."""
    engine = None if device is None else HipEngine(device)
    try:
        yield engine
    finally:
        if engine is not None:
            engine.close()


_COMMANDS = {  # subcommand -> its call from (the parsed arguments, the engine of ``--device`` or None, the logger)
    "sourmash": lambda a, _engine, logger: run_sourmash_hip(a.fasta, a.database, cache=a.cache, name=a.name, kmersize=a.kmersize, scaled=a.scaled,
                                                            temp=a.temp, logger=logger, ingest=a.ingest, gpus=a.gpus, engine_factory=a.engine_factory),
    "fastani": lambda a, _engine, logger: run_fastani_hip(a.fasta, a.database, name=a.name, kmersize=a.kmersize, fragsize=a.fragsize, minmatch=a.minmatch, temp=a.temp,
                                                          logger=logger, ingest=a.ingest, gpus=a.gpus, engine_factory=a.engine_factory, query_batch=a.query_batch),
    "external-alignment": lambda a, _engine, logger: run_external_alignment_hip(a.fasta, a.database, alignment=a.alignment, label=a.label, name=a.name,
                                                                                temp=a.temp, logger=logger, gpus=a.gpus),
    "tetra": lambda a, engine, logger: run_tetra_hip(a.fasta, a.database, cache=a.cache, name=a.name, temp=a.temp, logger=logger, engine=engine, gpus=a.gpus),
    "resume": lambda a, _engine, logger: resume(a.database, run_id=a.run_id, cache=a.cache, temp=a.temp, logger=logger, ingest=a.ingest, gpus=a.gpus,
                                                engine_factory=a.engine_factory),
    "export-run": lambda a, _engine, logger: export_run(a.database, a.outdir, run_id=a.run_id, label=a.label, logger=logger),
    "classify": lambda a, engine, logger: classify(a.database, a.outdir, run_id=a.run_id, label=a.label, coverage_edges=a.coverage_edges,
                                                   score_edges=a.score_edges, cov_min=a.cov_min, mode=a.mode, engine=engine, logger=logger),
    "plot-run": lambda a, engine, logger: plot_run(a.database, a.outdir, run_id=a.run_id, label=a.label, formats=a.formats, engine=engine, logger=logger,
                                                   distributions=a.distributions, scatter=a.scatter, scatter_bins=a.scatter_bins),
    "plot-run-comp": lambda a, engine, logger: plot_run_comp(a.database, a.outdir, a.run_ids, columns=a.columns, formats=a.formats, engine=engine, logger=logger),
    "tree-run": lambda a, engine, logger: tree_run(a.database, a.outdir, run_id=a.run_id, label=a.label, method=a.method, missing=a.missing, engine=engine,
                                                   logger=logger),
    "bootstrap-run": lambda a, engine, logger: bootstrap_run(a.database, a.outdir, run_id=a.run_id, label=a.label, replicates=a.replicates, seed=a.seed,
                                                             missing=a.missing, alignment=a.alignment, keep_trees=a.keep_trees, engine=engine, logger=logger),
    "phylo-run": lambda a, engine, logger: phylo_run(a.database, a.outdir, run_id=a.run_id, label=a.label, model=a.model, missing=a.missing, replicates=a.replicates,
                                                     seed=a.seed, alignment=a.alignment, keep_trees=a.keep_trees, engine=engine, logger=logger),
    "ordinate-run": lambda a, engine, logger: ordinate_run(a.database, a.outdir, run_id=a.run_id, label=a.label, dimensions=a.dimensions, missing=a.missing,
                                                           formats=a.formats, engine=engine, logger=logger),
    "mantel-run-comp": lambda a, engine, logger: mantel_run_comp(a.database, a.outdir, a.run_ids, permutations=a.permutations, seed=a.seed, missing=a.missing,
                                                                 engine=engine, logger=logger),
    "dereplicate-run": lambda a, engine, logger: dereplicate_run(a.database, a.outdir, run_id=a.run_id, label=a.label, min_identity=a.min_identity,
                                                                 cov_min=a.cov_min, score_edges=a.score_edges, coverage_edges=a.coverage_edges, mode=a.mode,
                                                                 prefer=a.prefer, engine=engine, logger=logger),
    "search-run": lambda a, _engine, logger: search_run(a.query_fasta, a.database, a.outdir, run_id=a.run_id, cache=a.cache, label=a.label, top=a.top, rank=a.rank,
                                                        min_identity=a.min_identity, cov_min=a.cov_min, temp=a.temp, engine_factory=a.engine_factory, logger=logger),
}  # fmt: skip


def main(argv: list[str] | None = None) -> int:
    """``python -m pyani_plus_amd.rundb {sourmash,fastani,external-alignment,tetra,resume,export-run,classify,plot-run,plot-run-comp,tree-run,bootstrap-run,phylo-run,ordinate-run,mantel-run-comp,dereplicate-run,search-run} ...``: the run driver as a process of its own,
    with SIGINT and SIGTERM arriving as ``KeyboardInterrupt`` the way the reference's worker command arranges it
    (pyani_plus/private_cli.py:816-823), so that ``scancel`` / ``kill`` leave the finished batches recorded and the run
    marked "Worker interrupted" exactly as Ctrl-C does.  Only what the drivers above take as arguments; the reference's
    Typer front end is out of scope."""
    parser = argparse.ArgumentParser(prog="python -m pyani_plus_amd.rundb", description=main.__doc__)
    sub = parser.add_subparsers(dest="command", required=True)

    def common(p, *, run_options: bool) -> None:
        p.add_argument("--database", "-d", required=True, type=Path)
        p.add_argument("--temp", type=Path, default=None)
        p.add_argument("--gpus", type=int, default=1)
        p.add_argument("--ingest", choices=("json", "direct"), default="json")
        p.add_argument("--engine-factory", default=None, help="module:callable that makes the engine (tests)")
        p.add_argument("--verbose", "-v", action="store_true")
        if run_options:
            p.add_argument("fasta", type=Path)
            p.add_argument("--name", default=None)

    p_s = sub.add_parser("sourmash", help="FASTA directory -> all N^2 sourmash-hip comparisons")
    common(p_s, run_options=True)
    p_s.add_argument("--cache", type=Path, default=None)
    p_s.add_argument("--kmersize", type=int, default=sourmash_hip.KMER_SIZE)
    p_s.add_argument("--scaled", type=int, default=sourmash_hip.SCALED)
    p_f = sub.add_parser("fastani", help="FASTA directory -> all N^2 fastANI-hip comparisons")
    common(p_f, run_options=True)
    p_f.add_argument("--kmersize", type=int, default=None)
    p_f.add_argument("--fragsize", type=int, default=None)
    p_f.add_argument("--minmatch", type=float, default=None)
    p_f.add_argument("--query-batch", type=int, default=None)
    p_x = sub.add_parser("external-alignment", help="FASTA directory + its MSA -> all N^2 external-alignment-hip comparisons")
    common(p_x, run_options=True)
    p_x.add_argument("--alignment", required=True, type=Path, help="FASTA MSA of the genomes, one row per genome")
    p_x.add_argument("--label", **_LABEL_OPTION)
    p_t = sub.add_parser("tetra", help="FASTA directory -> all N^2 TETRA-hip comparisons (tetranucleotide Z-score correlations)")
    common(p_t, run_options=True)
    p_t.add_argument("--cache", type=Path, default=None)
    _device_option(p_t, "count and correlate")
    p_r = sub.add_parser("resume", help="complete a partial run")
    common(p_r, run_options=False)
    p_r.add_argument("--run-id", type=int, default=None)
    p_r.add_argument("--cache", type=Path, default=None)
    _report_parser(sub, "export-run", "long form and matrices of a run as TSV files")
    _report_parser(sub, "classify", "the genome cliques of a complete run as <method>_classify.tsv", device="build and sort the edge list", own=(
        ("--coverage-edges", {"choices": classify_mod.AGG_NAMES, "default": "min"}),
        ("--score-edges", {"choices": classify_mod.AGG_NAMES, "default": "mean"}),
        ("--cov-min", {"type": float, "default": classify_mod.MIN_COVERAGE}),
        ("--mode", {"choices": classify_mod.MODES, "default": "identity"}),
    ))  # fmt: skip
    _report_parser(sub, "plot-run", "the clustered heatmap tables and the scatter tables of a complete run", formats=("the tables", "the heatmap figures"),
                   device="compute the row distances, the distributions and the scatter rasters", more=(
        ("--distributions", {"action": "store_true", "help": "also each score's distribution: histogram and density tables, and the figure with an image format"}),
        ("--scatter", {"action": "store_true", "help": "also the two scatter figures (identity against query coverage and tANI) as rasters: their grid and margin tables, and the figure with an image format"}),
        ("--scatter-bins", {"type": int, "default": scatter_mod.GRID, "help": "cells per axis of a scatter figure's raster, 1 to 1024 (default 256)"}),
    ))  # fmt: skip
    _report_parser(sub, "plot-run-comp", "the identities of further runs against a reference run's, pair by pair", run_id=False, label=False,
                   formats=("the tables", "the two figures"), device="join the runs and take the histograms", own=(
        ("--run-ids", {"required": True, "help": "comma separated list of runs, the reference run first"}),
        ("--columns", {"type": int, "default": 0, "help": "panels per row of the figures (default 0: a square tiling)"}),
    ))  # fmt: skip
    _report_parser(sub, "tree-run", "the neighbour-joining or UPGMA tree of a complete run as <method>_identity_<nj|upgma>.nwk",
                   device="make the joins of neighbour joining", own=(("--method", {"choices": tree_mod.METHODS, "default": "nj"}), _MISSING_OPTION))
    _report_parser(sub, "bootstrap-run", "column-bootstrap support of tree-run's neighbour-joining tree, for a complete external-alignment-hip run",
                   device="make the weighted counts, the distances and the joins", own=(
        ("--replicates", {"type": int, "default": 100, "help": "bootstrap replicates, 1 to 100000 (default 100)"}),
        ("--seed", {"type": int, "default": 0, "help": "seed of the column draws, 0 to 2^64 - 1 (default 0)"}),
        _MISSING_OPTION,
        ("--alignment", {"type": Path, "default": None, "help": "the run's alignment (default: the configuration's file next to the database)"}),
        ("--keep-trees", {"action": "store_true", "help": "also write the replicate trees, one per line"}),
    ))  # fmt: skip
    _report_parser(sub, "phylo-run", "p, JC69 or K80 distances of a complete external-alignment-hip run from its alignment, their neighbour-joining tree and its bootstrap",
                   device="make the counts, the distances and the joins", own=(
        ("--model", {"choices": substitution_mod.MODELS[::-1], "default": substitution_mod.DEFAULT_MODEL, "help": "the substitution model (default k80)"}),
        ("--missing", {"type": float, "default": substitution_mod.DEFAULT_MISSING,
                       "help": "distance of a pair without a shared nucleotide column or too diverged for the model (default 3.0)"}),
        ("--replicates", {"type": int, "default": 0, "help": "bootstrap replicates, 0 to 100000 (default 0: no bootstrap)"}),
        ("--seed", {"type": int, "default": 0, "help": "seed of the column draws, 0 to 2^64 - 1 (default 0)"}),
        ("--alignment", {"type": Path, "default": None, "help": "the run's alignment (default: the configuration's file next to the database)"}),
        ("--keep-trees", {"action": "store_true", "help": "also write the replicate trees, one per line"}),
    ))  # fmt: skip
    _report_parser(sub, "ordinate-run", "the principal coordinates of a complete run as <method>_identity_pcoa.tsv and its eigenvalue table",
                   formats=("the two tables", "the figure"), device="centre the matrix and do the solver's products",
                   own=(("--dimensions", {"type": int, "default": 3, "help": "principal axes to compute (default 3)"}), _MISSING_OPTION))
    _report_parser(sub, "mantel-run-comp", "Mantel's permutation test of further complete runs against a reference run, over the genomes they share",
                   run_id=False, label=False, device="make the cross sums", own=(
        ("--run-ids", {"required": True, "help": "comma separated list of runs, the reference run first"}),
        ("--permutations", {"type": int, "default": 9999, "help": "permutations of the other run's genomes, 0 to 1000000 (default 9999)"}),
        ("--seed", {"type": int, "default": 0, "help": "seed of the permutations, 0 to 2^64 - 1 (default 0)"}),
        _MISSING_OPTION,
    ))  # fmt: skip
    _report_parser(sub, "dereplicate-run", "one representative genome per group of a complete run as <method>_dereplicate.tsv and <method>_representatives.tsv",
                   device="build the graph, select and assign", own=(
        ("--min-identity", {"type": float, "default": dereplicate_mod.MIN_IDENTITY, "help": "two genomes are adjacent from this aggregated identity on (default 0.95)"}),
        ("--cov-min", {"type": float, "default": classify_mod.MIN_COVERAGE, "help": "... and above this aggregated query coverage (default 0.5)"}),
        ("--score-edges", {"choices": classify_mod.AGG_NAMES, "default": "mean"}),
        ("--coverage-edges", {"choices": classify_mod.AGG_NAMES, "default": "min"}),
        ("--mode", {"choices": dereplicate_mod.MODES, "default": "greedy", "help": "greedy: keep a genome that no kept genome is adjacent to; cover: greedy dominating set"}),
        ("--prefer", {"choices": dereplicate_mod.PREFERENCES, "default": "length", "help": "the order of preference: the longer genome first (ties by label), or label order"}),
    ))  # fmt: skip
    _report_parser(sub, "search-run", "the nearest genomes of a sourmash-hip run for the genomes of a FASTA directory as <method>_search_hits.tsv and <method>_search_queries.tsv", own=(
        ("query_fasta", {"type": Path, "metavar": "QUERY_FASTA", "help": "directory of the genomes to look up; they are not added to the run"}),
        ("--cache", {"type": Path, "default": None, "help": "the run's .sig cache (default: a temporary one, so every genome of the run is sketched again)"}),
        ("--top", {"type": int, "default": search_mod.TOP, "help": "hits kept per query, 1 to 64 (default 5)"}),
        ("--rank", {"choices": search_mod.RANKS, "default": "identity",
                    "help": "identity: the larger of the two containments, the run's own identity; containment: how much of the query is contained"}),
        ("--min-identity", {"type": float, "default": 0.0, "help": "write a hit only from this identity on (default 0.0); this filters the top hits and does not look further down the ranking"}),
        ("--cov-min", {"type": float, "default": 0.0, "help": "... and from this query coverage on (default 0.0), in the same way"}),
        ("--temp", {"type": Path, "default": None}),
        ("--engine-factory", {"default": None, "help": "module:callable that makes the engine (tests)"}),
    ))  # fmt: skip
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO, format="%(levelname)s %(message)s")
    logger = logging.getLogger("pyani_plus_amd")
    with launch.signals_as_interrupt(), _device_engine(getattr(args, "device", None)) as engine:
        result = _COMMANDS[args.command](args, engine, logger)
        if isinstance(result, Run):
            logger.info("run-id %d: %s", result.run_id, result.status)
        else:  # a report: the path it wrote, or the paths
            for path in [result] if isinstance(result, Path) else result:
                print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
