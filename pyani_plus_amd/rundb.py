"""Run driver and persistence for the four methods ``sourmash-hip``, ``fastANI-hip``, ``external-alignment-hip`` and
``TETRA-hip`` (stdlib ``sqlite3``).

The reference's Python (Typer CLI, SQLAlchemy ORM, snakemake) does not travel to the GPU
box, so this module is the build's own counterpart of ``cli_sourmash`` / ``fastani`` / ``external_alignment`` +
``start_and_run_method`` + ``run_method`` minus snakemake (pyani_plus/public_cli.py:115-329, 502-554,
598-699), of ``resume``, ``export-run``, ``plot-run`` and ``plot-run-comp`` (their tables; pyani_plus/plot_run.py) and ``classify``
(702-828, 974-1091, 1095-1208, 1211-1331) and of the parts of ``db_orm`` they use (SURVEY.md
section 8b, last row):

* FASTA enumeration by the four extensions +- ``.gz`` (pyani_plus/utils.py:226-242)
* genome identity = md5 of the decompressed bytes (utils.py:142-196); length = sum of
  residues, description = first title (db_orm.py:832-866); duplicate md5 aborts
  (public_cli.py:165-171)
* the same tables / constraints as ``Base.metadata.create_all``
* JSON column import with INSERT OR IGNORE (private_cli.py:507-614, db_orm.py:1076)
* ``cache_comparisons``: N x N matrices over sorted md5, pandas ``to_json(orient="split")``
  (db_orm.py:393-466) -- built without the reference's O(N^3) ``hashes.index`` loop.

Every run takes the same steps: register the genomes, record the run, find what the database lacks
(``_begin_missing``), compute it (the method's ``_compute_missing_<method>``, listed in ``_METHODS``) and finish
(``_finish_run``); ``_RunState`` carries what the steps share.

Databases written here can be opened by the reference and vice versa.
"""

from __future__ import annotations

import argparse
import ctypes as C
import datetime
import enum
import hashlib
import importlib
import logging
import math
import os
import platform
import sqlite3
import sys
import tempfile
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from io import StringIO
from pathlib import Path

import numpy as np

from . import _capi, launch, wire
from . import classify as classify_mod
from . import cluster as cluster_mod
from . import distribution as distribution_mod
from . import distribution_figure, heatmap_figure, ordination_figure, run_comp_figure, scatter_figure
from . import ordination as ordination_mod
from . import run_comp as run_comp_mod
from . import scatter as scatter_mod
from . import tree as tree_mod
from ._capi import HipBackendError
from .distributed import shard_bounds_by_cost
from .engine import load_fasta_files
from .methods import external_alignment_hip, fastani_hip, sourmash_hip, tetra_hip
from .methods.external_alignment_hip import filename_stem  # also reached as ``rundb.filename_stem``

FASTA_EXTENSIONS = {".fasta", ".fas", ".fna", ".fa"}  # pyani_plus/__init__.py:48

SCHEMA = """
CREATE TABLE IF NOT EXISTS genomes (
    genome_hash VARCHAR NOT NULL, path VARCHAR NOT NULL, length INTEGER NOT NULL, description VARCHAR NOT NULL,
    CONSTRAINT pk_genomes PRIMARY KEY (genome_hash));
CREATE TABLE IF NOT EXISTS configurations (
    configuration_id INTEGER NOT NULL, method VARCHAR NOT NULL, program VARCHAR NOT NULL, version VARCHAR NOT NULL,
    fragsize INTEGER, mode VARCHAR, kmersize INTEGER, minmatch FLOAT, extra VARCHAR,
    CONSTRAINT pk_configurations PRIMARY KEY (configuration_id),
    CONSTRAINT uq_configurations_method UNIQUE (method, program, version, fragsize, mode, kmersize, minmatch, extra));
CREATE TABLE IF NOT EXISTS comparisons (
    comparison_id INTEGER NOT NULL, query_hash VARCHAR NOT NULL, subject_hash VARCHAR NOT NULL,
    configuration_id INTEGER NOT NULL, identity FLOAT, aln_length INTEGER, sim_errors INTEGER, cov_query FLOAT,
    cov_subject FLOAT, uname_system VARCHAR NOT NULL, uname_release VARCHAR NOT NULL, uname_machine VARCHAR NOT NULL,
    CONSTRAINT pk_comparisons PRIMARY KEY (comparison_id),
    CONSTRAINT uq_comparisons_query_hash UNIQUE (query_hash, subject_hash, configuration_id),
    CONSTRAINT fk_comparisons_query_hash_genomes FOREIGN KEY(query_hash) REFERENCES genomes (genome_hash),
    CONSTRAINT fk_comparisons_subject_hash_genomes FOREIGN KEY(subject_hash) REFERENCES genomes (genome_hash),
    CONSTRAINT fk_comparisons_configuration_id_configurations FOREIGN KEY(configuration_id)
        REFERENCES configurations (configuration_id));
CREATE TABLE IF NOT EXISTS runs (
    run_id INTEGER NOT NULL, configuration_id INTEGER NOT NULL, cmdline VARCHAR NOT NULL,
    fasta_directory VARCHAR NOT NULL, date DATETIME NOT NULL, status VARCHAR NOT NULL, name VARCHAR NOT NULL,
    df_identity VARCHAR, df_cov_query VARCHAR, df_aln_length VARCHAR, df_sim_errors VARCHAR, df_hadamard VARCHAR,
    CONSTRAINT pk_runs PRIMARY KEY (run_id),
    CONSTRAINT fk_runs_configuration_id_configurations FOREIGN KEY(configuration_id)
        REFERENCES configurations (configuration_id));
CREATE TABLE IF NOT EXISTS runs_genomes (
    genome_hash VARCHAR NOT NULL, run_id INTEGER NOT NULL, fasta_filename VARCHAR NOT NULL,
    CONSTRAINT pk_runs_genomes PRIMARY KEY (genome_hash, run_id),
    CONSTRAINT fk_runs_genomes_genome_hash_genomes FOREIGN KEY(genome_hash) REFERENCES genomes (genome_hash),
    CONSTRAINT fk_runs_genomes_run_id_runs FOREIGN KEY(run_id) REFERENCES runs (run_id));
"""


# ------------------------------------------------------------------ plain-object mirrors of the ORM rows
@dataclass
class Configuration:
    configuration_id: int
    method: str
    program: str
    version: str
    fragsize: int | None = None
    mode: str | None = None
    kmersize: int | None = None
    minmatch: float | None = None
    extra: str | None = None


@dataclass
class RunGenomeAssociation:
    genome_hash: str
    fasta_filename: str


@dataclass
class Run:
    """Duck-type of ``db_orm.Run`` as far as the method module reads it."""

    run_id: int
    configuration: Configuration
    fasta_directory: str
    fasta_hashes: list[RunGenomeAssociation]
    status: str
    name: str = ""

    @property
    def configuration_id(self) -> int:
        return self.configuration.configuration_id


class Session:
    """Minimal session: ``commit()`` persists ``run.status`` (what the worker's interrupt path needs)."""

    def __init__(self, conn: sqlite3.Connection, run: Run | None = None):
        self.conn = conn
        self.run = run

    def commit(self) -> None:
        if self.run is not None:
            self.conn.execute("UPDATE runs SET status=? WHERE run_id=?", (self.run.status, self.run.run_id))
        self.conn.commit()


# ------------------------------------------------------------------ FASTA bookkeeping
def check_fasta(logger: logging.Logger, fasta: Path) -> list[Path]:
    """FASTA files of a directory by extension (pyani_plus/utils.py:226-242)."""
    fasta = Path(fasta)
    if not fasta.is_dir():
        sourmash_hip.log_sys_exit(logger, f"FASTA input {fasta} is not a directory")
    names: list[Path] = []
    for ext in sorted(FASTA_EXTENSIONS):
        names.extend(fasta.glob("*" + ext))
        names.extend(fasta.glob("*" + ext + ".gz"))
    if not names:
        sourmash_hip.log_sys_exit(
            logger, f"No FASTA input genomes under {fasta} with extensions {', '.join(sorted(FASTA_EXTENSIONS))}"
        )
    return sorted(names)


def fasta_length_and_description(text: bytes) -> tuple[int, str | None]:
    """Sum of residues and first title, as fasta_bytes_iterator sees them (utils.py:67-90)."""
    length = 0
    description = None
    in_record = False
    for line in text.split(b"\n"):
        if line[:1] == b">":
            in_record = True
            if description is None:
                description = line[1:].rstrip().decode()
            continue
        if in_record:
            length += len(line.translate(None, b" \t\r\n"))
    return length, description


# ------------------------------------------------------------------ database
def connect_to_db(database: Path | str) -> sqlite3.Connection:
    conn = sqlite3.connect(str(database), timeout=30.0)
    conn.executescript(SCHEMA)
    conn.commit()
    return conn


def _find_configuration(conn, values: tuple):
    """The (configuration_id,) row with these values of ``wire.CONFIG_FIELDS``, or None."""
    return conn.execute(
        "SELECT configuration_id FROM configurations WHERE method=? AND program=? AND version=? AND fragsize IS ? "
        "AND mode IS ? AND kmersize IS ? AND minmatch IS ? AND extra IS ?",
        values,
    ).fetchone()


def db_configuration(conn, method, program, version, fragsize=None, mode=None, kmersize=None, minmatch=None,
                     extra=None) -> Configuration:
    """Return the matching configuration row, creating it if needed (db_orm.py:705-782)."""
    row = _find_configuration(conn, (method, program, version, fragsize, mode, kmersize, minmatch, extra))
    if row is None:
        cur = conn.execute(
            "INSERT INTO configurations (method, program, version, fragsize, mode, kmersize, minmatch, extra) "
            "VALUES (?,?,?,?,?,?,?,?)",
            (method, program, version, fragsize, mode, kmersize, minmatch, extra),
        )
        conn.commit()
        cid = cur.lastrowid
    else:
        cid = row[0]
    return Configuration(cid, method, program, version, fragsize, mode, kmersize, minmatch, extra)


def db_genome(conn, path: Path, md5: str, length: int, description: str) -> None:
    conn.execute(
        "INSERT OR IGNORE INTO genomes (genome_hash, path, length, description) VALUES (?,?,?,?)",
        (md5, str(path), length, description),
    )


def add_run(conn, config: Configuration, cmdline: str, fasta_directory: Path, status: str, name: str,
            fasta_to_hash: dict[Path, str]) -> Run:
    now = datetime.datetime.now(datetime.timezone.utc).replace(tzinfo=None).isoformat(sep=" ")
    cur = conn.execute(
        "INSERT INTO runs (configuration_id, cmdline, fasta_directory, date, status, name) VALUES (?,?,?,?,?,?)",
        (config.configuration_id, cmdline, str(fasta_directory), now, status, name),
    )
    run_id = cur.lastrowid
    assoc = []
    for filename, md5 in fasta_to_hash.items():
        conn.execute(
            "INSERT INTO runs_genomes (genome_hash, run_id, fasta_filename) VALUES (?,?,?)",
            (md5, run_id, Path(filename).name),
        )
        assoc.append(RunGenomeAssociation(md5, Path(filename).name))
    conn.commit()
    return Run(run_id, config, str(fasta_directory), assoc, status, name)


def load_run(conn, run_id: int) -> Run:
    row = conn.execute(
        "SELECT configuration_id, fasta_directory, status, name FROM runs WHERE run_id=?", (run_id,)
    ).fetchone()
    if row is None:
        msg = f"Database has no run {run_id}"
        raise ValueError(msg)
    crow = conn.execute(
        "SELECT configuration_id, method, program, version, fragsize, mode, kmersize, minmatch, extra "
        "FROM configurations WHERE configuration_id=?",
        (row[0],),
    ).fetchone()
    assoc = [
        RunGenomeAssociation(h, f)
        for h, f in conn.execute("SELECT genome_hash, fasta_filename FROM runs_genomes WHERE run_id=?", (run_id,))
    ]
    return Run(run_id, Configuration(*crow), row[1], assoc, row[2], row[3])


def _open_run(logger, database: Path | str, run_id: int | None, doing: str) -> tuple[sqlite3.Connection, Run]:
    """The database and its run ``run_id`` (None: the latest one), with the reference's messages
    (pyani_plus/public_cli.py:718-741)."""
    conn = connect_to_db(database)
    if run_id is None:
        row = conn.execute("SELECT MAX(run_id) FROM runs").fetchone()
        if row is None or row[0] is None:
            sourmash_hip.log_sys_exit(logger, f"Database {database} contains no runs.")
        run_id = row[0]
        logger.info("%s run-id %d", doing, run_id)
    try:
        return conn, load_run(conn, run_id)
    except ValueError:
        sourmash_hip.log_sys_exit(logger, f"Database {database} has no run-id {run_id}.")


def _select_run_comparisons(conn, run: Run, what: str, tail: str = "") -> sqlite3.Cursor:
    """``what`` of the comparisons among this run's genomes under its configuration (Run.comparisons(),
    db_orm.py:353-391)."""
    return conn.execute(
        f"SELECT {what} FROM comparisons c "
        "JOIN runs_genomes q ON c.query_hash = q.genome_hash AND q.run_id = ? "
        "JOIN runs_genomes s ON c.subject_hash = s.genome_hash AND s.run_id = ? "
        f"WHERE c.configuration_id = ? {tail}",
        (run.run_id, run.run_id, run.configuration_id),
    )


def count_run_comparisons(conn, run: Run) -> int:
    return _select_run_comparisons(conn, run, "COUNT(*)").fetchone()[0]


INSERT_COMPARISON = (
    "INSERT OR IGNORE INTO comparisons (query_hash, subject_hash, configuration_id, identity, aln_length, "
    "sim_errors, cov_query, uname_system, uname_release, uname_machine) VALUES (?,?,?,?,?,?,?,?,?,?)"
)


def import_json_comparisons(logger: logging.Logger, conn, json_filename: Path) -> int:
    """Import one column file; the configuration must already exist; ``cov_subject`` is ignored
    (pyani_plus/private_cli.py:507-614)."""
    data = wire.load_json_comparisons(json_filename)
    cfg = data["configuration"]
    row = _find_configuration(conn, tuple(cfg[k] for k in wire.CONFIG_FIELDS))
    if row is None:
        sourmash_hip.log_sys_exit(logger, f"JSON file {json_filename} configuration not in database")
    cid = row[0]
    uname = data["uname"]
    rows = [
        (
            e["query_hash"], e["subject_hash"], cid, e["identity"], e.get("aln_length"), e.get("sim_errors"),
            e.get("cov_query"), uname["system"], uname["release"], uname["machine"],
        )  # fmt: skip
        for e in data["comparisons"]
    ]
    conn.executemany(INSERT_COMPARISON, rows)
    conn.commit()
    return len(rows)


def _database_file(conn) -> str | None:
    """Path of the connection's main database, or None for an in-memory / temporary one."""
    for _seq, name, path in conn.execute("PRAGMA database_list"):
        if name == "main":
            return path or None
    return None


def ingest_matrices_native(conn, run: Run, queries: list[str], subjects: list[str], identity, cov_query, is_null, *,
                           aln_length=None, sim_errors=None) -> int | None:
    """``ingest_matrices`` through ``pa_sqlite_insert_comparisons`` (one prepared statement stepped from C on a
    connection of its own).  Returns the number of comparisons handled, or None when the native route does not
    apply (in-memory database, libsqlite3.so.0 not loadable) -- the caller then uses Python's sqlite3 module."""
    path = _database_file(conn)
    if path is None:
        return None
    nq, ns = len(queries), len(subjects)
    if nq == 0 or ns == 0:
        return 0
    uname = platform.uname()
    identity = np.ascontiguousarray(identity, dtype=np.float64)
    cov_query = np.ascontiguousarray(cov_query, dtype=np.float64)
    null = np.ascontiguousarray(is_null, dtype=np.uint8)
    assert identity.shape == (nq, ns) == cov_query.shape == null.shape
    q_arr = (C.c_char_p * nq)(*[q.encode() for q in queries])
    s_arr = (C.c_char_p * ns)(*[s.encode() for s in subjects])
    conn.commit()  # the call opens its own connection: nothing of ours may hold the write lock
    inserted = C.c_uint64()
    aln = err = None
    if aln_length is not None:
        aln = np.ascontiguousarray(aln_length, dtype=np.int64)
        err = np.ascontiguousarray(sim_errors, dtype=np.int64)
        assert aln.shape == (nq, ns) == err.shape
    status = _capi.load_library().pa_sqlite_insert_comparisons_ex(
        path.encode(), run.configuration_id, uname.system.encode(), uname.release.encode(), uname.machine.encode(),
        q_arr, nq, s_arr, ns, identity.ctypes.data, cov_query.ctypes.data, null.ctypes.data,
        None if aln is None else aln.ctypes.data, None if err is None else err.ctypes.data, C.byref(inserted),
    )  # fmt: skip
    if status == _capi.PA_E_IO and "libsqlite3" in _capi.last_error():
        return None
    _capi.check(status, "pa_sqlite_insert_comparisons")
    return nq * ns


def ingest_matrices(conn, run: Run, queries: list[str], subjects: list[str], identity, cov_query, is_null, *,
                    chunk_rows: int = 1_000_000, native: bool = True, aln_length=None, sim_errors=None) -> int:
    """Comparison rows straight from the result matrices (the reference goes through one
    Python dict per row, a JSON file and its re-parse: pyani_plus/private_cli.py:1863-1888, 507-614).

    Rows go in query-major with ascending subjects -- the order of the UNIQUE(query_hash, subject_hash,
    configuration_id) index when both lists are sorted, so the index grows by appends.  With ``native`` the rows
    are stepped from C (``ingest_matrices_native``); otherwise, or when that route does not apply, in chunks of
    ``chunk_rows`` through one ``executemany`` each."""
    if native:
        done = ingest_matrices_native(conn, run, queries, subjects, identity, cov_query, is_null, aln_length=aln_length, sim_errors=sim_errors)
        if done is not None:
            return done
    uname = platform.uname()
    cid = run.configuration_id
    nq, ns = len(queries), len(subjects)
    identity = np.asarray(identity, dtype=np.float64)
    cov_query = np.asarray(cov_query, dtype=np.float64)
    null = np.asarray(is_null, dtype=bool)
    rows_per_chunk = max(1, chunk_rows // max(ns, 1))
    constants = (uname.system, uname.release, uname.machine)
    for q0 in range(0, nq, rows_per_chunk):
        q1 = min(nq, q0 + rows_per_chunk)
        ident = identity[q0:q1].astype(object)
        cov = cov_query[q0:q1].astype(object)
        ident[null[q0:q1]] = None
        cov[null[q0:q1]] = None
        if aln_length is None:
            aln = err = np.full(ident.shape, None, dtype=object)
        else:
            aln = np.asarray(aln_length)[q0:q1].astype(np.int64).astype(object)  # Python ints: sqlite3 stores numpy scalars as blobs
            err = np.asarray(sim_errors)[q0:q1].astype(np.int64).astype(object)
            aln[null[q0:q1]] = None
            err[null[q0:q1]] = None
        rows = (
            (q, s, cid, i, a, e, c, *constants)
            for q, irow, crow, arow, erow in zip(queries[q0:q1], ident, cov, aln, err)
            for s, i, c, a, e in zip(subjects, irow, crow, arow, erow)
        )
        conn.executemany(INSERT_COMPARISON, rows)
    conn.commit()
    return nq * ns


def _matrices_to_json(hashes: list[str], mats: dict) -> dict[str, str]:
    """The five ``runs.df_*`` strings as pandas writes them (db_orm.py:442-465); hadamard = identity * cov_query."""
    import pandas as pd  # loaded when the first matrix cache is formatted, not with the module

    mats["hadamard"] = mats["identity"] * mats["cov_query"]
    return {
        f"df_{key}": pd.DataFrame(data=mat, index=hashes, columns=hashes, dtype=float).to_json(orient="split")
        for key, mat in mats.items()
    }


def format_matrix_cache(hashes: list[str], identity, cov_query, is_null, *, aln_length=None, sim_errors=None) -> dict[str, str] | None:
    """The five ``runs.df_*`` strings from matrices in memory (rows = query, columns = subject, both in ``hashes``
    order = sorted md5); None when they would not fit a SQLite value."""
    assert hashes == sorted(hashes)
    n = len(hashes)
    if _matrix_cache_too_big(n):
        return None
    ident = np.where(is_null, np.nan, identity)
    cov = np.where(is_null, np.nan, cov_query)
    nan = np.full((n, n), np.nan)
    aln = nan if aln_length is None else np.where(is_null, np.nan, np.asarray(aln_length, dtype=np.float64))
    err = nan if sim_errors is None else np.where(is_null, np.nan, np.asarray(sim_errors, dtype=np.float64))
    return _matrices_to_json(hashes, {"identity": ident, "cov_query": cov, "aln_length": aln, "sim_errors": err})


def cache_matrices(conn, run: Run, hashes: list[str], identity, cov_query, is_null, *, formatted=None) -> dict[str, str]:
    """``cache_comparisons`` from matrices that are already in memory: same strings as the SELECT-based form, without
    reading 10^8 rows back.  ``formatted`` = the result of an earlier ``format_matrix_cache`` of the same matrices."""
    out = formatted if formatted is not None else format_matrix_cache(hashes, identity, cov_query, is_null)
    _store_matrix_cache(conn, run, out)
    return out or {}


def _matrix_cache_too_big(n: int) -> bool:
    """A cached matrix is about 13 characters per cell ("0.9997081124,"): beyond ~7.5e7 cells its JSON text passes
    SQLite's 10^9-byte value limit, so formatting it would be wasted work."""
    return n * n * 13 > 950_000_000


def _store_matrix_cache(conn, run: Run, out: dict[str, str] | None) -> bool:
    """``runs.df_*`` hold the matrices as JSON text (db_orm.py:442-465).  SQLite refuses a value of more than
    10^9 bytes (SQLITE_MAX_LENGTH), which a 10 000 x 10 000 matrix exceeds (about 1.3 GB of text) -- in the
    reference just as here.  The comparisons table is complete either way; the cache columns then stay NULL, which
    the reference treats as "not cached yet" (db_orm.py:393-405)."""
    try:
        if out is None:
            raise sqlite3.DataError("not attempted")
        conn.execute(
            "UPDATE runs SET df_identity=?, df_cov_query=?, df_aln_length=?, df_sim_errors=?, df_hadamard=? WHERE run_id=?",
            (out["df_identity"], out["df_cov_query"], out["df_aln_length"], out["df_sim_errors"], out["df_hadamard"],
             run.run_id),
        )
    except (sqlite3.DataError, OverflowError) as err:
        logging.getLogger("pyani_plus_amd").warning(
            "matrix cache of run %d not stored (%s): %d genomes give JSON strings beyond SQLite's 10^9-byte limit",
            run.run_id, err, len(run.fasta_hashes),
        )
        conn.rollback()
        return False
    conn.commit()
    return True


def cache_comparisons(conn, run: Run) -> dict[str, str]:
    """Fill runs.df_* with the N x N matrices (rows = query, columns = subject, sorted md5)."""
    if _matrix_cache_too_big(len(run.fasta_hashes)):
        _store_matrix_cache(conn, run, None)
        return {}
    hashes, mats = _comparison_matrices(conn, run)
    out = _matrices_to_json(hashes, mats)
    _store_matrix_cache(conn, run, out)
    return out


def _comparison_matrices(conn, run: Run) -> tuple[list[str], dict]:
    """(sorted md5s, the four N x N matrices of the run's comparisons: rows = query, columns = subject, NaN where there
    is no value)."""
    hashes = sorted(a.genome_hash for a in run.fasta_hashes)
    index = {h: i for i, h in enumerate(hashes)}
    n = len(hashes)
    mats = {k: np.full((n, n), np.nan, float) for k in ("identity", "cov_query", "aln_length", "sim_errors")}
    rows = _select_run_comparisons(conn, run, "c.query_hash, c.subject_hash, c.identity, c.cov_query, c.aln_length, c.sim_errors").fetchall()
    if rows:
        # one dictionary lookup per row (the reference does a list.index per row: O(N^3) overall)
        r_idx = np.fromiter((index[r[0]] for r in rows), dtype=np.int64, count=len(rows))
        c_idx = np.fromiter((index[r[1]] for r in rows), dtype=np.int64, count=len(rows))
        for col, key in enumerate(("identity", "cov_query", "aln_length", "sim_errors"), start=2):
            mats[key][r_idx, c_idx] = np.array([r[col] for r in rows], dtype=float)  # None -> NaN
    return hashes, mats


def _load_tile(logger, tile_file: Path, config: Configuration) -> tuple:
    """(queries, subjects, identity, cov_query, is_null) of a ``wire.save_tile`` file made under ``config``."""
    tile_config, *tile = wire.load_tile(tile_file)
    for key in wire.CONFIG_FIELDS:
        if tile_config[key] != getattr(config, key):
            sourmash_hip.log_sys_exit(logger, f"Tile file {tile_file} configuration does not match the run ({key})")
    return tuple(tile)


def import_tile(logger: logging.Logger, conn, run: Run, tile_file: Path) -> int:
    """Import one binary column file written by ``wire.save_tile`` (resuming a direct-ingest run)."""
    return ingest_matrices(conn, run, *_load_tile(logger, tile_file, run.configuration))


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
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")
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


# ------------------------------------------------------------------ export-run (pyani_plus/public_cli.py:974-1091)
def export_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem",
               logger: logging.Logger | None = None) -> list[Path]:
    """Write ``<method>_run_<id>.tsv`` (long form) and the six matrices ``<method>_{identity,aln_lengths,sim_errors,
    query_cov,hadamard,tANI}.tsv`` of a run, byte for byte what the reference's ``export-run`` writes from the same
    database: long form in ``Run.comparisons()`` order with ``NA`` for NULL and Python ``str(float)``; matrices from
    the cached ``df_*`` strings through pandas ``to_csv(sep="\t")``, labelled by ``md5``, ``filename`` or ``stem`` and
    sorted by label (db_orm.py:590-624).  A partial run gets the long form only and then the reference's error."""
    import pandas as pd

    logger = logger or logging.getLogger("pyani_plus_amd")
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    conn, run = _open_run(logger, database, run_id, "Exporting")
    run_id = run.run_id
    if not run.fasta_hashes:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run_id} has no genomes")
    method = run.configuration.method
    if label == "md5":
        mapping = {a.genome_hash: a.genome_hash for a in run.fasta_hashes}
    elif label == "filename":
        mapping = {a.genome_hash: a.fasta_filename for a in run.fasta_hashes}
    elif label == "stem":
        mapping = {a.genome_hash: filename_stem(a.fasta_filename) for a in run.fasta_hashes}
    else:
        sourmash_hip.log_sys_exit(logger, f"Unexpected label scheme {label!r}")

    def float_or_na(value) -> str:
        return "NA" if value is None else str(value)

    written = [outdir / f"{method}_run_{run_id}.tsv"]
    rows = _select_run_comparisons(
        conn, run, "c.query_hash, c.subject_hash, c.identity, c.cov_query, c.cov_subject, c.aln_length, c.sim_errors", "ORDER BY c.comparison_id"
    ).fetchall()
    with written[0].open("w") as handle:
        handle.write("#Query\tSubject\tIdentity\tQuery-Cov\tSubject-Cov\tHadamard\ttANI\tAlign-Len\tSim-Errors\n")
        for q, s_hash, identity, cov_query, cov_subject, aln_length, sim_errors in rows:
            hadamard = None if identity is None or cov_query is None else identity * cov_query
            tani = None if hadamard is None else -math.log(hadamard)
            handle.write(
                f"{mapping[q]}\t{mapping[s_hash]}\t{float_or_na(identity)}\t{float_or_na(cov_query)}\t{float_or_na(cov_subject)}"
                f"\t{float_or_na(hadamard)}\t{float_or_na(tani)}\t{float_or_na(aln_length)}\t{float_or_na(sim_errors)}\n"
            )
    logger.info("Wrote long-form to %s", written[0])
    n = len(run.fasta_hashes)
    if len(rows) != n * n:  # db_orm.load_run(check_complete=True)
        sourmash_hip.log_sys_exit(logger, f"run-id {run_id} has {len(rows)} of {n}^2={n * n} comparisons, {n * n - len(rows)} needed")
    cached = conn.execute(
        "SELECT df_identity, df_aln_length, df_sim_errors, df_cov_query, df_hadamard FROM runs WHERE run_id=?", (run_id,)
    ).fetchone()
    if any(c is None for c in cached):
        out = cache_comparisons(conn, run)
        cached = tuple(out.get(k) for k in ("df_identity", "df_aln_length", "df_sim_errors", "df_cov_query", "df_hadamard"))
        if any(c is None for c in cached):
            sourmash_hip.log_sys_exit(logger, f"Could not load run {method} matrix")
    frames = [pd.read_json(StringIO(c), orient="split", dtype=float) for c in cached]
    with np.errstate(divide="ignore", invalid="ignore"):
        frames.append(-np.log(frames[4]))  # tANI = -ln(hadamard), not cached (db_orm.py:566-588)
    if label == "stem" and len(set(mapping.values())) < len(mapping):
        sourmash_hip.log_sys_exit(logger, "Duplicate filename stems, consider using MD5 labelling.")
    for frame, kind in zip(frames, ("identity", "aln_lengths", "sim_errors", "query_cov", "hadamard", "tANI")):
        if label != "md5":
            frame = frame.rename(index=mapping, columns=mapping).sort_index(axis=0).sort_index(axis=1)  # noqa: PLW2901
        written.append(outdir / f"{method}_{kind}.tsv")
        frame.to_csv(written[-1], sep="\t")
    logger.info("Wrote matrices to %s/%s_*.tsv", outdir, method)
    conn.close()
    return written


# ------------------------------------------------------------------ what classify and plot-run read of a complete run
def _score_frames(logger, conn, run: Run) -> list:
    """The identity, query coverage and Hadamard matrices of a complete run as frames over sorted md5: the cached
    ``runs.df_*`` strings the reference reads (10 decimals), filled with ``cache_comparisons`` first when they are missing;
    for a run too large for the cache, the comparisons table, unrounded."""
    import pandas as pd

    kinds = ("identity", "cov_query", "hadamard")
    if _matrix_cache_too_big(len(run.fasta_hashes)):
        hashes, mats = _comparison_matrices(conn, run)
        mats["hadamard"] = mats["identity"] * mats["cov_query"]
        return [pd.DataFrame(mats[k], index=hashes, columns=hashes) for k in kinds]
    cached = conn.execute("SELECT df_identity, df_cov_query, df_hadamard FROM runs WHERE run_id=?", (run.run_id,)).fetchone()
    if any(c is None for c in cached):
        out = cache_comparisons(conn, run)
        cached = tuple(out.get(f"df_{k}") for k in kinds)
        if any(c is None for c in cached):
            sourmash_hip.log_sys_exit(logger, f"Could not load run {run.configuration.method} matrix")
    return [pd.read_json(StringIO(c), orient="split", dtype=float) for c in cached]


def _relabelled(logger, run: Run, frames: list, label: str) -> list:
    """``Run.relabelled_matrix`` (db_orm.py:590-624) of every frame: labelled by ``md5`` (as they are), ``filename`` or
    ``stem`` and sorted by label on both axes, with the reference's messages for duplicate stems and an unknown label."""
    if label == "md5":
        return frames
    if label == "filename":
        mapping = {a.genome_hash: a.fasta_filename for a in run.fasta_hashes}
    elif label == "stem":
        mapping = {a.genome_hash: filename_stem(a.fasta_filename) for a in run.fasta_hashes}
        if len(set(mapping.values())) < len(mapping):
            sourmash_hip.log_sys_exit(logger, "Duplicate filename stems, consider using MD5 labelling.")
    else:
        sourmash_hip.log_sys_exit(logger, f"Unexpected label scheme {label!r}")
    return [f.rename(index=mapping, columns=mapping).sort_index(axis=0).sort_index(axis=1) for f in frames]


# ------------------------------------------------------------------ classify (pyani_plus/public_cli.py:1211-1331)
def classify(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", coverage_edges: str = "min",  # noqa: PLR0913
             score_edges: str = "mean", cov_min: float = classify_mod.MIN_COVERAGE, mode: str = "identity", engine=None,
             logger: logging.Logger | None = None) -> Path:
    """Write ``<method>_classify.tsv``, the table of genome cliques of a complete run (``n_nodes, max_cov,
    min_<score>, max_<score>, members``; the score is ``identity`` or ``-tANI``), with the reference's header and number
    formatting and its messages for a missing database, an incomplete run, duplicate stems and an unknown label.

    The matrices are the ones the reference reads: the cached ``runs.df_*`` JSON strings (10 decimals), filled with
    ``cache_comparisons`` first when they are missing, relabelled and sorted by label.  Which rows there are is the
    reference's answer whenever no two edges have the same score; with ties, and for the order of rows and members,
    ``pyani_plus_amd.classify`` says what this project defines.  A run too large for the cache (about 8 500 genomes
    and more) cannot be classified by the reference at all; its matrices are then taken from the comparisons table,
    unrounded, which is beyond what the reference defines.

    ``engine``: a ``HipEngine`` builds and sorts the edge list on the GPU; None does it on the host.  The plot of the
    reference (``plot_classify``) is not made."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")
    for name, role in ((coverage_edges, "coverage"), (score_edges, "score")):
        if name not in classify_mod.AGG_NAMES:
            sourmash_hip.log_sys_exit(logger, f"Unknown {role} aggregator {name!r}: expected one of {', '.join(classify_mod.AGG_NAMES)}")
    if mode not in classify_mod.MODES:
        sourmash_hip.log_sys_exit(logger, f"Unknown classify mode {mode!r}: expected one of {', '.join(classify_mod.MODES)}")
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    conn, run = _open_run(logger, database, run_id, "Exporting")
    run_id = run.run_id
    n = len(run.fasta_hashes)
    done = count_run_comparisons(conn, run)
    if not n:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run_id} has no genomes")
    if done != n * n:  # db_orm.load_run(check_complete=True)
        sourmash_hip.log_sys_exit(logger, f"run-id {run_id} has {done} of {n}^2={n * n} comparisons, {n * n - done} needed")
    method = run.configuration.method
    frames = _score_frames(logger, conn, run)
    conn.close()
    if done == 1 and n == 1:
        logger.warning("Run %d has %d comparison across %d genome. Reporting single clique.", run_id, done, n)
    else:
        logger.info("Run %d has %d comparisons across %d genomes.", run_id, done, n)
    identity, cov, hadamard = _relabelled(logger, run, frames, label)
    score = identity.to_numpy(dtype=float) if mode == "identity" else classify_mod.tani_scores(hadamard.to_numpy(dtype=float))
    rows = classify_mod.classify_matrices([str(x) for x in cov.columns], score, cov.to_numpy(dtype=float), coverage_edges=coverage_edges,
                                          score_edges=score_edges, cov_min=cov_min, engine=engine)
    written = outdir / f"{method}_classify.tsv"
    written.write_text(classify_mod.classify_tsv(rows, mode))
    logger.info("Wrote classify output to %s", outdir)
    return written


# ------------------------------------------------------------------ a run's distances (tree-run, ordinate-run)
def _require_database(logger, database) -> None:
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")


def _distance_run(logger, database, outdir, run_id: int | None, label: str, missing: float, what: str):  # noqa: PLR0913
    """What tree-run and ordinate-run start from: ``(outdir, method, identity, distances)`` of a complete run -- the
    output directory made, the run opened and checked, its identity frame relabelled and sorted by label as ``classify``
    and ``plot-run`` read it, and ``tree.run_distances`` of it -- with the reference's messages for an incomplete run,
    duplicate stems and an unknown label.  ``what`` is the thing an identity above 1 leaves undefined."""
    if not (math.isfinite(missing) and missing >= 0):
        sourmash_hip.log_sys_exit(logger, f"The distance of a pair without identity must be finite and not negative, not {missing!r}")
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    conn, run = _open_run(logger, database, run_id, "Exporting")
    run_id = run.run_id
    n = len(run.fasta_hashes)
    done = count_run_comparisons(conn, run)
    if not n:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run_id} has no genomes")
    if done != n * n:  # db_orm.load_run(check_complete=True)
        sourmash_hip.log_sys_exit(logger, f"run-id {run_id} has {done} of {n}^2={n * n} comparisons, {n * n - done} needed")
    run_method = run.configuration.method
    frames = _score_frames(logger, conn, run)
    conn.close()
    logger.info("Run %d has %d comparisons across %d genomes.", run_id, done, n)
    identity = _relabelled(logger, run, frames, label)[0]
    distances = tree_mod.run_distances(identity, missing, logger)
    if (distances < 0).any():
        sourmash_hip.log_sys_exit(logger, f"An identity above 1 gives a negative distance: no {what} is defined")
    return outdir, run_method, identity, distances


# ------------------------------------------------------------------ tree-run (this project's own: the reference writes no tree)
def tree_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", method: str = "nj", missing: float = 1.0,  # noqa: PLR0913
             engine=None, logger: logging.Logger | None = None) -> Path:
    """Write ``<method>_identity_<nj|upgma>.nwk``: the tree of a complete run's genomes as one line of Newick text, from
    the distances ``1 - identity`` (``tree.run_distances``: the two directions averaged; ``missing`` where a pair has no
    identity either way).  ``method`` "nj" is canonical neighbour joining (unrooted, written with a
    trifurcation at the last join), "upgma" the average-linkage tree of the same distances.  The matrices and labels are
    the ones ``classify`` and ``plot-run`` read, with the reference's messages for a missing database, an incomplete run,
    duplicate stems and an unknown label.

    ``engine``: a ``HipEngine`` makes the joins of "nj" on the GPU; None makes them on the host, with the same bits.
    UPGMA runs on the host either way."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    if method not in tree_mod.METHODS:
        sourmash_hip.log_sys_exit(logger, f"Unknown tree method {method!r}: expected one of {', '.join(tree_mod.METHODS)}")
    outdir, run_method, identity, distances = _distance_run(logger, database, outdir, run_id, label, missing, "tree")
    table = tree_mod.neighbour_joining(distances, engine=engine) if method == "nj" else tree_mod.upgma(distances)
    written = outdir / f"{run_method}_identity_{method}.nwk"
    written.write_text(tree_mod.newick(table, [str(x) for x in identity.columns]) + "\n")
    logger.info("Wrote %s tree to %s", method, written)
    return written


# ------------------------------------------------------------------ ordinate-run (this project's own: the reference writes no ordination)
def ordinate_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", dimensions: int = 3,  # noqa: PLR0913
                 missing: float = 1.0, formats: tuple[str, ...] = ("tsv",), engine=None, logger: logging.Logger | None = None) -> list[Path]:
    """Write the principal coordinates of a complete run's genomes (``ordination.pcoa``) from the
    distances ``1 - identity`` that ``tree-run`` uses (``tree.run_distances``; ``missing`` where a pair has no identity
    either way), opened and checked exactly as ``tree_run`` does, with the same messages:

    * ``<method>_identity_pcoa.tsv``: ``genome, PC1 .. PCk``, one row per genome in the label-sorted order of the
      matrices, values as ``repr(float)``;
    * ``<method>_identity_pcoa_eigenvalues.tsv``: ``component, eigenvalue, proportion_of_trace, cumulative, residual``
      (the trace includes the negative eigenvalues: see ``ordination.Ordination``);
    * with an image format (``png``, ``pdf``, ``svg``, ``jpg``), ``<method>_identity_pcoa.<ext>``: PC1 against PC2.

    ``engine``: a ``HipEngine`` centres the matrix and does the solver's products on the GPU; None does both on the
    host, with the same bytes.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    formats = tuple(formats)
    images = [ext for ext in formats if ext != "tsv"]
    if images:
        try:
            importlib.import_module("matplotlib")
        except ImportError:
            sourmash_hip.log_sys_exit(logger, f"Image formats ({', '.join(images)}) need matplotlib, which cannot be imported; only tsv is available")
    if int(dimensions) < 1 or int(dimensions) > _capi.PA_EIGS_MAX_K:
        sourmash_hip.log_sys_exit(logger, f"Expected 1 to {_capi.PA_EIGS_MAX_K} dimensions, not {dimensions!r}")
    outdir, method, identity, distances = _distance_run(logger, database, outdir, run_id, label, missing, "ordination")
    n = len(distances)
    if int(dimensions) > n:
        sourmash_hip.log_sys_exit(logger, f"{int(dimensions)} dimensions for {n} genomes: at most as many axes as genomes")
    result = ordination_mod.pcoa(distances, int(dimensions), engine=engine)
    labels = [str(x) for x in identity.columns]
    stem = f"{method}_identity_pcoa"
    written = []
    if "tsv" in formats:
        written += [outdir / f"{stem}.tsv", outdir / f"{stem}_eigenvalues.tsv"]
        written[-2].write_text(ordination_mod.coordinates_tsv(result, labels))
        written[-1].write_text(ordination_mod.eigenvalues_tsv(result))
    for ext in images:
        written.append(outdir / f"{stem}.{ext}")
        ordination_figure.draw_ordination(result, labels, f"{method} identity", written[-1])
    logger.info("Wrote %d axes of %d genomes (%d iterations, shift %r) to %s", int(dimensions), n, result.info[1], result.info[2], outdir)
    return written


# ------------------------------------------------------------------ plot-run (pyani_plus/public_cli.py:1095-1136)
# score, colour map, what a NaN cell counts as when the rows are clustered (pyani_plus/plot_run.py:320-325)
_PLOT_SCORES = (("identity", "spbnd_BuRd", 0), ("query_cov", "BuRd", 0), ("hadamard", "viridis", 0), ("tANI", "viridis_r", -5))


def _write_scatter_tables(logger, conn, run: Run, outdir: Path) -> list[Path]:
    """``<method>_{query_cov,tANI}_scatter.tsv`` (pyani_plus/plot_run.py:231-293): identity, the y value and the query's
    length of every comparison that has both, unrounded, in ``comparison_id`` order, numbers as Python's ``str``."""
    method = run.configuration.method
    lengths = dict(conn.execute("SELECT genome_hash, length FROM genomes"))
    rows = [
        (identity, cov_query, lengths[query])
        for query, identity, cov_query in _select_run_comparisons(conn, run, "c.query_hash, c.identity, c.cov_query", "ORDER BY c.comparison_id")
    ]
    written = []
    for caption, name in (("Query coverage", "query_cov"), ("tANI", "tANI")):
        values = [(x, y, c) for x, y, c in rows if x is not None and y is not None]
        if not values:
            logger.warning("No valid identity, %s values from %s run", caption, method)
            return written
        logger.info("Plotting %d/%d %s vs identity %s comparisons", len(values), len(rows), caption, method)
        if name == "tANI":
            zeros = sum(1 for x, y, _c in values if x * y == 0)
            if zeros:
                # -log(0): the reference raises here and plots nothing more; this row is written with inf instead
                logger.warning("%d %s comparisons have a zero Hadamard product: their tANI is written as inf", zeros, method)
            values = [(x, -math.log(x * y) if x * y else math.inf, c) for x, y, c in values]
        written.append(outdir / f"{method}_{name}_scatter.tsv")
        with written[-1].open("w") as handle:
            handle.write(f"#identity\t{name}\tquery_length\n")
            for x, y, c in values:
                handle.write(f"{x}\t{y}\t{c}\n")
    return written


def _run_label(genome, label: str) -> str:
    """The label ``_relabelled`` gives a genome of the run."""
    return {"md5": genome.genome_hash, "filename": genome.fasta_filename}.get(label) or filename_stem(genome.fasta_filename)


def _write_scatter_figures(logger, method: str, frames: dict, lengths: np.ndarray, outdir: Path, formats: tuple[str, ...], bins: int,  # noqa: PLR0913
                           engine, warned: int | None) -> list[Path]:
    """The scatter figures of ``plot_run(scatter=True)`` and their tables (``pyani_plus_amd.scatter``), from the
    relabelled identity, query coverage and Hadamard frames; ``lengths``: the query length of each row.  ``warned``: the
    position of the score the scatter tables have already logged the no-valid-values warning for, or None."""
    n = len(lengths)
    cells = {name: np.ascontiguousarray(frames[name].to_numpy(dtype=float)) for name in ("identity", "query_cov")}
    cells["tANI"] = -classify_mod.tani_scores(frames["hadamard"].to_numpy(dtype=float))  # -log(h) if h else nan
    written: list[Path] = []
    try:
        if engine is not None:
            cells = {name: engine.torch.from_numpy(np.ascontiguousarray(v)).to(engine.device) for name, v in cells.items()}  # uploaded once
        for position, (caption, name) in enumerate((("Query coverage", "query_cov"), ("tANI", "tANI"))):
            data = scatter_mod.describe(cells["identity"], cells[name], lengths, n, engine, bins, logger)
            if data is None:
                if warned != position:
                    logger.warning("No valid identity, %s values from %s run", caption, method)
                return written
            if "tsv" in formats:
                written.append(outdir / f"{method}_{name}_scatter_grid.tsv")
                scatter_mod.write_grid_tsv(written[-1], data)
                for axis, hist in (("x", data.x_hist), ("y", data.y_hist)):
                    written.append(outdir / f"{method}_{name}_scatter_{axis}_hist.tsv")
                    distribution_mod.write_hist_tsv(written[-1], hist)
            for ext in formats:
                if ext != "tsv":
                    written.append(outdir / f"{method}_{name}_scatter.{ext}")
                    scatter_figure.draw_scatter(data, caption, written[-1])
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "plot-run scatter figures", err)
    return written


def plot_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", formats: tuple[str, ...] = ("tsv",),  # noqa: PLR0913
             engine=None, logger: logging.Logger | None = None, distributions: bool = False, scatter: bool = False,
             scatter_bins: int = scatter_mod.GRID) -> list[Path]:
    """Write what the reference's ``plot-run`` computes for a complete run: the clustered heatmap tables
    ``<method>_{identity,query_cov,hadamard,tANI}_heatmap.tsv`` and the scatter tables
    ``<method>_{query_cov,tANI}_scatter.tsv``, byte for byte what the reference writes from the same database, with its
    messages for a missing database, an incomplete run, duplicate stems, an unknown label, an all-NaN matrix and a
    matrix with some NaNs.

    Each matrix (the cached ``runs.df_*`` strings; tANI is ``-log(h) if h else nan`` of the relabelled Hadamard matrix)
    is relabelled, sorted by label, and put into the leaf order of the average-linkage clustering of its rows with NaN
    cells counted as 0 (tANI: -5): what seaborn's ``clustermap`` computes for the reference, restated by
    ``pyani_plus_amd.cluster`` with the same bits.  Every matrix is clustered on its own.

    ``formats``: ``tsv`` writes the tables; any other format (``png``, ``pdf``, ``svg``, ``jpg``) adds the heatmap figure
    with its row dendrogram, drawn with matplotlib alone.  The reference's scatter figures are made with ``scatter``.
    A comparison with a zero Hadamard product is written to the tANI scatter table as ``inf``, where the reference raises.

    ``distributions``: also the score distribution of each matrix that is plotted (``pyani_plus_amd.distribution``):
    with ``tsv`` the tables ``<method>_<score>_dist_hist.tsv`` (``#left TAB right TAB count``, the bins of
    ``numpy.histogram(cells, "auto")``) and ``<method>_<score>_dist_kde.tsv`` (``#x TAB density``, scipy's
    ``gaussian_kde`` on seaborn's 200-point grid; the header alone for fewer than two cells or cells that are all
    equal), floats as ``repr``; with an image format the reference's ``<method>_<score>_dist.<ext>``, histogram, density
    and rug.  The reference writes no table for a distribution: the two are this project's.  Off by default.

    ``scatter``: also the reference's two scatter figures, identity against query coverage and against tANI
    (``pyani_plus_amd.scatter``), after everything else and in that order.  The reference draws a marker per comparison,
    coloured by the query's length, with automatic histograms on the margins; here the joint panel is a raster of
    ``scatter_bins`` x ``scatter_bins`` cells (1 to 1024, 256 by default) over the ranges of the valid points, a cell in
    the colour of the last point that falls into it, which is what overdrawn markers show.  The points are the cells of
    the matrices above in row-major order (rows = query); a point is valid iff neither value is NaN, so a zero Hadamard
    product (tANI NaN) drops out.  Two things are this project's choices: "last" is by that row-major order of the
    label-sorted matrix, where the reference's is ``comparison_id`` order, and for runs that fit the cache the values are
    the cached 10-decimal ones, as for the distributions.  With ``tsv``: ``<method>_<y>_scatter_grid.tsv``
    (``#x_left x_right y_left y_right count query_length``, a line per non-empty cell, x-major) and the margins
    ``<method>_<y>_scatter_x_hist.tsv`` and ``<method>_<y>_scatter_y_hist.tsv`` (as ``_dist_hist.tsv``); with an image
    format the reference's ``<method>_<y>_scatter.<ext>``.  Without a valid point the reference's warning is logged and
    neither this figure nor the next is made.  Off by default.

    ``engine``: a ``HipEngine`` computes the row distances, the distributions and the scatter rasters on the GPU; None on
    the host.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")
    formats = tuple(formats)
    images = [ext for ext in formats if ext != "tsv"]
    if images:
        try:
            importlib.import_module("matplotlib")
        except ImportError:
            sourmash_hip.log_sys_exit(logger, f"Image formats ({', '.join(images)}) need matplotlib, which cannot be imported; only tsv is available")
    if scatter and not 1 <= int(scatter_bins) <= scatter_mod.MAX_BINS:
        sourmash_hip.log_sys_exit(logger, f"--scatter-bins {scatter_bins}: expected 1 to {scatter_mod.MAX_BINS}")
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    conn, run = _open_run(logger, database, run_id, "Plotting")
    run_id = run.run_id
    n = len(run.fasta_hashes)
    done = count_run_comparisons(conn, run)
    if not n:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run_id} has no genomes")
    if done != n * n:  # db_orm.load_run(check_complete=True)
        sourmash_hip.log_sys_exit(logger, f"run-id {run_id} has {done} of {n}^2={n * n} comparisons, {n * n - done} needed")
    method = run.configuration.method
    frames = dict(zip(("identity", "query_cov", "hadamard"), _relabelled(logger, run, _score_frames(logger, conn, run), label)))
    written = _write_scatter_tables(logger, conn, run, outdir) if "tsv" in formats else []
    scatter_tables = len(written)
    genome_lengths = dict(conn.execute("SELECT genome_hash, length FROM genomes")) if scatter else {}
    conn.close()
    for name, color_scheme, na_fill in _PLOT_SCORES:
        if name == "tANI":
            hadamard = frames["hadamard"]
            matrix = hadamard.copy()
            matrix.iloc[:, :] = -classify_mod.tani_scores(hadamard.to_numpy(dtype=float))  # -log(h) if h else nan; -log(1.0) is -0.0
        else:
            matrix = frames[name]
        nulls = int(matrix.isna().to_numpy().sum())
        if nulls == n * n:
            logger.warning("Cannot plot %s as all NA", name)
            continue
        if nulls:
            logger.warning("%s matrix contains %d nulls (out of %d\u00b2=%d %s comparisons)", name, nulls, n, n * n, method)
        try:
            tree, leaves = cluster_mod.cluster_tree(matrix.to_numpy(dtype=float), na_fill, engine)
        except HipBackendError as err:
            sourmash_hip.backend_failure(logger, f"plot-run clustering of {name}", err)
        table = matrix.iloc[leaves, leaves]
        for ext in formats:
            written.append(outdir / f"{method}_{name}_heatmap.{ext}")
            if ext == "tsv":
                table.to_csv(written[-1], sep="\t")
            else:
                heatmap_figure.draw_heatmap(table, tree, leaves, name, color_scheme, written[-1])
        if distributions:
            try:
                cells = np.ascontiguousarray(matrix.to_numpy(dtype=float))
                values = engine.torch.from_numpy(cells).to(engine.device) if engine is not None else cells  # uploaded once
                dist = distribution_mod.describe(values, engine, logger)
                rug = distribution_mod.rug_counts(values, name, dist, engine) if images else None
            except HipBackendError as err:
                sourmash_hip.backend_failure(logger, f"plot-run distribution of {name}", err)
            if "tsv" in formats:
                written.append(outdir / f"{method}_{name}_dist_hist.tsv")
                distribution_mod.write_hist_tsv(written[-1], dist)
                written.append(outdir / f"{method}_{name}_dist_kde.tsv")
                distribution_mod.write_kde_tsv(written[-1], dist)
            for ext in images:
                written.append(outdir / f"{method}_{name}_dist.{ext}")
                distribution_figure.draw_distribution(dist, rug, name, written[-1])
    if scatter:
        by_label = {_run_label(a, label): genome_lengths[a.genome_hash] for a in run.fasta_hashes}
        lengths = np.array([by_label[q] for q in frames["identity"].index], dtype=np.int64)
        # the scatter tables have logged the warning for the first score they found no comparison for
        warned = scatter_tables if "tsv" in formats else None
        written += _write_scatter_figures(logger, method, frames, lengths, outdir, formats, int(scatter_bins), engine, warned)
    logger.info("Wrote %d images to %s/%s_*.*", len(written), outdir, method)
    return written


# ------------------------------------------------------------------ plot-run-comp (pyani_plus/public_cli.py:1140-1208)
_RUN_COMP_CHUNK = 1 << 16  # comparisons fetched from SQLite at a time


def _run_comparison_columns(conn, run: Run) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(q, s, identity)`` of the run's comparisons in ``comparison_id`` order: uint32 positions of the query and the
    subject in the TEMP table ``run_comp_ref`` (``run_comp.NONE`` for a genome that is not in it) and float64 identities
    (NaN for NULL).  The hashes are turned into positions by SQLite and the rows become arrays a chunk at a time: no
    Python dictionary is consulted per row and no list of all the rows is built."""
    cursor = _select_run_comparisons(
        conn, run,
        "COALESCE((SELECT h.idx FROM temp.run_comp_ref h WHERE h.genome_hash = c.query_hash), -1), "
        "COALESCE((SELECT h.idx FROM temp.run_comp_ref h WHERE h.genome_hash = c.subject_hash), -1), c.identity",
        "ORDER BY c.comparison_id",
    )  # fmt: skip
    parts: list[tuple[np.ndarray, np.ndarray, np.ndarray]] = []
    while rows := cursor.fetchmany(_RUN_COMP_CHUNK):
        q, s, y = zip(*rows)
        parts.append((np.array(q, dtype=np.int64).astype(np.uint32), np.array(s, dtype=np.int64).astype(np.uint32), np.array(y, dtype=np.float64)))
    if not parts:
        return np.empty(0, dtype=np.uint32), np.empty(0, dtype=np.uint32), np.empty(0, dtype=np.float64)
    return tuple(np.concatenate(column) for column in zip(*parts))


def plot_run_comp(database: Path | str, outdir: Path, run_ids, *, columns: int = 0, formats: tuple[str, ...] = ("tsv",),  # noqa: PLR0913
                  engine=None, logger: logging.Logger | None = None) -> list[Path]:
    """Compare the identities of runs of one database pair by pair, as the reference's ``plot-run-comp`` does: the first
    of ``run_ids`` (a comma separated string, or integers) is the reference run, and for each further run the table
    ``<method>_identity_<ref>_vs_<other>.tsv`` holds a line ``x TAB y`` for every ordered genome pair both runs have an
    identity for (x the reference run's, y the other's, unrounded, under the header ``#<ref name> TAB <other name>``),
    with the reference's messages.  The rows are in the order of the other run's ``comparison_id``, where the reference
    leaves the order to the SQLite planner.  The runs need not be complete.

    ``formats``: ``tsv`` writes the tables; any other format (``png``, ``pdf``, ``svg``, ``jpg``) adds
    ``<method>_identity_<ref>_{scatter,diff}_vs_others.<ext>`` on the reference's grid (``columns`` panels a row, 0 for a
    square tiling), drawn with matplotlib alone from the computed 30-bin histograms (``pyani_plus_amd.run_comp``).

    ``engine``: a ``HipEngine`` joins the runs and takes the histograms on the GPU; None on the host, with the same
    bytes.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")
    formats = tuple(formats)
    images = [ext for ext in formats if ext != "tsv"]
    if images:
        try:
            importlib.import_module("matplotlib")
        except ImportError:
            sourmash_hip.log_sys_exit(logger, f"Image formats ({', '.join(images)}) need matplotlib, which cannot be imported; only tsv is available")
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    try:
        runs = [int(x) for x in (run_ids.split(",") if isinstance(run_ids, str) else run_ids)]
    except (TypeError, ValueError):
        sourmash_hip.log_sys_exit(logger, f"Expected comma separated list of runs, not: {run_ids}")
    if len(runs) < 2:  # noqa: PLR2004
        sourmash_hip.log_sys_exit(logger, "Need at least two runs for a comparison")
    ref_id, other_ids = runs[0], runs[1:]
    conn, ref_run = _open_run(logger, database, ref_id, "Plotting")
    if not count_run_comparisons(conn, ref_run):
        sourmash_hip.log_sys_exit(logger, f"Run {ref_id} has no comparisons")
    method = ref_run.configuration.method
    hashes = sorted(a.genome_hash for a in ref_run.fasta_hashes)
    conn.execute("DROP TABLE IF EXISTS temp.run_comp_ref")
    conn.execute("CREATE TEMP TABLE run_comp_ref (genome_hash VARCHAR NOT NULL PRIMARY KEY, idx INTEGER NOT NULL)")
    conn.executemany("INSERT INTO temp.run_comp_ref VALUES (?, ?)", zip(hashes, range(len(hashes))))
    q, s, y = _run_comparison_columns(conn, ref_run)
    ref = np.full((len(hashes), len(hashes)), np.nan)
    ref[q, s] = y  # (query, subject) is unique under one configuration
    del q, s, y
    logger.info("Plotting %d runs against %s run %d which has %d comparisons", len(other_ids), method, ref_id, int(np.count_nonzero(~np.isnan(ref))))
    written: list[Path] = []
    comparisons, other_names = [], []
    try:
        ref_values = engine.torch.from_numpy(ref).to(engine.device) if engine is not None else ref  # uploaded once
        x_hist = run_comp_mod.range_and_counts(ref_values, engine)
        for other_id in other_ids:
            try:
                other = load_run(conn, other_id)
            except ValueError:
                sourmash_hip.log_sys_exit(logger, f"Database {database} has no run-id {other_id}.")
            comp = run_comp_mod.compare(ref_values, *_run_comparison_columns(conn, other), engine, x_hist=x_hist)
            if not len(comp.x):
                sourmash_hip.log_sys_exit(logger, f"Runs {ref_id} and {other_id} have no comparisons in common")
            logger.info("Plotting %s run %d vs %s run %d, with %d comparisons in common", other.configuration.method, other_id, method, ref_id, len(comp.x))
            if "tsv" in formats:
                written.append(outdir / f"{method}_identity_{ref_id}_vs_{other_id}.tsv")
                run_comp_mod.write_pairs_tsv(written[-1], f"#{ref_run.name}\t{other.name}", comp.x, comp.y)
            if images:  # the figures need every run's values at once; the tables do not
                comparisons.append(comp)
                other_names.append(other.name)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "plot-run-comp", err)
    finally:
        conn.close()
    for mode in ("scatter", "diff"):
        for ext in images:
            written.append(outdir / f"{method}_identity_{ref_id}_{mode}_vs_others.{ext}")
            run_comp_figure.draw_comparison(mode, ref_run.name, other_names, comparisons, written[-1], columns)
    logger.info("Wrote %d images to %s/%s_identity_%d_vs_*.*", 2 * len(images), outdir, method, ref_id)
    return written


# ------------------------------------------------------------------ the driver as a process
def main(argv: list[str] | None = None) -> int:
    """``python -m pyani_plus_amd.rundb {sourmash,fastani,external-alignment,tetra,resume,export-run,classify,plot-run,plot-run-comp,tree-run,ordinate-run} ...``: the run driver as a process of its own,
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
    p_x.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_t = sub.add_parser("tetra", help="FASTA directory -> all N^2 TETRA-hip comparisons (tetranucleotide Z-score correlations)")
    common(p_t, run_options=True)
    p_t.add_argument("--cache", type=Path, default=None)
    p_t.add_argument("--device", type=int, default=None, help="count and correlate on this GPU (default: on the host)")
    p_r = sub.add_parser("resume", help="complete a partial run")
    common(p_r, run_options=False)
    p_r.add_argument("--run-id", type=int, default=None)
    p_r.add_argument("--cache", type=Path, default=None)
    p_e = sub.add_parser("export-run", help="long form and matrices of a run as TSV files")
    p_e.add_argument("--database", "-d", required=True, type=Path)
    p_e.add_argument("--outdir", "-o", required=True, type=Path)
    p_e.add_argument("--run-id", type=int, default=None)
    p_e.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_e.add_argument("--verbose", "-v", action="store_true")
    p_c = sub.add_parser("classify", help="the genome cliques of a complete run as <method>_classify.tsv")
    p_c.add_argument("--database", "-d", required=True, type=Path)
    p_c.add_argument("--outdir", "-o", required=True, type=Path)
    p_c.add_argument("--run-id", type=int, default=None)
    p_c.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_c.add_argument("--coverage-edges", choices=classify_mod.AGG_NAMES, default="min")
    p_c.add_argument("--score-edges", choices=classify_mod.AGG_NAMES, default="mean")
    p_c.add_argument("--cov-min", type=float, default=classify_mod.MIN_COVERAGE)
    p_c.add_argument("--mode", choices=classify_mod.MODES, default="identity")
    p_c.add_argument("--device", type=int, default=None, help="build and sort the edge list on this GPU (default: on the host)")
    p_c.add_argument("--verbose", "-v", action="store_true")
    p_p = sub.add_parser("plot-run", help="the clustered heatmap tables and the scatter tables of a complete run")
    p_p.add_argument("--database", "-d", required=True, type=Path)
    p_p.add_argument("--outdir", "-o", required=True, type=Path)
    p_p.add_argument("--run-id", type=int, default=None)
    p_p.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_p.add_argument("--formats", default="tsv", help="comma separated: tsv for the tables, png, pdf, svg or jpg for the heatmap figures (matplotlib)")
    p_p.add_argument("--distributions", action="store_true", help="also each score's distribution: histogram and density tables, and the figure with an image format")
    p_p.add_argument("--scatter", action="store_true", help="also the two scatter figures (identity against query coverage and tANI) as rasters: their grid and margin tables, and the figure with an image format")
    p_p.add_argument("--scatter-bins", type=int, default=scatter_mod.GRID, help="cells per axis of a scatter figure's raster, 1 to 1024 (default 256)")
    p_p.add_argument("--device", type=int, default=None, help="compute the row distances, the distributions and the scatter rasters on this GPU (default: on the host)")
    p_p.add_argument("--verbose", "-v", action="store_true")
    p_pc = sub.add_parser("plot-run-comp", help="the identities of further runs against a reference run's, pair by pair")
    p_pc.add_argument("--database", "-d", required=True, type=Path)
    p_pc.add_argument("--outdir", "-o", required=True, type=Path)
    p_pc.add_argument("--run-ids", required=True, help="comma separated list of runs, the reference run first")
    p_pc.add_argument("--columns", type=int, default=0, help="panels per row of the figures (default 0: a square tiling)")
    p_pc.add_argument("--formats", default="tsv", help="comma separated: tsv for the tables, png, pdf, svg or jpg for the two figures (matplotlib)")
    p_pc.add_argument("--device", type=int, default=None, help="join the runs and take the histograms on this GPU (default: on the host)")
    p_pc.add_argument("--verbose", "-v", action="store_true")
    p_tr = sub.add_parser("tree-run", help="the neighbour-joining or UPGMA tree of a complete run as <method>_identity_<nj|upgma>.nwk")
    p_tr.add_argument("--database", "-d", required=True, type=Path)
    p_tr.add_argument("--outdir", "-o", required=True, type=Path)
    p_tr.add_argument("--run-id", type=int, default=None)
    p_tr.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_tr.add_argument("--method", choices=tree_mod.METHODS, default="nj")
    p_tr.add_argument("--missing", type=float, default=1.0, help="distance of a pair with no identity in either direction (default 1.0)")
    p_tr.add_argument("--device", type=int, default=None, help="make the joins of neighbour joining on this GPU (default: on the host)")
    p_tr.add_argument("--verbose", "-v", action="store_true")
    p_or = sub.add_parser("ordinate-run", help="the principal coordinates of a complete run as <method>_identity_pcoa.tsv and its eigenvalue table")
    p_or.add_argument("--database", "-d", required=True, type=Path)
    p_or.add_argument("--outdir", "-o", required=True, type=Path)
    p_or.add_argument("--run-id", type=int, default=None)
    p_or.add_argument("--label", choices=("md5", "filename", "stem"), default="stem")
    p_or.add_argument("--dimensions", type=int, default=3, help="principal axes to compute (default 3)")
    p_or.add_argument("--missing", type=float, default=1.0, help="distance of a pair with no identity in either direction (default 1.0)")
    p_or.add_argument("--formats", default="tsv", help="comma separated: tsv for the two tables, png, pdf, svg or jpg for the figure (matplotlib)")
    p_or.add_argument("--device", type=int, default=None, help="centre the matrix and do the solver's products on this GPU (default: on the host)")
    p_or.add_argument("--verbose", "-v", action="store_true")
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO, format="%(levelname)s %(message)s")
    logger = logging.getLogger("pyani_plus_amd")
    with launch.signals_as_interrupt():
        if args.command == "sourmash":
            run = run_sourmash_hip(args.fasta, args.database, cache=args.cache, name=args.name, kmersize=args.kmersize, scaled=args.scaled,
                                   temp=args.temp, logger=logger, ingest=args.ingest, gpus=args.gpus, engine_factory=args.engine_factory)
        elif args.command == "fastani":
            run = run_fastani_hip(args.fasta, args.database, name=args.name, kmersize=args.kmersize, fragsize=args.fragsize,
                                  minmatch=args.minmatch, temp=args.temp, logger=logger, ingest=args.ingest, gpus=args.gpus,
                                  engine_factory=args.engine_factory, query_batch=args.query_batch)
        elif args.command == "external-alignment":
            run = run_external_alignment_hip(args.fasta, args.database, alignment=args.alignment, label=args.label, name=args.name,
                                             temp=args.temp, logger=logger, gpus=args.gpus)
        elif args.command == "tetra":
            engine = None
            if args.device is not None:
                from .engine import HipEngine

                engine = HipEngine(args.device)
            try:
                run = run_tetra_hip(args.fasta, args.database, cache=args.cache, name=args.name, temp=args.temp, logger=logger, engine=engine,
                                    gpus=args.gpus)
            finally:
                if engine is not None:
                    engine.close()
        elif args.command == "resume":
            run = resume(args.database, run_id=args.run_id, cache=args.cache, temp=args.temp, logger=logger, ingest=args.ingest,
                         gpus=args.gpus, engine_factory=args.engine_factory)
        elif args.command in {"classify", "plot-run", "plot-run-comp", "tree-run", "ordinate-run"}:
            engine = None
            if args.device is not None:
                from .engine import HipEngine

                engine = HipEngine(args.device)
            try:
                if args.command == "classify":
                    print(classify(args.database, args.outdir, run_id=args.run_id, label=args.label, coverage_edges=args.coverage_edges,
                                   score_edges=args.score_edges, cov_min=args.cov_min, mode=args.mode, engine=engine, logger=logger))
                elif args.command == "tree-run":
                    print(tree_run(args.database, args.outdir, run_id=args.run_id, label=args.label, method=args.method, missing=args.missing,
                                   engine=engine, logger=logger))
                elif args.command == "ordinate-run":
                    formats = tuple(f for f in args.formats.split(",") if f)
                    for path in ordinate_run(args.database, args.outdir, run_id=args.run_id, label=args.label, dimensions=args.dimensions,
                                             missing=args.missing, formats=formats, engine=engine, logger=logger):
                        print(path)
                elif args.command == "plot-run-comp":
                    formats = tuple(f for f in args.formats.split(",") if f)
                    for path in plot_run_comp(args.database, args.outdir, args.run_ids, columns=args.columns, formats=formats, engine=engine, logger=logger):
                        print(path)
                else:
                    formats = tuple(f for f in args.formats.split(",") if f)
                    for path in plot_run(args.database, args.outdir, run_id=args.run_id, label=args.label, formats=formats, engine=engine, logger=logger,
                                         distributions=args.distributions, scatter=args.scatter, scatter_bins=args.scatter_bins):
                        print(path)
            finally:
                if engine is not None:
                    engine.close()
            return 0
        else:
            for path in export_run(args.database, args.outdir, run_id=args.run_id, label=args.label, logger=logger):
                print(path)
            return 0
    logger.info("run-id %d: %s", run.run_id, run.status)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
