"""The run database (stdlib ``sqlite3``): the build's own counterpart of the parts of ``db_orm`` that the run drivers
(``rundb``) and the run reports (``reports``) use (last row).  It imports neither of them.

* FASTA enumeration by the four extensions +- ``.gz`` (pyani_plus/utils.py:226-242)
* genome identity = md5 of the decompressed bytes (utils.py:142-196); length = sum of
  residues, description = first title (db_orm.py:832-866)
* the same tables / constraints as ``Base.metadata.create_all``
* JSON column import with INSERT OR IGNORE (private_cli.py:507-614, db_orm.py:1076)
* ``cache_comparisons``: N x N matrices over sorted md5, pandas ``to_json(orient="split")``
  (db_orm.py:393-466) -- built without the reference's O(N^3) ``hashes.index`` loop.

Databases written here can be opened by the reference and vice versa.
"""

from __future__ import annotations

import ctypes as C
import datetime
import logging
import platform
import sqlite3
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _capi, wire
from .methods import sourmash_hip

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


# ------------------------------------------------------------------ the matrix cache (``runs.df_*``)
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


def genome_lengths(conn, run: Run) -> dict[str, int]:
    """genome_hash -> ``genomes.length`` (bases) of the run's genomes."""
    wanted = {a.genome_hash for a in run.fasta_hashes}
    rows = conn.execute("SELECT g.genome_hash, g.length FROM genomes g JOIN runs_genomes rg ON rg.genome_hash = g.genome_hash WHERE rg.run_id=?",
                        (run.run_id,)).fetchall()  # fmt: skip
    return {h: int(length) for h, length in rows if h in wanted}
