"""The ``external-alignment-hip`` method: pyani-plus's external-alignment path on an MI355X.

Drop-in shaped like the column worker ``private_cli.compute_external_alignment`` (pyani_plus/private_cli.py:1930-2041)
and ``compute_external_alignment_column`` (pyani_plus/methods/external_alignment.py:33-156): same positional
signature, configuration checks, messages, JSON rows and row order, interrupt behaviour and return codes.

Where the reference parses the whole alignment twice per subject column and runs about ten numpy passes per pair,
this module reads the file once (``engine.load_msa``: md5 beside a parallel parse), bit-slices the rows on the device
and counts every pair it needs in one kernel call (``HipEngine.msa_upload`` / ``msa_pair_counts``); the host turns
the two counts per pair into the reference's five numbers (``msa_metrics``) and writes the rows natively
(``pa_append_msa_json``).  With ``subject_hash == ""`` all columns come from one symmetric device call.

Deviation: a compared row without residues makes the reference divide by zero (``ZeroDivisionError``); here the input
is refused up front with a message that names the row.
"""

from __future__ import annotations

import ctypes as C
import logging
from pathlib import Path

import numpy as np

from .. import _capi, wire
from .sourmash_hip import ExternalToolData, backend_failure, get_engine, log_sys_exit

METHOD = "external-alignment-hip"
RECORDING_FAILED = 2  # pyani_plus/private_cli.py:188
ROWS_PER_APPEND = 1 << 20  # rows formatted and appended to the column file per call (an interrupt keeps the finished ones)


def get_external_alignment_hip() -> ExternalToolData:
    """The "tool" of this method is the HIP shared library (as ``sourmash_hip.get_sourmash_hip``)."""
    from .. import __version__

    _capi.load_library()
    return ExternalToolData(_capi.LIB_PATH, __version__)


def filename_stem(filename: str) -> str:
    """The file name without directory, ``.gz`` and extension (pyani_plus/utils.py:93-105)."""
    if "/" in filename:
        filename = filename.rsplit("/", 1)[1]
    return Path(filename[:-3]).stem if filename.endswith(".gz") else Path(filename).stem


def record_name(title: bytes) -> str:
    """``title.decode().split(None, 1)[0]`` (external_alignment.py:66); an empty title has the empty name."""
    parts = title.decode().split(None, 1)
    return parts[0] if parts else ""


def make_extra(md5: str, label: str, alignment: Path) -> str:
    """``configuration.extra`` as the reference writes it (pyani_plus/public_cli.py:680-682): the file name last."""
    return f"md5={md5};label={label};alignment={Path(alignment).name}"


def _database_dir(session) -> Path | None:
    """Directory of the run's database: SQLAlchemy sessions (``session.bind.url``) and ``rundb.Session`` alike."""
    bind = getattr(session, "bind", None)
    if bind is not None:
        url = str(bind.url)
        if not url.startswith("sqlite:///"):
            msg = f"Expected SQLite3 URL to start sqlite:/// not {url}"
            raise ValueError(msg)
        return Path(url[10:]).parent
    conn = getattr(session, "conn", None)
    if conn is not None:
        for _seq, name, path in conn.execute("PRAGMA database_list"):
            if name == "main" and path:
                return Path(path).parent
    return None


def label_mapping(run, label: str):
    """Record name -> genome hash (private_cli.py:1996-2005)."""
    if label == "md5":
        return lambda x: x
    if label == "filename":
        return {_.fasta_filename: _.genome_hash for _ in run.fasta_hashes}.get
    return {filename_stem(_.fasta_filename): _.genome_hash for _ in run.fasta_hashes}.get


class MsaColumns:
    """The alignment as the column worker sees it: record names, their hashes, residue counts, and the device counts."""

    def __init__(self, logger: logging.Logger, msa, mapping, label: str, alignment: Path):
        self.msa = msa
        self.alignment = Path(alignment)
        self.names = [record_name(t) for t in msa.titles]
        self.hashes: list[str] = []
        for name in self.names:
            genome_hash = mapping(name)
            if not genome_hash:
                log_sys_exit(logger, f"Could not map {name} as {label}")
            self.hashes.append(genome_hash)
        self.rec_len = np.asarray(msa.lengths, dtype=np.int64)
        # non-gap bytes per record: the rows are padded with '-' up to the stride, so stride - (number of '-')
        self.n_residues = msa.rows.shape[1] - np.count_nonzero(msa.rows == ord("-"), axis=1).astype(np.int64)
        self.uniq = sorted(set(self.hashes))
        rank = {h: i for i, h in enumerate(self.uniq)}
        self.rank = np.array([rank[h] for h in self.hashes], dtype=np.int64)
        self.first_record: dict[str, int] = {}
        for i, h in enumerate(self.hashes):
            self.first_record.setdefault(h, i)
        self._wanted_for: tuple[frozenset, np.ndarray] | None = None

    def _wanted(self, query_set: set[str]) -> np.ndarray:
        key = frozenset(query_set)
        if self._wanted_for is None or self._wanted_for[0] != key:
            self._wanted_for = (key, np.array([h in query_set for h in self.uniq], dtype=bool))
        return self._wanted_for[1]

    def column_rows(self, logger: logging.Logger, subject_hash: str, query_set: set[str]):
        """(query record, subject record) of each row of one subject column, in the reference's order
        (external_alignment.py:95-156): file order, records below the subject or not asked for skipped, a self record
        one row, any other (q, s) then (s, q)."""
        s_rec = self.first_record.get(subject_hash)
        if s_rec is None:
            log_sys_exit(logger, f"Did not find subject {subject_hash} in {self.alignment.name}")
        s_rank = self.rank[s_rec]
        wanted = self._wanted(query_set)
        sel = np.flatnonzero((self.rank >= s_rank) & wanted[self.rank])
        self_row = self.rank[sel] == s_rank
        others = sel[~self_row]
        bad = others[self.rec_len[others] != self.rec_len[s_rec]]
        if bad.size:
            q = int(bad[0])
            log_sys_exit(
                logger,
                "Bad external-alignment, different lengths"
                f" {self.rec_len[q]} and {self.rec_len[s_rec]}"
                f" from {self.names[q]} and {self.names[s_rec]}``",
            )
        empty = others[self.n_residues[others] == 0]
        if others.size and (empty.size or self.n_residues[s_rec] == 0):
            q = int(empty[0]) if empty.size else s_rec
            log_sys_exit(logger, f"Bad external-alignment, {self.names[q]} has no residues in {self.alignment.name}")
        reps = np.where(self_row, 1, 2)
        q_rec = np.repeat(sel, reps)
        s_rec_rows = np.full(q_rec.size, s_rec, dtype=np.int64)
        # the second row of each pair is the mirror: (s, q)
        second = np.zeros(q_rec.size, dtype=bool)
        starts = np.cumsum(reps) - reps
        second[starts[~self_row] + 1] = True
        q_out = np.where(second, s_rec, q_rec)
        s_out = np.where(second, q_rec, s_rec_rows)
        return q_out, s_out, np.repeat(self_row, reps)


def column_values(cols: MsaColumns, q_rec, s_rec, is_self, match, both, subject_record: int | None):
    """The five numbers of each row: self rows (1.0, n, 0, 1.0, 1.0) as the reference yields them, the others from
    (M, B, n_q, n_s).  ``match`` / ``both``: [N records, 1] counts against ``subject_record``, or ([N, N], None)."""
    from ..engine import msa_metrics

    n = cols.n_residues
    other = ~is_self
    if subject_record is None:
        m, bo = match[q_rec, s_rec], both[q_rec, s_rec]
    else:  # M and B are symmetric: (q, s) and (s, q) both read the row of the record that is not the subject
        rec = np.where(s_rec == subject_record, q_rec, s_rec)
        m, bo = match[rec, 0], both[rec, 0]
    ident = np.ones(q_rec.size)
    aln = n[q_rec].astype(np.int64)
    err = np.zeros(q_rec.size, dtype=np.int64)
    covq = np.ones(q_rec.size)
    covs = np.ones(q_rec.size)
    if other.any():
        i, al, er, cq, cs = msa_metrics(m[other].view(np.uint32), bo[other].view(np.uint32), n[q_rec[other]], n[s_rec[other]])
        ident[other], aln[other], err[other], covq[other], covs[other] = i, al, er, cq, cs
    return ident, aln, err, covq, covs


class MsaColumnWriter:
    """The column file grown block by block (``pa_append_msa_json``): a complete JSON document after every block."""

    SUFFIX = "]}"

    def __init__(self, logger: logging.Logger, json_filename: Path, configuration, hashes: list[str]):
        self.logger = logger
        self.path = Path(json_filename)
        self.rows = 0
        self.hashes = hashes
        self._arr = (C.c_char_p * max(len(hashes), 1))(*[h.encode() for h in hashes])
        wire.export_json_matrices(logger, self.path, configuration, [], [], np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0), bool))

    def append(self, q_idx, s_idx, ident, aln, err, covq, covs) -> None:
        lib = _capi.load_library()
        q_idx = np.ascontiguousarray(q_idx, dtype=np.uint32)
        s_idx = np.ascontiguousarray(s_idx, dtype=np.uint32)
        arrays = [np.ascontiguousarray(x, dtype=d) for x, d in ((ident, np.float64), (aln, np.int64), (err, np.int64), (covq, np.float64), (covs, np.float64))]
        n = q_idx.size
        if n == 0:
            return
        _capi.check(
            lib.pa_append_msa_json(
                str(self.path).encode(), self.SUFFIX.encode(), int(self.rows > 0), self._arr, len(self.hashes), q_idx.ctypes.data, s_idx.ctypes.data,
                n, *(a.ctypes.data for a in arrays),
            ),  # fmt: skip
            "pa_append_msa_json",
        )
        self.rows += n
        self.logger.debug("Saved %d comparisons to %s", self.rows, self.path)


def check_configuration(logger: logging.Logger, run, session) -> tuple[Path, str, str]:
    """The checks of private_cli.py:1950-1990 for this method -> (alignment path, md5, label)."""
    configuration = run.configuration
    if configuration.method != METHOD:
        log_sys_exit(logger, f"Run-id {run.run_id} expected {configuration.method} results")
    tool = get_external_alignment_hip()
    if configuration.program != tool.exe_path.stem or configuration.version != tool.version:
        log_sys_exit(
            logger,
            f"Run configuration was {configuration.program} {configuration.version} but we have {tool.exe_path.stem} {tool.version}",
        )
    if not configuration.extra:
        log_sys_exit(logger, "Missing configuration.extra setting")
    try:
        args = dict(_.split("=", 1) for _ in configuration.extra.split(";", 2))
    except ValueError:
        args = {}
    if list(args) != ["md5", "label", "alignment"]:
        log_sys_exit(logger, f"configuration.extra={configuration.extra!r} unexpected")
    alignment = Path(args["alignment"])
    if not alignment.is_absolute():
        db_dir = _database_dir(session)
        if db_dir is not None:
            logger.debug("Treating %s as relative to %s", alignment, db_dir)
            alignment = db_dir / alignment
    return alignment, args["md5"], args["label"]


def load_alignment(logger: logging.Logger, run, session):
    """Configuration checks, then the alignment read once -> (MsaColumns, label)."""
    from ..engine import load_msa

    alignment, md5, label = check_configuration(logger, run, session)
    logger.info("Parsing %s (MD5=%s, label=%s)", alignment, md5, label)
    if not alignment.is_file():
        log_sys_exit(logger, f"Missing alignment file {alignment}")
    try:
        msa = load_msa(alignment)
    except _capi.HipBackendError as err:
        backend_failure(logger, f"{METHOD} alignment loading", err)
    if md5 != msa.md5:
        log_sys_exit(logger, f"MD5 checksum of {alignment} didn't match.")
    return MsaColumns(logger, msa, label_mapping(run, label), label, alignment), label


def compute_external_alignment_hip(  # noqa: PLR0913
    logger: logging.Logger,
    tmp_dir: Path,  # noqa: ARG001
    session,
    run,
    json_filename: Path,
    fasta_dir: Path,  # noqa: ARG001
    hash_to_filename: dict[str, str],  # noqa: ARG001
    filename_to_hash: dict[str, str],  # noqa: ARG001
    query_hashes: dict[str, int],
    subject_hash: str,
    *,
    cache: Path = Path(),  # noqa: ARG001
    engine=None,
) -> int:
    """One subject column (``subject_hash``) or, with ``subject_hash == ""``, every column of the run's genomes in
    sorted order, written to ``json_filename`` with the reference's rows in the reference's order.  A failing save
    returns 2; an interrupt keeps the rows written so far and marks the run "Worker interrupted"."""
    cols, _label = load_alignment(logger, run, session)
    query_set = set(query_hashes)
    subjects = [subject_hash] if subject_hash else sorted(query_set)
    try:
        writer = MsaColumnWriter(logger, json_filename, run.configuration, cols.uniq)
    except Exception:
        logger.exception("Unexpected exception saving JSON:")
        return RECORDING_FAILED
    try:
        plan = [(s, *cols.column_rows(logger, s, query_set)) for s in subjects]
        if not any(q.size for _s, q, _t, _u in plan):
            return 0
        eng = engine or get_engine()
        try:
            dm = eng.msa_upload(cols.msa)
            if subject_hash:
                subject_record = cols.first_record[subject_hash]
                match, both = eng.msa_pair_counts(dm, (0, cols.msa.n_rows), (subject_record, subject_record + 1))
            else:
                subject_record = None
                match, both = eng.msa_pair_counts(dm, symmetric=True)
            match, both = match.cpu().numpy(), both.cpu().numpy()
        except _capi.HipBackendError as err:
            backend_failure(logger, f"{METHOD} comparison", err)
        pending = []
        for _s, q_rec, s_rec_rows, is_self in plan:
            values = column_values(cols, q_rec, s_rec_rows, is_self, match, both, subject_record)
            pending.append((cols.rank[q_rec], cols.rank[s_rec_rows], *values))
            if sum(p[0].size for p in pending) >= ROWS_PER_APPEND:
                _flush(writer, pending)
                pending = []
        _flush(writer, pending)
    except _SaveFailed:
        logger.exception("Unexpected exception saving JSON:")
        return RECORDING_FAILED
    except KeyboardInterrupt:
        logger.error("Interrupted with %d completed %s comparisons", writer.rows, METHOD)  # noqa: TRY400
        run.status = "Worker interrupted"
        session.commit()
    return 0


class _SaveFailed(Exception):
    pass


def _flush(writer: MsaColumnWriter, pending: list) -> None:
    if not pending:
        return
    parts = [np.concatenate([p[i] for p in pending]) for i in range(7)]
    try:
        writer.append(*parts)
    except Exception as err:
        raise _SaveFailed from err
