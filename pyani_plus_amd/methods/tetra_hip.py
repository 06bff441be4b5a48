"""The ``TETRA-hip`` method: the correlations between the tetranucleotide usage Z-scores of all genome pairs.

The reference has no such method (pyani-plus wraps ANIm, dnadiff, ANIb, fastANI, sourmash, ...; TETRA is the fourth
classic method of pyani and is also offered by JSpecies).  The definition is this project's own contract, after Teeling
et al. 2004: ``include/pyani_hip.h`` states it, ``DESIGN.md`` section 7g explains it, ``tests/tetra_cases.py`` restates
it independently.  No bit parity with pyani or JSpecies is claimed.

The module is shaped like ``sourmash_hip``: ``prepare_genomes(logger, run, cache)`` leaves one small file per genome in
the cache, ``compute_tetra_hip(...)`` takes the reference's ten positional worker arguments and writes the JSON column
file its importer reads.  A row carries ``identity`` = r (NULL where either genome is degenerate) and NULL coverage:
TETRA has none, and unrelated genomes often correlate negatively, which a coverage column would turn into a negative
Hadamard value.

``engine`` None computes on the host (``pa_tetra_counts_host``, ``pa_tetra_corr_host``); a ``HipEngine`` computes the
counts and the correlations on its device, with the same bits.  The Z-scores are 256 values per genome and are always
computed on the host.
"""

from __future__ import annotations

import json
import logging
import os
from collections.abc import Iterator
from pathlib import Path

import numpy as np

from .. import __version__, _capi, wire
from .sourmash_hip import PREPARE_BATCH_BASES, RECORDING_FAILED, ExternalToolData, _check_tool_version, backend_failure, log_sys_exit

METHOD = "TETRA-hip"
DEVICE_TILE_COLUMNS = 2048  # subject columns evaluated (and flushed to the column file) per call


def get_tetra_hip() -> ExternalToolData:
    """The "tool" of this method is the HIP shared library: program and version are the library's."""
    _capi.load_library()
    return ExternalToolData(_capi.LIB_PATH, __version__)


def count_cache_dir(cache: Path) -> Path:
    return Path(cache) / "tetra_hip"


def count_file(cache: Path, genome_hash: str) -> Path:
    return count_cache_dir(cache) / f"{genome_hash}.json"


def write_counts(cache: Path, genome_hash: str, counts) -> Path:
    """The 336 forward counts of one genome as ``<cache>/tetra_hip/<md5>.json``: written under another name and renamed,
    so that a reader never sees half a file."""
    path = count_file(cache, genome_hash)
    counts = np.asarray(counts, dtype=np.uint64)
    assert counts.shape == (_capi.PA_TETRA_BINS,)
    tmp = path.with_name(f".{path.name}.{os.getpid()}.part")
    tmp.write_text(json.dumps({"genome_hash": genome_hash, "counts": [int(c) for c in counts]}))
    tmp.replace(path)
    return path


def read_counts(logger: logging.Logger, cache: Path, genome_hash: str) -> np.ndarray:
    path = count_file(cache, genome_hash)
    if not path.is_file():
        log_sys_exit(logger, f"Missing {METHOD} count file '{path}'")
    try:
        data = json.loads(path.read_text())
        counts = np.array(data["counts"], dtype=np.uint64)
        if data["genome_hash"] != genome_hash or counts.shape != (_capi.PA_TETRA_BINS,):
            raise ValueError(f"not the {_capi.PA_TETRA_BINS} counts of {genome_hash}")
    except (ValueError, KeyError, TypeError, OverflowError) as err:
        log_sys_exit(logger, f"Unreadable {METHOD} count file '{path}': {err}")
    return counts


def count_arena(arena, engine=None) -> np.ndarray:
    """Forward counts ``[n_genomes, 336]`` of a host arena: on ``engine``'s device, or on the host without one."""
    from ..engine import tetra_counts_host

    return tetra_counts_host(arena) if engine is None else engine.tetra_counts(arena)


def prepare_genomes(logger: logging.Logger, run, cache: Path, *, engine=None, precounted: dict | None = None) -> Iterator:
    """Write the count files of the run's genomes into ``cache/tetra_hip``; a file that is present is never recomputed.
    Yields the run's FASTA entries as their files are completed.  ``precounted`` = ``{genome_hash: counts}`` from a
    caller that has just read the files for their checksums (``rundb.run_tetra_hip``)."""
    config = run.configuration
    if config.method != METHOD:
        log_sys_exit(logger, f"Expected run to be for {METHOD}, not method {config.method}")
    if not Path(cache).is_dir():
        msg = f"Cache directory '{cache}' does not exist"
        raise ValueError(msg)
    count_cache_dir(cache).mkdir(exist_ok=True)
    fasta_dir = Path(run.fasta_directory)
    todo = []
    for entry in run.fasta_hashes:
        if count_file(cache, entry.genome_hash).is_file():
            yield entry
        elif precounted is not None and entry.genome_hash in precounted:
            write_counts(cache, entry.genome_hash, precounted[entry.genome_hash])
            yield entry
        else:
            todo.append(entry)
    if not todo:
        return
    from ..engine import load_fasta_files

    batches: list[list] = [[]]
    size = 0
    for entry in todo:
        path = fasta_dir / entry.fasta_filename
        est = (4 if path.name.endswith(".gz") else 1) * (path.stat().st_size if path.is_file() else 0)
        if batches[-1] and size + est > PREPARE_BATCH_BASES:
            batches.append([])
            size = 0
        batches[-1].append(entry)
        size += est
    for batch in batches:
        infos, arena = load_fasta_files([fasta_dir / e.fasta_filename for e in batch])
        for info in infos:
            if info.status != 0:
                log_sys_exit(logger, info.message)
        try:
            counts = count_arena(arena, engine)
        except _capi.HipBackendError as err:
            backend_failure(logger, f"{METHOD} counting", err)
        for entry, info, row in zip(batch, infos, counts):
            if info.md5 != entry.genome_hash:
                log_sys_exit(logger, f"{fasta_dir / entry.fasta_filename} has MD5 {info.md5}, the run recorded {entry.genome_hash}")
            write_counts(cache, entry.genome_hash, row)
            yield entry


def iter_tetra_tiles(logger: logging.Logger, subject_hashes, query_hashes, cache: Path, *, engine=None,
                     tile_columns: int = DEVICE_TILE_COLUMNS) -> Iterator[tuple]:  # fmt: skip
    """Yield ``(queries, tile_subjects, r)`` for one tile of subject columns after the other (sorted queries x sorted
    subjects; NaN where a genome is degenerate).  The count files are read once, the Z-scores and unit rows made once."""
    from ..engine import tetra_correlations_host, tetra_zscores

    queries, subjects = sorted(query_hashes), sorted(subject_hashes)
    if not queries or not subjects:
        return
    order = queries + sorted(set(subjects) - set(queries))  # queries first, then subjects not among them
    index = {h: i for i, h in enumerate(order)}
    counts = np.stack([read_counts(logger, cache, h) for h in order])
    _z, unit = tetra_zscores(counts)
    nq = len(queries)
    d_unit = unit if engine is None else engine._f64_on_device(unit)  # noqa: SLF001 - uploaded once for all tiles
    tile_columns = max(1, int(tile_columns))
    for t0 in range(0, len(subjects), tile_columns):
        tile = subjects[t0 : t0 + tile_columns]
        sub_idx = np.array([index[s] for s in tile])
        lo, hi = int(sub_idx.min()), int(sub_idx.max()) + 1
        if hi - lo != len(sub_idx):
            lo, hi = 0, len(order)  # scattered subjects: the covering block, columns picked below
        if engine is None:
            r = tetra_correlations_host(d_unit, (0, nq), (lo, hi))
        else:
            r = engine.tetra_correlations(d_unit, (0, nq), (lo, hi))
        yield queries, tile, np.ascontiguousarray(r[:, sub_idx - lo])


def compute_tetra_hip(  # noqa: PLR0913
    logger: logging.Logger,
    tmp_dir: Path,  # noqa: ARG001 - no intermediate files are needed
    session,
    run,
    json_filename: Path,
    fasta_dir: Path,  # noqa: ARG001
    hash_to_filename: dict[str, str],  # noqa: ARG001
    filename_to_hash: dict[str, str],  # noqa: ARG001
    query_hashes: dict[str, int],
    subject_hash: str = "",
    *,
    cache: Path = Path(),
    engine=None,
    tile_columns: int = DEVICE_TILE_COLUMNS,
) -> int:
    """Many-vs-subject (all-vs-all when ``subject_hash`` is empty) into the JSON column file: ``identity`` = r, NULL
    where a genome is degenerate; ``cov_query`` NULL; ``aln_length``, ``sim_errors`` and ``cov_subject`` unset.  The file
    grows by one tile of subject columns at a time and is complete JSON after each, so an interrupt keeps the finished
    tiles.  A failing library call ends the worker through ``log_sys_exit``; a failing save returns 2."""
    configuration = run.configuration
    _check_tool_version(logger, get_tetra_hip(), configuration)
    if not count_cache_dir(cache).is_dir():
        log_sys_exit(logger, f"Missing {METHOD} count directory '{count_cache_dir(cache)}' - check cache setting '{cache}'.")
    try:
        writer = wire.ColumnFileWriter(logger, json_filename, configuration)
    except Exception:
        logger.exception("Unexpected exception saving JSON:")
        return RECORDING_FAILED
    try:
        tiles = iter_tetra_tiles(logger, {subject_hash} if subject_hash else set(query_hashes), set(query_hashes), cache, engine=engine,
                                 tile_columns=tile_columns)  # fmt: skip
        for queries, subjects, r in tiles:
            try:
                writer.append_identity(queries, subjects, r)
            except Exception:
                logger.exception("Unexpected exception saving JSON:")
                return RECORDING_FAILED
    except KeyboardInterrupt:
        logger.error("Interrupted with %d completed %s comparisons", writer.rows, METHOD)  # noqa: TRY400
        run.status = "Worker interrupted"
        session.commit()
    except _capi.HipBackendError as err:
        backend_failure(logger, f"{METHOD} comparison", err)
    return 0
