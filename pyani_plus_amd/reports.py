"""The reports of a recorded run: the build's own counterpart of ``export-run``, ``plot-run`` and ``plot-run-comp``
(their tables; pyani_plus/plot_run.py) and ``classify`` (pyani_plus/public_cli.py:974-1091, 1095-1208, 1211-1331), and
this project's ``tree-run``, ``bootstrap-run``, ``phylo-run``, ``ordinate-run``, ``mantel-run-comp`` and ``dereplicate-run``.  They read the database through ``run_store`` and compute in the
report modules (``classify``, ``cluster``, ``distribution``, ``scatter``, ``run_comp``, ``tree``, ``substitution``, ``ordination``, ``mantel``,
``dereplicate`` and the figure modules); ``rundb`` re-exports them and is their command line, and nothing here imports it.

Every command opens the same way -- the database is there, the image formats can be drawn, the output directory is
made, the run is there and complete, the labels are known and distinct -- and each check is stated once below.  The
order in which a command makes them is behaviour: it decides which message two failures give and what is written by then."""

from __future__ import annotations

import importlib
import logging
import math
from io import StringIO
from pathlib import Path

import numpy as np

from . import _capi
from . import bootstrap as bootstrap_mod
from . import classify as classify_mod
from . import cluster as cluster_mod
from . import dereplicate as dereplicate_mod
from . import distribution as distribution_mod
from . import distribution_figure, heatmap_figure, ordination_figure, run_comp_figure, scatter_figure
from . import mantel as mantel_mod
from . import ordination as ordination_mod
from . import run_comp as run_comp_mod
from . import scatter as scatter_mod
from . import substitution as substitution_mod
from . import tree as tree_mod
from ._capi import HipBackendError
from .methods import external_alignment_hip, sourmash_hip
from .methods.external_alignment_hip import filename_stem
from .run_store import (Run, _comparison_matrices, _matrix_cache_too_big, _open_run, _select_run_comparisons, cache_comparisons,
                        count_run_comparisons, genome_lengths, load_run)  # fmt: skip


# ------------------------------------------------------------------ how every report opens
def _require_database(logger, database) -> None:
    if str(database) == ":memory:" or not Path(database).is_file():
        sourmash_hip.log_sys_exit(logger, f"Database {database} does not exist")


def _image_formats(logger, formats) -> tuple[tuple[str, ...], list[str]]:
    """``(formats, the image formats among them)``; an image format needs matplotlib."""
    formats = tuple(formats)
    images = [ext for ext in formats if ext != "tsv"]
    if images:
        try:
            importlib.import_module("matplotlib")
        except ImportError:
            sourmash_hip.log_sys_exit(logger, f"Image formats ({', '.join(images)}) need matplotlib, which cannot be imported; only tsv is available")
    return formats, images


def _make_outdir(logger, outdir) -> Path:
    outdir = Path(outdir)
    if not outdir.is_dir():
        logger.warning("Output directory %s does not exist, making it.", outdir)
        outdir.mkdir()
    return outdir


def _require_genomes(logger, run: Run) -> int:
    if not run.fasta_hashes:
        sourmash_hip.log_sys_exit(logger, f"Run-id {run.run_id} has no genomes")
    return len(run.fasta_hashes)


def _require_complete(logger, run: Run, done: int) -> None:
    """``done`` comparisons are all of the run's (db_orm.load_run(check_complete=True))."""
    n = len(run.fasta_hashes)
    if done != n * n:
        sourmash_hip.log_sys_exit(logger, f"run-id {run.run_id} has {done} of {n}^2={n * n} comparisons, {n * n - done} needed")


def _open_complete_run(logger, database, run_id: int | None, doing: str) -> tuple:
    """``(connection, run, its number of genomes n, its n^2 comparisons)`` of a run that has genomes and is complete."""
    conn, run = _open_run(logger, database, run_id, doing)
    done = count_run_comparisons(conn, run)
    n = _require_genomes(logger, run)
    _require_complete(logger, run, done)
    return conn, run, n, done


# ------------------------------------------------------------------ labels (``Run.relabelled_matrix``, db_orm.py:590-624)
def _label_mapping(logger, run: Run, label: str) -> dict[str, str]:
    """genome_hash -> the genome's label under the scheme ``md5``, ``filename`` or ``stem``."""
    if label == "md5":
        return {a.genome_hash: a.genome_hash for a in run.fasta_hashes}
    if label == "filename":
        return {a.genome_hash: a.fasta_filename for a in run.fasta_hashes}
    if label == "stem":
        return {a.genome_hash: filename_stem(a.fasta_filename) for a in run.fasta_hashes}
    sourmash_hip.log_sys_exit(logger, f"Unexpected label scheme {label!r}")


def _require_distinct_stems(logger, label: str, mapping: dict[str, str]) -> None:
    if label == "stem" and len(set(mapping.values())) < len(mapping):
        sourmash_hip.log_sys_exit(logger, "Duplicate filename stems, consider using MD5 labelling.")


def _relabel(frame, label: str, mapping: dict[str, str]):
    """A frame over md5 labelled by ``mapping`` and sorted by label on both axes (``md5``: as it is)."""
    return frame if label == "md5" else frame.rename(index=mapping, columns=mapping).sort_index(axis=0).sort_index(axis=1)


def _relabelled(logger, run: Run, frames: list, label: str) -> list:
    """Every frame relabelled, with the reference's messages for an unknown label and duplicate stems."""
    mapping = _label_mapping(logger, run, label)
    _require_distinct_stems(logger, label, mapping)
    return [_relabel(frame, label, mapping) for frame in frames]


# ------------------------------------------------------------------ the matrices of a complete run
def _cached_frames(logger, conn, run: Run, kinds: tuple[str, ...]) -> list:
    """The cached ``runs.df_<kind>`` strings (10 decimals) as frames over sorted md5, filled first when they are missing."""
    import pandas as pd

    columns = [f"df_{kind}" for kind in kinds]
    cached = conn.execute(f"SELECT {', '.join(columns)} FROM runs WHERE run_id=?", (run.run_id,)).fetchone()
    if any(c is None for c in cached):
        out = cache_comparisons(conn, run)
        cached = tuple(out.get(column) for column in columns)
        if any(c is None for c in cached):
            sourmash_hip.log_sys_exit(logger, f"Could not load run {run.configuration.method} matrix")
    return [pd.read_json(StringIO(c), orient="split", dtype=float) for c in cached]


def _score_frames(logger, conn, run: Run) -> list:
    """The identity, query coverage and Hadamard matrices of a complete run as frames over sorted md5: the cached ones;
    for a run too large for the cache, the comparisons table, unrounded."""
    import pandas as pd

    kinds = ("identity", "cov_query", "hadamard")
    if _matrix_cache_too_big(len(run.fasta_hashes)):
        hashes, mats = _comparison_matrices(conn, run)
        mats["hadamard"] = mats["identity"] * mats["cov_query"]
        return [pd.DataFrame(mats[k], index=hashes, columns=hashes) for k in kinds]
    return _cached_frames(logger, conn, run, kinds)


# ------------------------------------------------------------------ export-run (pyani_plus/public_cli.py:974-1091)
def export_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem",
               logger: logging.Logger | None = None) -> list[Path]:
    """Write ``<method>_run_<id>.tsv`` (long form) and the six matrices ``<method>_{identity,aln_lengths,sim_errors,
    query_cov,hadamard,tANI}.tsv`` of a run, byte for byte what the reference's ``export-run`` writes from the same
    database: long form in ``Run.comparisons()`` order with ``NA`` for NULL and Python ``str(float)``; matrices from
    the cached ``df_*`` strings through pandas ``to_csv(sep="\t")``, labelled by ``md5``, ``filename`` or ``stem`` and
    sorted by label (db_orm.py:590-624).  A partial run gets the long form only and then the reference's error."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    outdir = _make_outdir(logger, outdir)
    conn, run = _open_run(logger, database, run_id, "Exporting")
    _require_genomes(logger, run)
    method = run.configuration.method
    mapping = _label_mapping(logger, run, label)

    def float_or_na(value) -> str:
        return "NA" if value is None else str(value)

    written = [outdir / f"{method}_run_{run.run_id}.tsv"]
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
    _require_complete(logger, run, len(rows))  # only now: a partial run has its long form
    frames = _cached_frames(logger, conn, run, ("identity", "aln_length", "sim_errors", "cov_query", "hadamard"))
    with np.errstate(divide="ignore", invalid="ignore"):
        frames.append(-np.log(frames[4]))  # tANI = -ln(hadamard), not cached (db_orm.py:566-588)
    _require_distinct_stems(logger, label, mapping)
    for frame, kind in zip(frames, ("identity", "aln_lengths", "sim_errors", "query_cov", "hadamard", "tANI")):
        written.append(outdir / f"{method}_{kind}.tsv")
        _relabel(frame, label, mapping).to_csv(written[-1], sep="\t")
    logger.info("Wrote matrices to %s/%s_*.tsv", outdir, method)
    conn.close()
    return written


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
    _require_database(logger, database)
    for name, role in ((coverage_edges, "coverage"), (score_edges, "score")):
        if name not in classify_mod.AGG_NAMES:
            sourmash_hip.log_sys_exit(logger, f"Unknown {role} aggregator {name!r}: expected one of {', '.join(classify_mod.AGG_NAMES)}")
    if mode not in classify_mod.MODES:
        sourmash_hip.log_sys_exit(logger, f"Unknown classify mode {mode!r}: expected one of {', '.join(classify_mod.MODES)}")
    outdir = _make_outdir(logger, outdir)
    conn, run, n, done = _open_complete_run(logger, database, run_id, "Exporting")
    frames = _score_frames(logger, conn, run)
    conn.close()
    if done == 1 and n == 1:
        logger.warning("Run %d has %d comparison across %d genome. Reporting single clique.", run.run_id, done, n)
    else:
        logger.info("Run %d has %d comparisons across %d genomes.", run.run_id, done, n)
    identity, cov, hadamard = _relabelled(logger, run, frames, label)
    score = identity.to_numpy(dtype=float) if mode == "identity" else classify_mod.tani_scores(hadamard.to_numpy(dtype=float))
    rows = classify_mod.classify_matrices([str(x) for x in cov.columns], score, cov.to_numpy(dtype=float), coverage_edges=coverage_edges,
                                          score_edges=score_edges, cov_min=cov_min, engine=engine)
    written = outdir / f"{run.configuration.method}_classify.tsv"
    written.write_text(classify_mod.classify_tsv(rows, mode))
    logger.info("Wrote classify output to %s", outdir)
    return written


# ------------------------------------------------------------------ a run's distances (tree-run, ordinate-run)
def _require_missing_distance(logger, missing: float) -> None:
    if not (math.isfinite(missing) and missing >= 0):
        sourmash_hip.log_sys_exit(logger, f"The distance of a pair without identity must be finite and not negative, not {missing!r}")


def _require_no_negative_distance(logger, distances: np.ndarray, what: str) -> None:
    if (distances < 0).any():
        sourmash_hip.log_sys_exit(logger, f"An identity above 1 gives a negative distance: no {what} is defined")


def _distance_run(logger, database, outdir, run_id: int | None, label: str, missing: float, what: str):  # noqa: PLR0913
    """What tree-run and ordinate-run start from: ``(outdir, method, identity, distances)`` of a complete run -- the
    output directory made, the run opened and checked, its identity frame relabelled and sorted by label as ``classify``
    and ``plot-run`` read it, and ``tree.run_distances`` of it -- with the reference's messages for an incomplete run,
    duplicate stems and an unknown label.  ``what`` is the thing an identity above 1 leaves undefined."""
    _require_missing_distance(logger, missing)
    outdir = _make_outdir(logger, outdir)
    conn, run, n, done = _open_complete_run(logger, database, run_id, "Exporting")
    frames = _score_frames(logger, conn, run)
    conn.close()
    logger.info("Run %d has %d comparisons across %d genomes.", run.run_id, done, n)
    identity = _relabelled(logger, run, frames, label)[0]
    distances = tree_mod.run_distances(identity, missing, logger)
    _require_no_negative_distance(logger, distances, what)
    return outdir, run.configuration.method, identity, distances


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


# ------------------------------------------------------------------ bootstrap-run (this project's own: the reference writes no support)
def _bootstrap_alignment(logger, run: Run, conn, alignment: Path | None, hashes: list[str], who: str = "bootstrap-run"):
    """The run's alignment as ``engine.LoadedMSA`` with one row per genome, in the order of ``hashes``: found and checked
    as the column worker does (``external_alignment_hip.check_configuration``: next to the database unless ``alignment``
    says where; the md5 is the configuration's either way), a genome's row being its first record."""
    from types import SimpleNamespace

    from . import engine as engine_mod

    found, md5, msa_label = external_alignment_hip.check_configuration(logger, run, SimpleNamespace(conn=conn))
    path = Path(alignment) if alignment is not None else found
    logger.info("Parsing %s (MD5=%s, label=%s)", path, md5, msa_label)
    if not path.is_file():
        sourmash_hip.log_sys_exit(logger, f"Missing alignment file {path}")
    try:
        msa = engine_mod.load_msa(path)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, f"{who} alignment loading", err)
    if md5 != msa.md5:
        sourmash_hip.log_sys_exit(logger, f"MD5 checksum of {path} didn't match.")
    cols = external_alignment_hip.MsaColumns(logger, msa, external_alignment_hip.label_mapping(run, msa_label), msa_label, path)
    records = []
    for genome_hash in hashes:
        if genome_hash not in cols.first_record:
            sourmash_hip.log_sys_exit(logger, f"Did not find genome {genome_hash} in {path.name}")
        records.append(cols.first_record[genome_hash])
    lengths = cols.rec_len[records]
    if (lengths != msa.n_cols).any():
        short = records[int(np.flatnonzero(lengths != msa.n_cols)[0])]
        sourmash_hip.log_sys_exit(logger, f"Bad external-alignment, different lengths {cols.rec_len[short]} and {msa.n_cols} from {cols.names[short]} in {path.name}")
    rows = np.ascontiguousarray(msa.rows[records])
    return engine_mod.LoadedMSA(msa.md5, [msa.titles[r] for r in records], msa.lengths[records], msa.histogram, rows, msa.n_cols)


def _labelled_alignment(logger, conn, run: Run, n: int, done: int, label: str, alignment: Path | None, who: str):  # noqa: PLR0913
    """``(identity, labels, msa)`` of a complete external-alignment-hip run: its identity frame relabelled and sorted by
    label as ``tree-run`` reads it, the labels in that order, and the run's alignment (``_bootstrap_alignment``) with a
    row per genome in the same order.  Closes ``conn``."""
    try:
        frames = _score_frames(logger, conn, run)
        logger.info("Run %d has %d comparisons across %d genomes.", run.run_id, done, n)
        mapping = _label_mapping(logger, run, label)
        identity = _relabelled(logger, run, frames, label)[0]
        labels = [str(x) for x in identity.columns]
        hash_of = {str(shown): genome_hash for genome_hash, shown in mapping.items()}
        msa = _bootstrap_alignment(logger, run, conn, alignment, [hash_of[x] for x in labels], who)
    finally:
        conn.close()
    return identity, labels, msa


def bootstrap_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", replicates: int = 100, seed: int = 0,  # noqa: PLR0913
                  missing: float = 1.0, alignment: Path | None = None, keep_trees: bool = False, engine=None,
                  logger: logging.Logger | None = None) -> list[Path]:
    """Column-bootstrap support of ``tree-run``'s neighbour-joining tree of a complete ``external-alignment-hip`` run
    (``bootstrap.bootstrap``): ``replicates`` (1 to 100 000) times the columns of the run's
    alignment are drawn anew with replacement from ``seed`` (0 to 2^64 - 1), the tree is rebuilt from the distances
    ``1 - identity`` of the drawn columns (``missing`` where a pair has no aligned column left), and every edge of
    ``tree-run``'s tree is given the number of rebuilt trees that have it.  The genomes are in the order of
    ``tree-run``'s matrix under the same ``label``; the alignment is looked for next to the database, as the worker
    does, or at ``alignment``, and its md5 is checked against the run's configuration.  A run of another method has no
    columns to resample, and fewer than 4 genomes have no internal edge: each ends with its message.

    * ``<method>_identity_nj_bootstrap.nwk``: ``tree-run``'s tree, every internal node but the root of the text labelled
      with the support of the edge above it, a count and not a percentage;
    * ``<method>_identity_nj_bootstrap.tsv``: ``#node n_leaves length support replicates``, a line per labelled node;
    * with ``keep_trees``, ``<method>_identity_nj_replicates.nwk``: a replicate tree per line, in replicate order.

    ``engine``: a ``HipEngine`` makes the weighted counts, the distances and the joins on the GPU; None makes them on
    the host, with the same bytes.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    if isinstance(replicates, bool) or not isinstance(replicates, int) or not 1 <= replicates <= bootstrap_mod.MAX_REPLICATES:
        sourmash_hip.log_sys_exit(logger, f"Expected 1 to {bootstrap_mod.MAX_REPLICATES} replicates, not {replicates!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        sourmash_hip.log_sys_exit(logger, f"Expected a seed from 0 to 2^64 - 1, not {seed!r}")
    _require_missing_distance(logger, missing)
    outdir = _make_outdir(logger, outdir)
    conn, run, n, done = _open_complete_run(logger, database, run_id, "Exporting")
    method = run.configuration.method
    if method != external_alignment_hip.METHOD:
        sourmash_hip.log_sys_exit(
            logger, f"Run-id {run.run_id} is a {method} run: it has no columns to resample (bootstrap-run needs an {external_alignment_hip.METHOD} run)")
    if n < 4:  # noqa: PLR2004
        sourmash_hip.log_sys_exit(logger, f"Run-id {run.run_id} has {n} genomes: a tree of fewer than 4 has no internal edge to support")
    identity, labels, msa = _labelled_alignment(logger, conn, run, n, done, label, alignment, "bootstrap-run")
    distances = tree_mod.run_distances(identity, missing, logger)
    _require_no_negative_distance(logger, distances, "tree")
    try:
        table = tree_mod.neighbour_joining(distances, engine=engine)
        device_msa = engine.msa_upload(msa) if engine is not None else None
        result = bootstrap_mod.bootstrap(table, msa.rows, msa.n_cols, replicates, seed, missing, engine=engine, device_msa=device_msa)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "bootstrap-run", err)
    stem = f"{method}_identity_nj"
    written = [outdir / f"{stem}_bootstrap.nwk", outdir / f"{stem}_bootstrap.tsv"]
    written[0].write_text(bootstrap_mod.support_newick(result, labels) + "\n")
    written[1].write_text(bootstrap_mod.support_tsv(result))
    if keep_trees:
        written.append(outdir / f"{stem}_replicates.nwk")
        written[-1].write_text("".join(tree_mod.newick(t, labels) + "\n" for t in result.trees))
    logger.info("Wrote the support of %d edges among %d replicates to %s", max(n - 3, 0), replicates, written[0])
    return written


# ------------------------------------------------------------------ phylo-run (this project's own: the reference has no substitution distance)
def phylo_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem", model: str = substitution_mod.DEFAULT_MODEL,  # noqa: PLR0913
              missing: float = substitution_mod.DEFAULT_MISSING, replicates: int = 0, seed: int = 0, alignment: Path | None = None,
              keep_trees: bool = False, engine=None, logger: logging.Logger | None = None) -> list[Path]:
    """Substitution distances of the genomes of a complete ``external-alignment-hip`` run from its alignment, their
    neighbour-joining tree and, with ``replicates`` (0 to 100 000), its column bootstrap (``substitution.phylo``;
    DESIGN.md section 7m).  ``model`` is "p" (the share of differing columns among those with a nucleotide in both
    rows), "jc69" or "k80"; a pair without such a column, or one too diverged for the model's logarithm, gets the
    distance ``missing``, and both kinds are counted in the log.  The genomes are in the order of ``tree-run``'s matrix
    under the same ``label``; the alignment is found and checked as ``bootstrap-run`` does, and ``seed`` draws the
    columns ``bootstrap-run`` draws.  A run of another method has no columns, and fewer than 4 genomes have no internal
    edge to support: each ends with ``bootstrap-run``'s message.

    * ``<method>_<model>_distances.tsv``: the labelled square matrix, values as ``repr``;
    * ``<method>_<model>_nj.nwk``: its neighbour-joining tree;
    * with replicates, ``<method>_<model>_nj_bootstrap.nwk`` and ``<method>_<model>_nj_bootstrap.tsv`` as
      ``bootstrap-run`` writes them, and with ``keep_trees`` ``<method>_<model>_nj_replicates.nwk``.

    ``engine``: a ``HipEngine`` makes the counts, the distances and the joins on the GPU; None makes them on the host,
    with the same bytes.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    if model not in substitution_mod.MODELS:
        sourmash_hip.log_sys_exit(logger, f"Unknown substitution model {model!r}: expected one of {', '.join(substitution_mod.MODELS)}")
    if isinstance(replicates, bool) or not isinstance(replicates, int) or not 0 <= replicates <= bootstrap_mod.MAX_REPLICATES:
        sourmash_hip.log_sys_exit(logger, f"Expected 0 to {bootstrap_mod.MAX_REPLICATES} replicates, not {replicates!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        sourmash_hip.log_sys_exit(logger, f"Expected a seed from 0 to 2^64 - 1, not {seed!r}")
    _require_missing_distance(logger, missing)
    outdir = _make_outdir(logger, outdir)
    conn, run, n, done = _open_complete_run(logger, database, run_id, "Exporting")
    method = run.configuration.method
    if method != external_alignment_hip.METHOD:
        sourmash_hip.log_sys_exit(
            logger, f"Run-id {run.run_id} is a {method} run: it has no columns to resample (phylo-run needs an {external_alignment_hip.METHOD} run)")
    if replicates and n < 4:  # noqa: PLR2004
        sourmash_hip.log_sys_exit(logger, f"Run-id {run.run_id} has {n} genomes: a tree of fewer than 4 has no internal edge to support")
    _identity, labels, msa = _labelled_alignment(logger, conn, run, n, done, label, alignment, "phylo-run")
    try:
        device_msa = engine.msa_subst_upload(msa) if engine is not None else None
        result = substitution_mod.phylo(msa.rows, msa.n_cols, model, missing, replicates, seed, engine=engine, device_msa=device_msa)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "phylo-run", err)
    logger.info("%s distances of %d genomes: %d pairs without a shared nucleotide column, %d saturated pairs (distance %r)", model, n,
                result.no_columns, result.saturated, float(missing))
    stem = f"{method}_{model}"
    written = [outdir / f"{stem}_distances.tsv", outdir / f"{stem}_nj.nwk"]
    written[0].write_text(substitution_mod.distances_tsv(result.distances, labels))
    written[1].write_text(tree_mod.newick(result.table, labels) + "\n")
    if result.bootstrap is not None:
        written += [outdir / f"{stem}_nj_bootstrap.nwk", outdir / f"{stem}_nj_bootstrap.tsv"]
        written[2].write_text(bootstrap_mod.support_newick(result.bootstrap, labels) + "\n")
        written[3].write_text(bootstrap_mod.support_tsv(result.bootstrap))
        if keep_trees:
            written.append(outdir / f"{stem}_nj_replicates.nwk")
            written[-1].write_text("".join(tree_mod.newick(t, labels) + "\n" for t in result.bootstrap.trees))
        logger.info("Wrote the support of %d edges among %d replicates to %s", max(n - 3, 0), replicates, written[2])
    logger.info("Wrote %s distances and their tree to %s", model, outdir)
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
    formats, images = _image_formats(logger, formats)
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


def _write_scatter_tables(logger, conn, run: Run, outdir: Path, genome_lengths: dict[str, int]) -> list[Path]:
    """``<method>_{query_cov,tANI}_scatter.tsv`` (pyani_plus/plot_run.py:231-293): identity, the y value and the query's
    length of every comparison that has both, unrounded, in ``comparison_id`` order, numbers as Python's ``str``."""
    method = run.configuration.method
    rows = [
        (identity, cov_query, genome_lengths[query])
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
    _require_database(logger, database)
    formats, images = _image_formats(logger, formats)
    if scatter and not 1 <= int(scatter_bins) <= scatter_mod.MAX_BINS:
        sourmash_hip.log_sys_exit(logger, f"--scatter-bins {scatter_bins}: expected 1 to {scatter_mod.MAX_BINS}")
    outdir = _make_outdir(logger, outdir)
    conn, run, n, _done = _open_complete_run(logger, database, run_id, "Plotting")
    method = run.configuration.method
    frames = dict(zip(("identity", "query_cov", "hadamard"), _relabelled(logger, run, _score_frames(logger, conn, run), label)))
    genome_lengths = dict(conn.execute("SELECT genome_hash, length FROM genomes"))  # of the queries: both kinds of scatter output show them
    written = _write_scatter_tables(logger, conn, run, outdir, genome_lengths) if "tsv" in formats else []
    scatter_tables = len(written)
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
        by_label = {labelled: genome_lengths[md5] for md5, labelled in _label_mapping(logger, run, label).items()}
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


def _parse_run_ids(logger, run_ids) -> list[int]:
    """The runs of a comparison, the reference run first: a comma separated string, or integers."""
    try:
        runs = [int(x) for x in (run_ids.split(",") if isinstance(run_ids, str) else run_ids)]
    except (TypeError, ValueError):
        sourmash_hip.log_sys_exit(logger, f"Expected comma separated list of runs, not: {run_ids}")
    if len(runs) < 2:  # noqa: PLR2004
        sourmash_hip.log_sys_exit(logger, "Need at least two runs for a comparison")
    return runs


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
    _require_database(logger, database)
    formats, images = _image_formats(logger, formats)
    outdir = _make_outdir(logger, outdir)
    runs = _parse_run_ids(logger, run_ids)
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


# ------------------------------------------------------------------ mantel-run-comp (this project's own: the reference gives no number)
def mantel_run_comp(database: Path | str, outdir: Path, run_ids, *, permutations: int = 9999, seed: int = 0, missing: float = 1.0,  # noqa: PLR0913
                    engine=None, logger: logging.Logger | None = None) -> list[Path]:
    """Mantel's permutation test (``mantel.mantel_test``) between complete runs of one database:
    the first of ``run_ids`` (a comma separated string, or integers) is the reference run, and each further run is
    compared with it over the genomes both runs hold (their hashes, sorted; at least 3).  A run's distances are the ones
    ``tree-run`` uses (``tree.run_distances`` of its identity matrix; ``missing`` where a pair has no identity either
    way), restricted to those genomes.  ``permutations`` (0 to 1 000 000) permutations of the other run's genomes come
    from ``seed`` (0 to 2^64 - 1).

    * ``<method>_identity_<ref>_mantel.tsv``: ``#run_id method name genomes pairs mantel_r permutations seed
      at_least_observed p_value``, one line per other run, floats as ``repr``, ``NA`` where a run's distances are all
      equal;
    * ``<method>_identity_<ref>_vs_<other>_mantel_null.tsv`` for every other run: ``#permutation mantel_r``, one line per
      permutation (with ``NA`` above, the header alone).

    ``engine``: a ``HipEngine`` makes the cross sums on the GPU; None makes them on the host, with the same bytes.
    Returns the written paths, the summary first."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    if isinstance(permutations, bool) or not isinstance(permutations, int) or not 0 <= permutations <= mantel_mod.MAX_PERMUTATIONS:
        sourmash_hip.log_sys_exit(logger, f"Expected 0 to {mantel_mod.MAX_PERMUTATIONS} permutations, not {permutations!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        sourmash_hip.log_sys_exit(logger, f"Expected a seed from 0 to 2^64 - 1, not {seed!r}")
    _require_missing_distance(logger, missing)
    outdir = _make_outdir(logger, outdir)
    runs = _parse_run_ids(logger, run_ids)
    opened = []
    for run_id in runs:
        conn, run, n, done = _open_complete_run(logger, database, run_id, "Comparing")
        identity = _score_frames(logger, conn, run)[0]
        conn.close()
        logger.info("Run %d has %d comparisons across %d genomes.", run.run_id, done, n)
        opened.append((run, identity))
    ref_run, ref_identity = opened[0]
    method = ref_run.configuration.method

    def distances(identity, hashes: list[str]) -> np.ndarray:
        d = tree_mod.run_distances(identity.loc[hashes, hashes], missing, logger)
        _require_no_negative_distance(logger, d, "Mantel test")
        return d

    lines, written = [], [outdir / f"{method}_identity_{ref_run.run_id}_mantel.tsv"]
    try:
        for run, identity in opened[1:]:
            common = sorted({a.genome_hash for a in ref_run.fasta_hashes} & {a.genome_hash for a in run.fasta_hashes})
            if len(common) < 3:  # noqa: PLR2004
                sourmash_hip.log_sys_exit(
                    logger, f"Runs {ref_run.run_id} and {run.run_id} have {len(common)} genomes in common: a Mantel test needs at least 3")
            test = mantel_mod.mantel_test(distances(ref_identity, common), distances(identity, common), permutations, seed, engine=engine, logger=logger)
            logger.info("%s run %d vs %s run %d over %d genomes: Mantel r %s, p %s", run.configuration.method, run.run_id, method, ref_run.run_id,
                        len(common), test.r, test.p)
            lines.append(mantel_mod.summary_line(run.run_id, run.configuration.method, run.name, test))
            written.append(outdir / f"{method}_identity_{ref_run.run_id}_vs_{run.run_id}_mantel_null.tsv")
            mantel_mod.write_null_tsv(written[-1], test)
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "mantel-run-comp", err)
    mantel_mod.write_summary_tsv(written[0], lines)
    logger.info("Wrote %d tables to %s/%s_identity_%d_*mantel*.tsv", len(written), outdir, method, ref_run.run_id)
    return written


# ------------------------------------------------------------------ dereplicate-run (this project's own: the reference picks no representatives)
def dereplicate_run(database: Path | str, outdir: Path, *, run_id: int | None = None, label: str = "stem",  # noqa: PLR0913
                    min_identity: float = dereplicate_mod.MIN_IDENTITY, cov_min: float = classify_mod.MIN_COVERAGE, score_edges: str = "mean",
                    coverage_edges: str = "min", mode: str = "greedy", prefer: str = "length", engine=None,
                    logger: logging.Logger | None = None) -> list[Path]:
    """One representative genome per group of a complete run (``dereplicate.dereplicate_matrices``; DESIGN.md section
    7k): two genomes are adjacent when their aggregated identity is at least ``min_identity`` and their aggregated query
    coverage above ``cov_min`` -- the graph ``classify`` has at the moment its ``min_identity`` column reads that value.
    ``mode`` "greedy" walks the genomes in order of preference and keeps one that no kept genome is adjacent to (the
    galah / skDER rule); "cover" chooses again and again the genome whose neighbourhood holds the most genomes not yet
    represented.  Every other genome goes to the adjacent representative of the highest identity.  ``prefer`` "length"
    puts the longer genome first (ties by label), "label" is label order.  The matrices and labels are the ones
    ``classify`` reads, with the reference's messages for a missing database, an incomplete run, duplicate stems and an
    unknown label.

    * ``<method>_dereplicate.tsv``: ``genome, representative, identity, length``, a row per genome, grouped by
      representative in order of preference, the representative's own row first;
    * ``<method>_representatives.tsv``: ``representative, n_members, length, min_identity``, a row per representative.

    ``engine``: a ``HipEngine`` builds the graph, selects and assigns on the GPU; None does so on the host, with the
    same bytes.  Returns the written paths."""
    logger = logger or logging.getLogger("pyani_plus_amd")
    _require_database(logger, database)
    for value, what in ((min_identity, "identity"), (cov_min, "coverage")):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or math.isnan(value):
            sourmash_hip.log_sys_exit(logger, f"The minimum {what} must be a number, not {value!r}")
    for name, role in ((coverage_edges, "coverage"), (score_edges, "score")):
        if name not in classify_mod.AGG_NAMES:
            sourmash_hip.log_sys_exit(logger, f"Unknown {role} aggregator {name!r}: expected one of {', '.join(classify_mod.AGG_NAMES)}")
    if mode not in dereplicate_mod.MODES:
        sourmash_hip.log_sys_exit(logger, f"Unknown dereplication mode {mode!r}: expected one of {', '.join(dereplicate_mod.MODES)}")
    if prefer not in dereplicate_mod.PREFERENCES:
        sourmash_hip.log_sys_exit(logger, f"Unknown preference {prefer!r}: expected one of {', '.join(dereplicate_mod.PREFERENCES)}")
    outdir = _make_outdir(logger, outdir)
    conn, run, n, done = _open_complete_run(logger, database, run_id, "Exporting")
    frames = _score_frames(logger, conn, run)
    lengths = genome_lengths(conn, run)
    conn.close()
    logger.info("Run %d has %d comparisons across %d genomes.", run.run_id, done, n)
    mapping = _label_mapping(logger, run, label)
    identity, cov, _hadamard = _relabelled(logger, run, frames, label)
    labels = [str(x) for x in cov.columns]
    length_of = {str(mapping[h]): lengths[h] for h in mapping}
    try:
        result = dereplicate_mod.dereplicate_matrices(labels, [length_of[x] for x in labels], identity.to_numpy(dtype=float), cov.to_numpy(dtype=float),
                                                      prefer=prefer, min_identity=min_identity, cov_min=cov_min, score_edges=score_edges,
                                                      coverage_edges=coverage_edges, mode=mode, engine=engine)  # fmt: skip
    except HipBackendError as err:
        sourmash_hip.backend_failure(logger, "dereplicate-run", err)
    written = dereplicate_mod.write_tables(outdir, run.configuration.method, result)
    logger.info("Wrote %d representatives of %d genomes to %s", int((result.representative == np.arange(n)).sum()), n, outdir)
    return written
