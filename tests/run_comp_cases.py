"""Inputs and restatements for plot-run-comp: the definition of the join with Python dictionaries, a numpy mask
restatement, inputs aimed at the group and workgroup edges of ``rc_join_kernel``, values aimed at the bin edges of the
histogram, and the database the end-to-end tests share.

Used by tests/test_run_comp_host.py (no GPU: the host twins and ``rundb.plot_run_comp``) and tests/test_gpu_run_comp.py
(the kernels).  ``T`` restates the kernel's rows per workgroup; when the kernel's changes, change it here, and the sizes
of the cases follow."""

from __future__ import annotations

import sqlite3

import numpy as np

from pyani_plus_amd import run_comp, rundb
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

# csrc/runcomp.hip: kRowsPerWg (kThreads * kGroups); a wave's ballot covers 64 consecutive rows
T = 1024
NONE = 0xFFFFFFFF
JOIN_ROWS = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7, 2**20 + 3)
JOIN_REFS = (1, 3, 257)
JOIN_PATTERNS = ("all", "none", "alternating", "last of 64", "first of T", "mixed")
HIST_BINS = (1, 7, 30)
HIST_SIZES = (1, 2, 63, 64, 65, 2**20 + 3)
HIST_FAMILIES = ("uniform", "adversarial", "equal", "two values", "nan", "outside")


def same_bits(got, want) -> None:
    """Two float64 arrays with the same shape and the same bit patterns, NaN payloads and zero signs included."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---------------------------------------------------------------- the definition
def dict_join(ref_rows, other_rows) -> list[tuple[float, float]]:
    """``[(x, y), ...]``: for each ``(query_hash, subject_hash, identity)`` of ``other_rows``, in their order, with an
    identity that is not None, the reference run's identity of the same ordered pair when it has one that is not None."""
    reference = {(q, s): identity for q, s, identity in ref_rows if identity is not None}
    return [(reference[q, s], identity) for q, s, identity in other_rows if identity is not None and (q, s) in reference]


def as_rows(ref, q, s, y):
    """Array inputs of the join as the two row lists of ``dict_join``: genome i is ``"g<i>"``, ``NONE`` a genome the
    reference run does not have, NaN is None."""
    n = len(ref)
    ref_rows = [(f"g{i}", f"g{j}", None if np.isnan(ref[i, j]) else float(ref[i, j])) for i in range(n) for j in range(n)]
    name = lambda i: f"g{i}" if i != NONE else "other"  # noqa: E731
    other_rows = [(name(int(a)), name(int(b)), None if np.isnan(v) else float(v)) for a, b, v in zip(q, s, y)]
    return ref_rows, other_rows


def numpy_join(ref, q, s, y):
    """The join as numpy masks: ``(x, y, d)``."""
    ref = np.asarray(ref, dtype=np.float64)
    n = len(ref)
    q, s, y = np.asarray(q, dtype=np.uint32), np.asarray(s, dtype=np.uint32), np.asarray(y, dtype=np.float64)
    inside = (q < n) & (s < n) & ~np.isnan(y)
    x = np.full(len(y), np.nan)
    x[inside] = ref.reshape(-1)[q[inside].astype(np.int64) * n + s[inside].astype(np.int64)] if n else np.nan
    keep = inside & ~np.isnan(x)
    return x[keep], y[keep], y[keep] - x[keep]


# ---------------------------------------------------------------- join inputs
def join_reference(n_ref: int, seed: int = 5) -> np.ndarray:
    """An n_ref x n_ref matrix of identities in [0, 1) with a quarter of the cells NaN from three genomes up (cell
    (0, 0) always has a value, cell (0, 1) never); a single genome has its one value."""
    rng = np.random.default_rng(seed + n_ref)
    ref = rng.random((n_ref, n_ref))
    if n_ref >= 3:  # noqa: PLR2004
        ref[rng.random((n_ref, n_ref)) < 0.25] = np.nan  # noqa: PLR2004
        ref[0, 0], ref[0, 1] = 0.5, np.nan
    return ref


def survive_mask(pattern: str, n_rows: int, rng) -> np.ndarray:
    i = np.arange(n_rows)
    if pattern == "all":
        return np.ones(n_rows, dtype=bool)
    if pattern == "none":
        return np.zeros(n_rows, dtype=bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "last of 64":
        return i % 64 == 63  # noqa: PLR2004
    if pattern == "first of T":
        return i % T == 0
    assert pattern == "mixed"
    return rng.random(n_rows) >= 0.4  # noqa: PLR2004


def join_inputs(n_rows: int, ref: np.ndarray, pattern: str, seed: int = 11):
    """``(q, s, y, n_survivors)``: rows of which exactly those of ``survive_mask`` survive.  A row that does not is ruled
    out, with equal shares, by a sentinel q, a sentinel s, a NaN y or a NaN cell of ``ref`` (a matrix without NaN cells
    gives that share to NaN y): in ``mixed`` that is 10 % of all rows each."""
    rng = np.random.default_rng(seed * 1_000_003 + n_rows)
    n_ref = len(ref)
    keep = survive_mask(pattern, n_rows, rng)
    valid, holes = np.argwhere(~np.isnan(ref)), np.argwhere(np.isnan(ref))
    cells = valid[rng.integers(0, len(valid), n_rows)]
    q, s = cells[:, 0].astype(np.uint32), cells[:, 1].astype(np.uint32)
    y = rng.random(n_rows)
    why = rng.integers(0, 4, n_rows)
    out = ~keep
    q[out & (why == 0)] = NONE
    s[out & (why == 1)] = NONE
    y[out & (why == 2)] = np.nan  # noqa: PLR2004
    cell = out & (why == 3)  # noqa: PLR2004
    if len(holes):
        picked = holes[rng.integers(0, len(holes), int(cell.sum()))]
        q[cell], s[cell] = picked[:, 0], picked[:, 1]
    else:
        y[cell] = np.nan
    assert n_ref > 0
    return q, s, y, int(keep.sum())


# ---------------------------------------------------------------- histogram inputs
def adversarial_values(edges) -> np.ndarray:
    """Every edge, its two neighbours among the doubles, the midpoints of the bins, and the first and last edge again."""
    edges = np.asarray(edges, dtype=np.float64)
    return np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), (edges[:-1] + edges[1:]) / 2, edges[:1], edges[-1:]])


def hist_inputs(family: str, n: int, bins: int, seed: int = 3):
    """``(values, edges)`` of one family; the edges are those of ``numpy.histogram(values, bins)`` except for
    ``adversarial`` (the edges its values are made from) and ``outside`` (the narrower range (0, 1) for values in (-1, 2))."""
    rng = np.random.default_rng(seed * 7919 + n * 31 + bins)
    if family == "uniform":
        v = rng.random(n)
    elif family == "adversarial":
        lo, hi = sorted(rng.random(2))
        edges = run_comp.hist_edges(lo, hi, bins)
        return np.resize(adversarial_values(edges), n), edges
    elif family == "equal":
        v = np.full(n, 0.75)
    elif family == "two values":
        v = np.where(np.arange(n) % 2 == 0, 0.25, 0.75)
    elif family == "nan":
        v = rng.random(n)
        v[rng.random(n) < 0.2] = np.nan  # noqa: PLR2004
        if np.isnan(v).all():
            return v, run_comp.hist_edges(0.0, 1.0, bins)
    else:
        assert family == "outside"
        return rng.random(n) * 3 - 1, run_comp.hist_edges(0.0, 1.0, bins)
    return v, run_comp.hist_edges(np.nanmin(v), np.nanmax(v), bins)


def numpy_hist(values, edges) -> np.ndarray:
    values = np.asarray(values, dtype=np.float64)
    return np.histogram(values[~np.isnan(values)], len(edges) - 1, range=(edges[0], edges[-1]))[0].astype(np.uint64)


# ---------------------------------------------------------------- the database of the end-to-end tests
VIRAL = GOLDEN / "viral_example"
OTHER_SCALED = 100


def make_viral_db(tmp):
    """A database with four runs of the viral fixture: 1 sourmash-hip, 2 fastANI-hip, 3 sourmash-hip with another
    ``scaled``, 4 sourmash-hip over a directory with two of the three genomes.  Computed by the oracle, no GPU."""
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp / "runs.sqlite"
    two = tmp / "two_genomes"
    two.mkdir()
    for fasta in sorted(p for p in VIRAL.iterdir() if p.suffix in rundb.FASTA_EXTENSIONS)[:2]:
        (two / fasta.name).write_bytes(fasta.read_bytes())
    assert rundb.run_sourmash_hip(VIRAL, db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp / "t1", name="sourmash run").status == "Done"
    assert rundb.run_fastani_hip(VIRAL, db, engine=OracleEngine(), temp=tmp / "t2", name="fastANI run").status == "Done"
    assert rundb.run_sourmash_hip(VIRAL, db, cache=tmp / "cache", scaled=OTHER_SCALED, engine=OracleEngine(), temp=tmp / "t3", name="other scaled").status == "Done"
    assert rundb.run_sourmash_hip(two, db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp / "t4", name="two genomes").status == "Done"
    return db


def run_rows(database, run_id: int) -> list[tuple[str, str, float | None]]:
    """``(query_hash, subject_hash, identity)`` of a run's comparisons in ``comparison_id`` order, by plain SQL."""
    conn = sqlite3.connect(database)
    try:
        return conn.execute(
            "SELECT c.query_hash, c.subject_hash, c.identity FROM comparisons c, runs r WHERE r.run_id = ? "
            "AND c.configuration_id = r.configuration_id "
            "AND c.query_hash IN (SELECT genome_hash FROM runs_genomes WHERE run_id = r.run_id) "
            "AND c.subject_hash IN (SELECT genome_hash FROM runs_genomes WHERE run_id = r.run_id) ORDER BY c.comparison_id",
            (run_id,),
        ).fetchall()
    finally:
        conn.close()


def expected_table(database, ref_id: int, other_id: int) -> bytes:
    """The table of the two runs from ``dict_join`` and Python's own float formatting."""
    conn = sqlite3.connect(database)
    names = dict(conn.execute("SELECT run_id, name FROM runs"))
    conn.close()
    lines = [f"#{names[ref_id]}\t{names[other_id]}\n"] + [f"{x}\t{y}\n" for x, y in dict_join(run_rows(database, ref_id), run_rows(database, other_id))]
    return "".join(lines).encode()
