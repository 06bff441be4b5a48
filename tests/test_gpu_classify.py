"""classify on the MI355X: ``pa_classify_edges`` against ``pa_classify_edges_host`` and against a numpy restatement, bit
for bit; the golden cases end to end with the device engine; ``rundb.classify`` after a real run.  Nothing here reads
the reference; no step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import classify as cl
from pyani_plus_amd import rundb
from pyani_plus_amd.engine import HipEngine
from pyani_plus_amd.synth import synth_classify_matrices
from tests.classify_cases import base_matrices, load_cases, matrices_md5
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu

AGGS = ("min", "max", "mean")
SIZES = (1, 2, 63, 64, 65, 1000, 3001)
CASES = load_cases()


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def numpy_edges(score, cov, score_edges, coverage_edges, cov_min):
    """The edge list restated with numpy: pairs in (i, j) order, the reference's aggregation with its argument order
    [M[j,i], M[i,j]], then one lexicographic sort by (score, i, j)."""
    n = len(score)
    i, j = np.triu_indices(n, 1)

    def agg(name, m):
        a, b = m[j, i], m[i, j]
        if name == "min":
            return np.where(b < a, b, a)
        if name == "max":
            return np.where(b > a, b, a)
        return (a + b) / 2.0

    with np.errstate(invalid="ignore"):
        c, s = agg(coverage_edges, cov), agg(score_edges, score)
        keep = ~np.isnan(c) & ~np.isnan(s) & (c > cov_min)
    i, j, s, c = i[keep], j[keep], s[keep], c[keep]
    order = np.lexsort((j, i, s))  # -0.0 and 0.0 compare equal
    return i[order].astype(np.uint32), j[order].astype(np.uint32), s[order], c[order]


def same_bits(got, want) -> None:
    assert len(got) == len(want) == 4
    for g, w, kind in zip(got, want, (np.uint32, np.uint32, np.uint64, np.uint64)):
        assert g.shape == w.shape
        assert np.array_equal(np.ascontiguousarray(g).view(kind), np.ascontiguousarray(w).view(kind))


def check(engine, score, cov, score_edges, coverage_edges, cov_min, *, host=True):
    got = engine.classify_edges(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, cov_min=cov_min)
    same_bits(got, numpy_edges(score, cov, score_edges, coverage_edges, cov_min))
    if host:
        same_bits(got, cl.edges_host(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, cov_min=cov_min))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_edges_equal_host_and_numpy_for_every_aggregator_pair(engine, n):
    _labels, ident, cov = synth_classify_matrices(n, 21, nan_frac=0.05)
    for sa in AGGS:
        for ca in AGGS:
            got = check(engine, ident, cov, sa, ca, 0.5)
            assert n < 60 or 0 < len(got[0]) < n * (n - 1) // 2


@pytest.mark.parametrize("n", SIZES)
def test_edges_with_heavy_ties(engine, n):
    """Identities rounded to two decimals and duplicated genomes: thousands of equal scores, kept in (i, j) order."""
    _labels, ident, cov = synth_classify_matrices(n, 22, nan_frac=0.02, decimals=2)
    if n >= 4:
        ident[: n // 2, : n // 2] = 1.0
    got = check(engine, ident, cov, "mean", "min", 0.5)
    if n >= 1000:  # a mean of two 2-decimal identities takes a few hundred values; there are 10^5 edges and more
        assert len(np.unique(got[2])) < len(got[2]) // 8


@pytest.mark.parametrize("n", SIZES)
def test_edges_in_tani_mode_with_both_zeros(engine, n):
    """tANI mode: every score is <= 0, and -0.0 and 0.0 are the same score but keep their own bits."""
    _labels, ident, cov = synth_classify_matrices(n, 23, nan_frac=0.03)
    score = cl.tani_scores(ident * cov)
    rng = np.random.default_rng(n)
    zero = rng.random((n, n)) < 0.1
    score[zero & ~np.isnan(score)] = 0.0
    score[zero & (rng.random((n, n)) < 0.5) & ~np.isnan(score)] = -0.0
    assert n < 3 or (score[~np.isnan(score)] <= 0).all()
    for sa in ("min", "max"):
        got = check(engine, score, cov, sa, "max", 0.3)
        if n >= 63 and sa == "max":  # a tenth of the cells are zeros, so about a fifth of the maxima of two are
            zeros = got[2][got[2] == 0.0]
            assert len(zeros) > 10 and len(np.unique(np.signbit(zeros))) == 2
            assert (np.diff(got[2]) >= 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_thresholds_that_keep_nothing_and_everything(engine, n):
    _labels, ident, cov = synth_classify_matrices(n, 24)
    assert len(check(engine, ident, cov, "mean", "min", 1.0)[0]) == 0
    assert len(check(engine, ident, cov, "mean", "max", -1.0)[0]) == n * (n - 1) // 2
    nan = np.full((n, n), np.nan)
    assert len(check(engine, nan, cov, "min", "min", 0.0)[0]) == 0


def test_device_tensors_and_argument_checks(engine):
    t = engine.torch
    _labels, ident, cov = synth_classify_matrices(200, 25, nan_frac=0.05)
    d_ident, d_cov = t.from_numpy(ident).to(engine.device), t.from_numpy(cov).to(engine.device)
    same_bits(engine.classify_edges(d_ident, d_cov), cl.edges_host(ident, cov))
    with pytest.raises(ValueError, match="Unknown score aggregator"):
        engine.classify_edges(ident, cov, score_edges="median")
    with pytest.raises(ValueError, match="square"):
        engine.classify_edges(ident, cov[:10])
    # the library's own checks: more genomes than 32-bit edge positions allow, room for too few edges
    import ctypes as C

    count = C.c_uint64(0)
    args = (d_ident.data_ptr(), d_cov.data_ptr())
    assert engine.lib.pa_classify_edges(engine.ctx, *args, 65537, 0, 0, 0.5, 0, None, None, None, None, C.byref(count)) == -1
    assert b"65536" in engine.lib.pa_last_error()
    assert engine.lib.pa_classify_edges(engine.ctx, *args, 200, 2, 0, 0.5, 5, None, None, None, None, C.byref(count)) == -4
    assert count.value == len(cl.edges_host(ident, cov)[0]) > 5


def test_profile_phases(engine):
    _labels, ident, cov = synth_classify_matrices(300, 26)
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        engine.classify_edges(ident, cov)
        prof = engine.prof_get()
    finally:
        engine.prof_enable(False)
    assert prof["cls_edges"][1] == 1 and prof["cls_sort"][1] == 1 and prof["cls_edges"][0] > 0 and prof["cls_sort"][0] > 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_with_the_device_engine(engine, case):
    labels, ident, cov = base_matrices(case["source"])
    assert matrices_md5(ident, cov) == case["md5"]
    score = ident if case["mode"] == "identity" else cl.tani_scores(ident * cov)
    kwargs = {"coverage_edges": case["coverage_edges"], "score_edges": case["score_edges"], "cov_min": case["cov_min"]}
    rows = cl.classify_matrices(labels, score, cov, engine=engine, **kwargs)
    got = {frozenset(r.members): (r.n_nodes, *(None if v is None else repr(float(v)) for v in (r.max_cov, r.min_score, r.max_score))) for r in rows}
    assert got == {frozenset(r["members"]): tuple(r["raw"]) for r in case["rows"]}
    assert rows == cl.classify_matrices(labels, score, cov, engine=None, **kwargs)
    lines = cl.classify_tsv(rows, case["mode"]).split("\n")
    assert lines[0] == case["header"]
    assert sorted((sorted(f[4].split(",")), f[:4]) for f in (line.split("\t") for line in lines[1:-1])) == [(r["members"], r["tsv"]) for r in case["rows"]]


@pytest.mark.parametrize("name", ["viral_example", "bacterial_example"])
def test_rundb_classify_after_a_real_run(engine, name, tmp_path):
    scaled, genomes = FIXTURE_SETS[name]
    db = tmp_path / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / name, db, cache=tmp_path / "cache", scaled=scaled, engine=engine, temp=tmp_path)
    assert run.status == "Done"
    for mode in ("identity", "tANI"):
        on_device = rundb.classify(db, tmp_path / f"device_{mode}", mode=mode, engine=engine)
        on_host = rundb.classify(db, tmp_path / f"host_{mode}", mode=mode)
        assert on_device.name == "sourmash-hip_classify.tsv"
        text = on_device.read_text()
        assert text == on_host.read_text()
        lines = text.split("\n")
        assert lines[0].split("\t")[2] == ("min_identity" if mode == "identity" else "min_-tANI")
        singles = [line.split("\t")[4] for line in lines[1:-1] if line.startswith("1\t")]
        assert sorted(singles) == sorted(rundb.filename_stem(f) for f in genomes.values())
        if mode == "identity":  # the rows of the reference on its own matrices of this fixture set
            case = next(c for c in CASES if c["name"] == f"{name}-sourmash-identity-cov0.5")
            assert sorted(sorted(line.split("\t")[4].split(",")) for line in lines[1:-1]) == [r["members"] for r in case["rows"]]
