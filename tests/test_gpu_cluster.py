"""plot-run's clustering on the MI355X: ``pa_rowdist_euclid`` against ``pa_rowdist_euclid_host`` and against a numpy
restatement, bit for bit; the golden cases through the device distances; ``rundb.plot_run`` after a real run.  Nothing
here reads the reference or needs scipy; no step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import cluster, rundb
from pyani_plus_amd.engine import HipEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.plot_run_cases import case_matrix, distance_inputs, filled, load_cases, matrix_md5, numpy_distances, same_bits

pytestmark = pytest.mark.gpu

# the tile edges (63, 64, 65), a ragged last column chunk and more than one chunk (257 and 130 columns of 16), more tiles
# than one wave of workgroups (1000 rows: 136 tiles of 64 x 64); then the run-time column count at the 256 that the
# correlation kernel fixes at compile time and one below it, exactly one stage, a single column, and one column past a
# stage on the smallest matrix
SHAPES = ((2, 2), (3, 3), (63, 63), (64, 64), (65, 65), (130, 257), (257, 130), (1000, 1000), (65, 256), (65, 255), (70, 16), (70, 1), (2, 17))
CASES = load_cases()
PLOTS = GOLDEN / "viral_example" / "plots"


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_distances_equal_host_and_numpy(engine, shape):
    n, m = shape
    for name, x in distance_inputs(n, m):
        got = engine.row_distances(x)
        assert got.shape == (n * (n - 1) // 2,), name
        same_bits(got, cluster.row_distances(x))
        if n <= 257:
            same_bits(got, numpy_distances(x))
        if name == "duplicated":
            assert got[0] == 0.0 and not np.signbit(got[0])  # rows 0 and 1 are equal: +0.0


def test_row_distances_of_a_device_tensor_and_small_inputs(engine):
    t = engine.torch
    x = np.random.default_rng(5).uniform(-1.0, 1.0, (70, 33))
    d = engine.row_distances_device(t.from_numpy(x).to(engine.device))
    assert d.is_cuda and d.dtype == t.float64
    same_bits(d.cpu().numpy(), cluster.row_distances(x))
    assert engine.row_distances(np.zeros((1, 5))).shape == (0,)
    assert engine.row_distances(np.zeros((0, 5))).shape == (0,)
    same_bits(engine.row_distances(np.zeros((3, 0))), np.zeros(3))
    with pytest.raises(ValueError, match="two dimensions"):
        engine.row_distances(np.zeros(4))
    with pytest.raises(ValueError, match="65537 rows; at most 65536"):  # before 17 GB of output are allocated
        engine.row_distances(np.zeros((65537, 0)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_with_the_device_distances(engine, case):
    assert matrix_md5(case_matrix(case)) == case["md5"], "the generator drifted"
    x = filled(case)
    d = engine.row_distances(x)
    z, leaves = cluster.linkage_average(d, len(x))
    assert leaves.tolist() == case["leaves"]
    assert z.shape == (len(x) - 1, 4) and np.array_equal(cluster.cluster_order(case_matrix(case), case["na_fill"], engine), leaves)


def test_plot_run_after_a_real_run(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp_path / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp_path / "cache", scaled=scaled, engine=engine, temp=tmp_path)
    assert run.status == "Done"
    written = rundb.plot_run(db, tmp_path / "plots", engine=engine)
    assert sorted(p.name for p in written) == sorted(
        [f"sourmash-hip_{s}_heatmap.tsv" for s in ("identity", "query_cov", "hadamard", "tANI")]
        + [f"sourmash-hip_{s}_scatter.tsv" for s in ("query_cov", "tANI")]
    )
    for score in ("identity", "query_cov", "hadamard", "tANI"):
        got = (tmp_path / "plots" / f"sourmash-hip_{score}_heatmap.tsv").read_bytes()
        assert got == (PLOTS / f"sourmash_{score}_heatmap.tsv").read_bytes(), score
    for score in ("query_cov", "tANI"):
        got = (tmp_path / "plots" / f"sourmash-hip_{score}_scatter.tsv").read_text().split("\n")
        assert sorted(got) == sorted((PLOTS / f"sourmash_{score}_scatter.tsv").read_text().split("\n")), score


def test_profile_phase(engine):
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        engine.row_distances(np.random.default_rng(9).uniform(0.0, 1.0, (300, 300)))
        ms, launches = engine.prof_get()["rowdist"]
    finally:
        engine.prof_enable(False)
    assert launches == 1 and ms > 0.0
