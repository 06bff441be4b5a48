"""tree-run on the MI355X: ``pa_nj`` against ``pa_nj_host`` bit for bit on every case of tests/tree_cases.py (children,
lengths and the last edge), twice on one case, its refusals, and ``rundb.tree_run`` with the engine against the host
run.  The largest of those cases is 511 joins of three small launches each.  Then the cases of their own: ties on more
than one scan tile, and 2048 joins whose first two are found past the join kernel's first trip over the candidates.  No
step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import rundb
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import HipEngine, nj_tree_host
from tests import tree_cases as tc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in tc.cases()]


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def same_table(got, want) -> None:
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    assert np.array_equal(got[2], want[2])
    assert np.float64(got[3]).view(np.uint64) == np.float64(want[3]).view(np.uint64)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_twin(engine, name):
    case = tc.case(name)
    n = len(case.D)
    got = engine.nj_tree(case.D)
    same_table(got, nj_tree_host(case.D))
    if case.edges is not None and n >= 2:
        assert tc.joins_bipartitions(n, *got) == case.edges


@pytest.mark.parametrize("name", [c.name for c in tc.tie_cases()])
def test_ties_across_tiles_go_by_node_id(engine, name):
    """Equal scores in different tiles and in slots that swap-remove has shuffled (tests/test_tree_host.py holds the
    condition on the inputs): the per-tile candidates and their reduction must pick the smallest lo, then hi."""
    D = tc.tie_case(name).D
    want = nj_tree_host(D)
    same_table(engine.nj_tree(D), want)
    if name == "copies258x86":  # and as the pipelines call it: on a device tensor, overwritten
        d = engine.torch.from_numpy(np.array(D)).to(engine.device)
        same_table(engine.nj_tree_inplace(d), want)


def test_a_join_found_past_the_first_trip_over_the_candidates(engine):
    """17 x 17 tiles in the first two joins, 289 candidates for the 256 lanes of the join kernel, the winners at 270."""
    far = tc.far_tile_case()
    got = engine.nj_tree(far.D)
    assert tuple(got[0][0]) == far.first[0] and tuple(got[0][1]) == far.first[1]
    same_table(got, tc.far_tile_twin())


def test_two_runs_give_the_same_table_and_a_tensor_is_left_alone(engine):
    t = engine.torch
    D = tc.case("random129").D
    d = t.from_numpy(np.array(D)).to(engine.device)
    first = engine.nj_tree(d)
    assert np.array_equal(d.cpu().numpy().view(np.uint64), D.view(np.uint64)), "the caller's tensor was overwritten"
    same_table(engine.nj_tree(D), first)
    same_table(first, nj_tree_host(D))


@pytest.mark.parametrize("what,D,cell", tc.invalid_matrices(), ids=[w for w, _, _ in tc.invalid_matrices()])
def test_invalid_matrices_are_refused(engine, what, D, cell):
    with pytest.raises(HipBackendError, match=rf"pa_nj: D\[{cell[0]},{cell[1]}\]") as err:
        engine.nj_tree(D)
    assert err.value.status == PA_E_INVALID
    # a refusal leaves the context usable
    same_table(engine.nj_tree(tc.case("random5").D), nj_tree_host(tc.case("random5").D))


def test_no_nodes_and_too_many_are_refused(engine):
    with pytest.raises(HipBackendError, match="0 nodes") as err:
        engine.nj_tree(np.zeros((0, 0)))
    assert err.value.status == PA_E_INVALID
    with pytest.raises(ValueError, match="square"):
        engine.nj_tree(np.zeros((3, 4)))


def test_tree_run_with_the_engine_writes_the_host_bytes(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp_path / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp_path / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp_path)
    assert run.status == "Done"
    host = rundb.tree_run(db, tmp_path / "host")
    device = rundb.tree_run(db, tmp_path / "device", engine=engine)
    assert device.name == host.name == "sourmash-hip_identity_nj.nwk"
    assert device.read_bytes() == host.read_bytes() and device.read_bytes().endswith(b";\n")


def test_profile_phases(engine):
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        engine.nj_tree(tc.case("random5").D)
        prof = engine.prof_get()
    finally:
        engine.prof_enable(False)
    assert [prof[k][1] for k in ("nj_scan", "nj_join", "nj_update")] == [3, 3, 3]
