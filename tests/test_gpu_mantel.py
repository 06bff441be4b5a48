"""mantel-run-comp on the MI355X: ``pa_mantel`` against its host twin and the restatement of tests/mantel_cases.py bit for
bit on the size grid, across the seam of a device batch, at the sizes that take the long-row launch (4 097) and an LDS
row past 64 KiB (8 200), twice on the same tensors, the refusals with the twin's messages, and ``rundb.mantel_run_comp``
with the engine against the host run.  No step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import _capi, rundb
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import HipEngine, mantel_host, mantel_permutations
from tests import mantel_cases as mc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.mantel_cases import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def same(got, want) -> None:
    assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0]))
    assert got[1].shape == want[1].shape and np.array_equal(bits(got[1]), bits(want[1]))


def small_good_call(engine) -> None:
    X, Y, perms, stats, sums = mc.case(4)
    same(engine.mantel(X, Y, perms), (stats, sums))


@pytest.mark.parametrize("n", mc.SIZES)
def test_device_equals_the_twin_and_the_restatement(engine, n):
    X, Y, perms, stats, sums = mc.case(n)
    got = engine.mantel(X, Y, perms)
    same(got, mantel_host(X, Y, perms))
    same(got, (stats, sums))


@pytest.mark.parametrize("extra", (-1, 0, 1))
def test_the_seam_of_a_batch(engine, extra):
    X, Y, _perms, stats, _sums = mc.case(65)
    count = _capi.PA_MANTEL_BATCH + extra
    perms = mantel_permutations(21, 65, 0, count)
    got = engine.mantel(X, Y, perms)
    same(got, mantel_host(X, Y, perms))
    _mean_x, _ss_x, x = mc.moments(X)
    _mean_y, _ss_y, y = mc.moments(Y)
    assert np.array_equal(bits(got[0]), bits(stats))
    assert np.array_equal(bits(got[1][-4:]), bits([mc.cross(x, y, pi) for pi in perms[-4:]]))


@pytest.mark.parametrize("n,count", ((4097, 2), (8200, 1)))
def test_long_rows(engine, n, count):
    X, Y = mc.related_pair(n, n)
    perms = mantel_permutations(n, n, 0, count)
    same(engine.mantel(X, Y, perms), mantel_host(X, Y, perms))


def test_no_permutations(engine):
    X, Y, _perms, stats, sums = mc.case(129)
    same(engine.mantel(X, Y, np.empty((0, 129), dtype=np.uint32)), (stats, sums[:1]))


def test_two_calls_on_the_same_tensors(engine):
    t = engine.torch
    X, Y, perms, stats, sums = mc.case(513)
    d_x, d_y = t.from_numpy(np.array(X)).to(engine.device), t.from_numpy(np.array(Y)).to(engine.device)
    first = engine.mantel(d_x, d_y, perms)
    second = engine.mantel(d_x, d_y, perms)
    same(first, second)
    same(first, (stats, sums))
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(X)) and np.array_equal(bits(d_y.cpu().numpy()), bits(Y))


def refused(engine, match: str, *arguments) -> None:
    with pytest.raises(HipBackendError, match=match) as err:
        engine.mantel(*arguments)
    assert err.value.status == PA_E_INVALID
    with pytest.raises(HipBackendError, match=match):  # the twin says the same
        mantel_host(*arguments)
    small_good_call(engine)


def test_refuses_two_genomes(engine):
    refused(engine, r"pa_mantel: 2 genomes; 3 to 16384", mc.random_distances(2, 1), mc.random_distances(2, 2), np.array([[1, 0]], dtype=np.uint32))


def test_refuses_rows_that_are_no_permutations(engine):
    X, Y, perms, _stats, _sums = mc.case(65)
    rows = np.array(perms[:4])
    rows[2, 40] = rows[2, 13]
    refused(engine, rf"pa_mantel: row 2 of the permutations holds {rows[2, 13]} at position 40: repeated from position 13", X, Y, rows)
    rows = np.array(perms[:4])
    rows[3, 9] = 65
    refused(engine, r"pa_mantel: row 3 of the permutations holds 65 at position 9: out of range for 65 genomes", X, Y, rows)


@pytest.mark.parametrize("what,D,cell", mc.invalid_matrices(), ids=[w for w, _, _ in mc.invalid_matrices()])
def test_refuses_matrices_that_break_the_rule(engine, what, D, cell):
    good = mc.random_distances(len(D), 8)
    perms = mc.permutations(1, len(D), 0, 2)
    refused(engine, rf"pa_mantel: X\[{cell[0]},{cell[1]}\] is not finite, is negative", D, good, perms)
    refused(engine, rf"pa_mantel: Y\[{cell[0]},{cell[1]}\] is not finite, is negative", good, D, perms)


def test_two_bad_matrices_name_x(engine):
    bad = mc.invalid_matrices()
    refused(engine, r"pa_mantel: X\[2,5\]", bad[0][1], bad[1][1], mc.permutations(1, 9, 0, 2))


def test_mantel_run_comp_with_the_engine_writes_the_host_bytes(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["bacterial_example"]
    db = tmp_path / "runs.sqlite"
    for value in (scaled, 2 * scaled):
        run = rundb.run_sourmash_hip(GOLDEN / "bacterial_example", db, cache=tmp_path / "cache", scaled=value, engine=OracleEngine(), temp=tmp_path)
        assert run.status == "Done"
    host = rundb.mantel_run_comp(db, tmp_path / "host", "1,2", permutations=300, seed=5)
    device = rundb.mantel_run_comp(db, tmp_path / "device", "1,2", permutations=300, seed=5, engine=engine)
    assert [p.name for p in device] == [p.name for p in host] == ["sourmash-hip_identity_1_mantel.tsv", "sourmash-hip_identity_1_vs_2_mantel_null.tsv"]
    assert [p.read_bytes() for p in device] == [p.read_bytes() for p in host]
    assert len(host[1].read_text().splitlines()) == 301
