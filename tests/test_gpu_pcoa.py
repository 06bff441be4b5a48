"""ordinate-run on the MI355X: ``pa_mul_tall_f64`` and ``pa_gower_center`` against their host twins bit for bit on the
shape grid of tests/pcoa_cases.py, ``pa_symm_top_eigs`` against its twin bit for bit on every solve (values, vectors,
residuals and info), twice on one case, the refusals, and ``rundb.ordinate_run`` with the engine against the host run.
The largest matrix of the product is 513 x 513, the largest of the solver 800 x 800; no step is tried twice."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import rundb
from pyani_plus_amd._capi import PA_E_INVALID, PA_E_NOCONVERGE, HipBackendError
from pyani_plus_amd.engine import HipEngine, gower_center_host, mul_tall_host, symm_top_eigs_host
from tests import pcoa_cases as pc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_solve(got, want) -> None:
    for a, b in zip(got[:3], want[:3]):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    assert got[3][:2] == want[3][:2] and bits(got[3][2]) == bits(want[3][2])


@pytest.mark.parametrize("p", pc.PRODUCT_WIDTHS)
@pytest.mark.parametrize("n", pc.product_sizes())
def test_product_equals_the_twin(engine, n, p):
    A, Q = pc.product_input(n, p)
    got = engine.mul_tall(A, Q)
    assert got.shape == (n, p)
    assert np.array_equal(bits(got), bits(mul_tall_host(A, Q)))
    assert np.array_equal(bits(got), bits(pc.product_restated(n, p)))


def test_product_twice_and_its_tensors_are_left_alone(engine):
    t = engine.torch
    A, Q = pc.product_input(513, 11)
    d_a, d_q = t.from_numpy(np.array(A)).to(engine.device), t.from_numpy(np.array(Q)).to(engine.device)
    first = engine.mul_tall_device(d_a, d_q).cpu().numpy()
    second = engine.mul_tall_device(d_a, d_q).cpu().numpy()
    assert np.array_equal(bits(first), bits(second)) and np.array_equal(bits(first), bits(pc.product_restated(513, 11)))
    assert np.array_equal(bits(d_a.cpu().numpy()), bits(A)) and np.array_equal(bits(d_q.cpu().numpy()), bits(Q))


@pytest.mark.parametrize("n", pc.CENTRING_SIZES)
def test_centring_equals_the_twin(engine, n):
    D = pc.random_distances(n, 300 + n)
    B, trace, fro2 = engine.gower_center(D)
    want = gower_center_host(D)
    assert np.array_equal(bits(B), bits(want[0])) and np.array_equal(bits(B), bits(B.T))
    assert bits(trace) == bits(want[1]) and bits(fro2) == bits(want[2])


@pytest.mark.parametrize("what,D,cell", pc.invalid_matrices(), ids=[w for w, _, _ in pc.invalid_matrices()])
def test_centring_refuses_and_leaves_the_context_usable(engine, what, D, cell):
    with pytest.raises(HipBackendError, match=rf"pa_gower_center: D\[{cell[0]},{cell[1]}\]") as err:
        engine.gower_center(D)
    assert err.value.status == PA_E_INVALID
    good = pc.random_distances(3, 1)
    assert np.array_equal(bits(engine.gower_center(good)[0]), bits(gower_center_host(good)[0]))


@pytest.mark.parametrize("name,k", pc.SOLVES, ids=[f"{n}-k{k}" for n, k in pc.SOLVES])
def test_solver_equals_the_twin(engine, name, k):
    c = pc.case(name)
    got = engine.symm_top_eigs(c.B, k, c.fro2)
    same_solve(got, symm_top_eigs_host(c.B, k, c.fro2))
    scale = pc.spectral_scale(name)
    assert (np.abs(got[0] - pc.eigh_top(name, k)) <= 1e-9 * scale).all() and (got[2] <= pc.TOL * scale).all()


def test_two_solves_give_the_same_bits_and_a_tensor_is_left_alone(engine):
    t = engine.torch
    c = pc.case("ani800")
    b = t.from_numpy(np.array(c.B)).to(engine.device)
    first = engine.symm_top_eigs(b, 3, c.fro2)
    assert np.array_equal(bits(b.cpu().numpy()), bits(c.B)), "the caller's tensor was overwritten"
    same_solve(engine.symm_top_eigs(c.B, 3, c.fro2), first)


def test_solver_refusals_leave_the_context_usable(engine):
    c = pc.case("noise400")
    with pytest.raises(HipBackendError, match=r"pa_symm_top_eigs: no convergence in 3 iterations") as err:
        engine.symm_top_eigs(c.B, 3, c.fro2, max_iter=3)
    assert err.value.status == PA_E_NOCONVERGE
    with pytest.raises(HipBackendError, match="eigenpairs") as err:
        engine.symm_top_eigs(pc.case("random9").B, 10, 1.0)
    assert err.value.status == PA_E_INVALID
    with pytest.raises(HipBackendError, match="33 columns"):
        engine.mul_tall(np.zeros((40, 40)), np.zeros((40, 33)))
    small = pc.case("two")
    same_solve(engine.symm_top_eigs(small.B, 2, small.fro2), symm_top_eigs_host(small.B, 2, small.fro2))


def test_ordinate_run_with_the_engine_writes_the_host_bytes(engine, tmp_path):
    scaled, _genomes = FIXTURE_SETS["bacterial_example"]
    db = tmp_path / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "bacterial_example", db, cache=tmp_path / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp_path)
    assert run.status == "Done"
    host = rundb.ordinate_run(db, tmp_path / "host")
    device = rundb.ordinate_run(db, tmp_path / "device", engine=engine)
    assert [p.name for p in device] == [p.name for p in host] == ["sourmash-hip_identity_pcoa.tsv", "sourmash-hip_identity_pcoa_eigenvalues.tsv"]
    assert [p.read_bytes() for p in device] == [p.read_bytes() for p in host]
