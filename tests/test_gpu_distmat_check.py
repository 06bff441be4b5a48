"""The one device check of a distance matrix on the MI355X, through its three callers (``engine.nj_tree``,
``engine.gower_center``, ``engine.mantel``): the reported cell and the count at the seam of two workgroups, the mirrored
cell that comes first, the grid-stride path past 65 536 workgroups, two bad matrices in one call, and the scalar slot the
three share, used by one after the other on one engine.  Every refusal is the host twin's text but for the prefix."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import HipEngine, gower_center_host, mantel_host, nj_tree_host
from tests import mantel_cases as mc
from tests.helpers import distance_check_cases, distance_refusal, invalid_distance_matrices

pytestmark = pytest.mark.gpu

CASES = distance_check_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def refusal(call, *arguments) -> str:
    """The library's message of a call that must be refused."""
    with pytest.raises(HipBackendError) as err:
        call(*arguments)
    assert err.value.status == PA_E_INVALID
    return str(err.value).split(": ", 1)[1]  # behind "<call> failed with status <s>: "


def after_prefix(message: str, prefix: str) -> str:
    assert message.startswith(prefix + ": ")
    return message[len(prefix) + 2 :]


def same_tree(got, want) -> None:
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(got[2], want[2]) and np.array_equal(bits(got[3]), bits(want[3]))


@pytest.mark.parametrize("name,D,cell,count", CASES, ids=IDS)
def test_tree_refusal_names_the_cell_and_the_count(engine, name, D, cell, count):
    got = refusal(engine.nj_tree, D)
    assert got == distance_refusal("pa_nj", "D", cell, count)
    assert after_prefix(got, "pa_nj") == after_prefix(refusal(nj_tree_host, D), "pa_nj_host")


@pytest.mark.parametrize("name,D,cell,count", CASES, ids=IDS)
def test_centring_refusal_names_the_cell_and_the_count(engine, name, D, cell, count):
    got = refusal(engine.gower_center, D)
    assert got == distance_refusal("pa_gower_center", "D", cell, count)
    assert after_prefix(got, "pa_gower_center") == after_prefix(refusal(gower_center_host, D), "pa_gower_center_host")


@pytest.mark.parametrize("name,D,cell,count", CASES, ids=IDS)
def test_mantel_refusal_names_the_matrix_the_cell_and_the_count(engine, name, D, cell, count):
    good = mc.random_distances(len(D), 8)
    perms = mc.permutations(1, len(D), 0, 2)
    for matrix, arguments in (("X", (D, good, perms)), ("Y", (good, D, perms))):
        got = refusal(engine.mantel, *arguments)
        assert got == distance_refusal("pa_mantel", matrix, cell, count)
        assert got == refusal(mantel_host, *arguments)  # the twin's prefix is the same


def test_grid_stride_path_finds_the_last_cell(engine):
    """4100^2 cells are more than 65 536 workgroups of 256: every lane walks more than one cell.  The matrix (134 MB) is
    made on the device."""
    t = engine.torch
    n = 4100
    assert n * n > 65536 * 256
    d = t.zeros((n, n), dtype=t.float64, device=engine.device)
    d[n - 1, n - 1] = 0.5
    got = refusal(engine.gower_center, d)
    assert got == distance_refusal("pa_gower_center", "D", (n - 1, n - 1), 1)
    assert after_prefix(got, "pa_gower_center") == after_prefix(refusal(gower_center_host, d.cpu().numpy()), "pa_gower_center_host")


def test_two_bad_matrices_report_x(engine):
    _, split, cell, count = CASES[0]
    _, second, other_cell, _ = CASES[1]
    assert cell != other_cell
    perms = mc.permutations(1, 17, 0, 2)
    got = refusal(engine.mantel, split, second, perms)
    assert got == distance_refusal("pa_mantel", "X", cell, count) == refusal(mantel_host, split, second, perms)
    got = refusal(engine.mantel, second, split, perms)
    assert got == distance_refusal("pa_mantel", "X", other_cell, count)


def test_the_three_callers_share_the_slot_one_after_the_other(engine):
    """A refusal leaves its words in the slot; the next caller's check starts from its own."""
    bad = {what: (D, cell) for what, D, cell in invalid_distance_matrices(9, 3)}
    good, other = mc.random_distances(9, 8), mc.random_distances(9, 9)
    perms = mc.permutations(1, 9, 0, 3)
    D, cell = bad["negative"]
    assert refusal(engine.nj_tree, D) == distance_refusal("pa_nj", "D", cell, 2)
    got = engine.gower_center(good)
    want = gower_center_host(good)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1:]), bits(want[1:]))
    D, cell = bad["diagonal"]
    assert refusal(engine.gower_center, D) == distance_refusal("pa_gower_center", "D", cell, 1)
    same_tree(engine.nj_tree(good), nj_tree_host(good))
    D, cell = bad["asymmetric"]
    assert refusal(engine.mantel, good, D, perms) == distance_refusal("pa_mantel", "Y", cell, 2)
    got = engine.mantel(good, other, perms)
    want = mantel_host(good, other, perms)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
