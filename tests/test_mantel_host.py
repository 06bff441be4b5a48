"""mantel-run-comp without a GPU: ``pa_mantel_host`` against the restatement of tests/mantel_cases.py bit for bit, the
thread count, the permutations of a seed (the pin, the windows, uniformity), answers that are known exactly, the
refusals with their messages, and the binding's constants against the header."""

from __future__ import annotations

import itertools
import logging
import re
from pathlib import Path

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd import mantel as mantel_mod
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import mantel_host, mantel_permutations
from tests import mantel_cases as mc
from tests.helpers import distance_check_cases, distance_refusal
from tests.mantel_cases import bits

HEADER = Path(__file__).resolve().parent.parent / "include" / "pyani_hip.h"


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("n", mc.SIZES)
def test_twin_equals_the_restatement(n):
    X, Y, perms, stats, sums = mc.case(n)
    assert len(perms) == mc.GENERATED + 2 and perms[-1][0] == n - 1 and perms[-2][0] == n - 1 and perms[-2][-1] == 0
    got_stats, got_sums = mantel_host(X, Y, perms)
    assert np.array_equal(bits(got_stats), bits(stats))
    assert np.array_equal(bits(got_sums), bits(sums))


@pytest.mark.parametrize("n", (65, 513))
def test_thread_count_and_batch_do_not_show(n):
    X, Y, perms, stats, sums = mc.case(n)
    for threads in (1, 3, 16):
        got_stats, got_sums = mantel_host(X, Y, perms, threads=threads)
        assert np.array_equal(bits(got_stats), bits(stats)) and np.array_equal(bits(got_sums), bits(sums))
    # fewer permutations in a call, and none
    got_stats, got_sums = mantel_host(X, Y, perms[5:8])
    assert np.array_equal(bits(got_stats), bits(stats)) and np.array_equal(bits(got_sums), bits(sums[[0, 6, 7, 8]]))
    got_stats, got_sums = mantel_host(X, Y, np.empty((0, n), dtype=np.uint32))
    assert np.array_equal(bits(got_stats), bits(stats)) and np.array_equal(bits(got_sums), bits(sums[:1]))


def test_more_permutations_than_a_host_batch():
    X, Y, _perms, _stats, sums = mc.case(65)
    perms = mc.permutations(3, 65, 0, 150)
    got = mantel_host(X, Y, perms)[1]
    _mean_x, _ss_x, x = mc.moments(X)
    _mean_y, _ss_y, y = mc.moments(Y)
    assert bits(got[0]) == bits(sums[0])
    assert np.array_equal(bits(got[1:]), bits([mc.cross(x, y, pi) for pi in perms]))


def test_inputs_are_left_alone():
    X, Y, perms, _stats, _sums = mc.case(130)
    copies = [np.array(a) for a in (X, Y, perms)]
    mantel_host(*copies)
    assert all(np.array_equal(a, b) for a, b in zip(copies, (X, Y, perms)))


# ------------------------------------------------------------------ the permutations of a seed
def test_generator_pin():
    assert mantel_permutations(1, 5, 0, 3).tolist() == [[2, 1, 3, 4, 0], [0, 1, 2, 4, 3], [0, 1, 4, 3, 2]]
    assert mc.permutations(1, 5, 0, 3).tolist() == [[2, 1, 3, 4, 0], [0, 1, 2, 4, 3], [0, 1, 4, 3, 2]]


@pytest.mark.parametrize("seed", (0, 1, 12345, (1 << 64) - 1))
def test_generator_equals_the_restatement(seed):
    for n in (1, 2, 3, 64, 130):
        assert np.array_equal(mantel_permutations(seed, n, 0, 40), mc.permutations(seed, n, 0, 40))
    assert np.array_equal(mantel_permutations(seed, 7, (1 << 40) + 5, 9), mc.permutations(seed, 7, (1 << 40) + 5, 9))


def test_generator_rows_do_not_depend_on_the_window():
    whole = mantel_permutations(9, 33, 0, 100)
    assert np.array_equal(mantel_permutations(9, 33, 37, 20), whole[37:57])
    assert np.array_equal(np.vstack([mantel_permutations(9, 33, q, 1) for q in range(90, 100)]), whole[90:])
    assert mantel_permutations(9, 33, 5, 0).shape == (0, 33)


def test_generator_seeds_differ_and_rows_are_permutations():
    a, b = mantel_permutations(1, 50, 0, 200), mantel_permutations(2, 50, 0, 200)
    assert not (a == b).all(axis=1).any()
    for rows in (a, b, mantel_permutations((1 << 64) - 1, 1000, 0, 5)):
        assert (np.sort(rows, axis=1) == np.arange(rows.shape[1])).all()


@pytest.mark.parametrize("seed", (0, 1, (1 << 64) - 1, 12345))
def test_generator_is_uniform_over_the_arrangements_of_four(seed):
    """24 000 rows over 24 arrangements: 1 000 expected each, standard deviation 31; the cap of 150 is 4.8 of them."""
    rows = mantel_permutations(seed, 4, 0, 24000)
    codes = rows.astype(np.int64) @ np.array([64, 16, 4, 1])
    arrangements, counts = np.unique(codes, return_counts=True)
    assert len(arrangements) == 24 == len(list(itertools.permutations(range(4))))
    print("arrangement counts", counts.min(), counts.max())
    assert (np.abs(counts - 1000) <= 150).all()


def test_generator_is_uniform_over_positions_and_values():
    """20 000 rows of n = 100: every (position, value) is expected 200 times, standard deviation 14; the cap of 80 is 5.7
    of them over 10 000 counts."""
    rows = mantel_permutations(7, 100, 0, 20000)
    counts = np.zeros((100, 100), dtype=np.int64)
    np.add.at(counts, (np.broadcast_to(np.arange(100), rows.shape), rows), 1)
    print("position-value counts", counts.min(), counts.max())
    assert (np.abs(counts - 200) <= 80).all()
    assert len(np.unique(rows, axis=0)) == len(rows)
    assert not (rows == np.arange(100)).all(axis=1).any()


# ------------------------------------------------------------------ known answers
def test_a_relabelled_copy_is_found_exactly():
    n = 130
    X = mc.dyadic_distances(n, 11)
    sigma = mc.permutations(5, n, 0, 1)[0].astype(np.intp)
    Y = np.ascontiguousarray(X[sigma][:, sigma])
    inverse = np.empty(n, dtype=np.uint32)
    inverse[sigma] = np.arange(n)
    stats, sums = mantel_host(X, Y, inverse[None, :])
    own = mantel_host(X, X, np.empty((0, n), dtype=np.uint32))
    assert bits(stats[0]) == bits(stats[1])  # the means; ss_y may differ from ss_x in the last bits: not asserted
    assert bits(sums[1]) == bits(stats[2]) == bits(own[1][0]) == bits(own[0][2])
    assert sums[0] < sums[1]


@pytest.mark.parametrize("n", mc.SIZES)
def test_observed_r_is_the_correlation_of_the_triangles(n):
    X, Y, _perms, _stats, _sums = mc.case(n)
    test = mantel_mod.mantel_test(X, Y, 0, 0)
    upper = np.triu_indices(n, 1)
    assert abs(test.r - np.corrcoef(X[upper], Y[upper])[0, 1]) <= 1e-10
    assert test.p == 1.0 and test.at_least == 0 and test.null_r.shape == (0,)


def test_ties_with_the_observed_value_count():
    X, Y, _perms, _stats, _sums = mc.case(3)
    test = mantel_mod.mantel_test(X, Y, 60, 4)
    perms = mc.permutations(4, 3, 0, 60)
    stats, sums = mc.restated(X, Y, perms)
    identity_rows = int((perms == np.arange(3)).all(axis=1).sum())
    ties, above = int((sums[1:] == sums[0]).sum()), int((sums[1:] > sums[0]).sum())
    assert identity_rows >= 1 and ties >= identity_rows
    assert test.at_least == ties + above
    assert test.p == (ties + above + 1) / 61
    scale = float(np.sqrt(stats[2] * stats[3]))
    assert np.array_equal(bits(test.null_r), bits(sums[1:] / scale)) and bits(test.r) == bits(sums[0] / scale)


def test_a_constant_matrix_has_no_correlation(caplog):
    caplog.set_level(logging.WARNING)
    X = mc.random_distances(12, 3)
    constant = np.full((12, 12), 0.25)
    np.fill_diagonal(constant, 0.0)
    for pair in ((X, constant), (constant, X)):
        test = mantel_mod.mantel_test(*pair, 10, 0)
        assert test.r is None and test.p is None and test.null_r is None and test.at_least is None
    assert "no correlation is defined" in caplog.text


def test_slices_do_not_show(monkeypatch):
    X, Y, _perms, _stats, _sums = mc.case(64)
    whole = mantel_mod.mantel_test(X, Y, 50, 2)
    monkeypatch.setattr(mantel_mod, "SLICE_BYTES", 7 * 4 * 64)  # seven permutations a slice
    sliced = mantel_mod.mantel_test(X, Y, 50, 2)
    assert np.array_equal(bits(sliced.null_r), bits(whole.null_r)) and sliced[:7] == whole[:7]


# ------------------------------------------------------------------ refusals
def refused(match: str, *arguments) -> None:
    with pytest.raises(HipBackendError, match=match) as err:
        mantel_host(*arguments)
    assert err.value.status == PA_E_INVALID


def test_refuses_two_genomes():
    refused(r"pa_mantel: 2 genomes; 3 to 16384", mc.random_distances(2, 1), mc.random_distances(2, 2), np.array([[1, 0]], dtype=np.uint32))


def test_refuses_too_many_genomes_before_anything_is_read():
    n = _capi.PA_MANTEL_MAX_N + 1
    zeros = np.zeros((n, n))  # never touched: its pages are not even allocated
    refused(rf"pa_mantel: {n} genomes; 3 to 16384", zeros, zeros, np.zeros((1, n), dtype=np.uint32))


def test_refuses_rows_that_are_no_permutations():
    X, Y, perms, _stats, _sums = mc.case(65)
    rows = np.array(perms[:4])
    rows[2, 40] = rows[2, 13]
    refused(rf"pa_mantel: row 2 of the permutations holds {rows[2, 13]} at position 40: repeated from position 13", X, Y, rows)
    rows = np.array(perms[:4])
    rows[3, 9] = 65
    refused(r"pa_mantel: row 3 of the permutations holds 65 at position 9: out of range for 65 genomes", X, Y, rows)


@pytest.mark.parametrize("what,D,cell", mc.invalid_matrices(), ids=[w for w, _, _ in mc.invalid_matrices()])
def test_refuses_matrices_that_break_the_rule(what, D, cell):
    good = mc.random_distances(len(D), 8)
    perms = mc.permutations(1, len(D), 0, 2)
    refused(rf"pa_mantel: X\[{cell[0]},{cell[1]}\] is not finite, is negative", D, good, perms)
    refused(rf"pa_mantel: Y\[{cell[0]},{cell[1]}\] is not finite, is negative", good, D, perms)


@pytest.mark.parametrize("name,D,cell,count", distance_check_cases(), ids=[c[0] for c in distance_check_cases()])
def test_a_refusal_names_the_first_cell_and_counts_them_all(name, D, cell, count):
    good = mc.random_distances(len(D), 8)
    perms = mc.permutations(1, len(D), 0, 2)
    for matrix, arguments in (("X", (D, good, perms)), ("Y", (good, D, perms))):
        with pytest.raises(HipBackendError) as err:
            mantel_host(*arguments)
        assert err.value.status == PA_E_INVALID and str(err.value).endswith(distance_refusal("pa_mantel", matrix, cell, count))


def test_two_bad_matrices_name_x_and_bad_rows_come_first():
    bad = mc.invalid_matrices()
    perms = mc.permutations(1, 9, 0, 2)
    refused(r"pa_mantel: X\[2,5\]", bad[0][1], bad[1][1], perms)
    refused(r"pa_mantel: X\[1,3\]", bad[1][1], bad[0][1], perms)
    rows = np.array(perms)
    rows[0, 0] = 9
    refused(r"pa_mantel: row 0 of the permutations holds 9 at position 0", bad[0][1], bad[1][1], rows)


def test_python_side_shapes():
    X = mc.random_distances(5, 1)
    with pytest.raises(ValueError, match="expected the same"):
        mantel_host(X, mc.random_distances(6, 1), np.empty((0, 5), dtype=np.uint32))
    with pytest.raises(ValueError, match=r"expected \(P, 5\)"):
        mantel_host(X, X, np.zeros((2, 4), dtype=np.uint32))
    with pytest.raises(ValueError, match="seed"):
        mantel_permutations(1 << 64, 5, 0, 1)


# ------------------------------------------------------------------ the binding
def test_binding_matches_the_header():
    text = HEADER.read_text()
    # the binding reads the header, so each value is pinned here, against both
    for name, pinned in (("PA_MANTEL_MAX_N", 16384), ("PA_MANTEL_LANES", 64), ("PA_MANTEL_BATCH", 256), ("PA_ABI_VERSION", 5)):
        value = int(re.search(rf"^#define {name} (\d+)", text, re.MULTILINE).group(1))
        assert value == pinned == getattr(_capi, name.removeprefix("PA_") if name == "PA_ABI_VERSION" else name), name
    assert _capi.ABI_VERSION == 5 and _capi.load_library().pa_abi_version() == 5
    assert _capi.PA_MANTEL_LANES == mc.LANES
    for symbol in ("pa_mantel", "pa_mantel_host", "pa_mantel_permutations"):
        assert symbol in _capi.SIGNATURES and re.search(rf"PA_API int {symbol}\(", text)
