"""bootstrap-run without a GPU: the weights, the host twins of the weighted counts and of the distances, and
``pa_tree_support``, each against the restatement of ``tests/bootstrap_cases.py``; then the refusals.

A weight above 255 cannot be drawn by any seed one could find (256 of L >= 256 draws on one column), so the refusal of
``pa_msa_boot_weights`` is met through the tools build, whose ``PA_BOOT_WEIGHT_LIMIT`` lowers the limit."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd import engine as engine_mod
from pyani_plus_amd import tree as tree_mod
from tests import bootstrap_cases as cases
from tests import tree_cases
from tests.msa_checker import counts_matrix


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize(("seed", "n_cols"), [(0, 97), (3, 1), ((1 << 64) - 1, 300)])
def test_weights_equal_the_restatement(seed, n_cols):
    got = engine_mod.msa_boot_weights(seed, n_cols, 0, 6)
    assert got.dtype == np.uint8 and got.shape == (6, n_cols)
    np.testing.assert_array_equal(got, cases.weights(seed, n_cols, 0, 6))
    assert (got.sum(axis=1, dtype=np.int64) == n_cols).all()


def test_first_and_count_slice_one_stream():
    whole = engine_mod.msa_boot_weights(5, 64, 0, 10)
    np.testing.assert_array_equal(engine_mod.msa_boot_weights(5, 64, 3, 4), whole[3:7])
    np.testing.assert_array_equal(engine_mod.msa_boot_weights(5, 64, 9, 1), whole[9:])
    assert engine_mod.msa_boot_weights(5, 64, 2, 0).shape == (0, 64)
    assert not np.array_equal(whole[0], whole[1]) and not np.array_equal(whole, engine_mod.msa_boot_weights(6, 64, 0, 10))


def test_small_alignments_reach_three_weight_planes():
    for _n, n_cols, _seed in cases.SUPPORT_ALIGNMENTS:
        assert 4 <= int(engine_mod.msa_boot_weights(0, n_cols, 0, cases.SUPPORT_REPLICATES).max()) <= 7


# ------------------------------------------------------------------ counts and distances
def test_the_count_cases_have_every_plane_count():
    """One case per ``bits`` (ACGT, the alphabet of every other case, is 3): the twin below and the device run them all."""
    for bits in (1, 2, 4, 5, 6, 7, 8):
        hist = np.bincount(cases.count_case(f"bits{bits}").rows.ravel(), minlength=256)
        assert engine_mod.msa_code_table(hist)[1] == bits
    assert engine_mod.msa_code_table(np.bincount(cases.count_case("rows65").rows.ravel(), minlength=256))[1] == 3


@pytest.mark.parametrize("name", [c.name for c in cases.count_cases()])
def test_host_counts_equal_the_restatement(name):
    case = cases.count_case(name)
    match, both = engine_mod.msa_boot_counts_host(case.rows, case.rows.shape[1], case.weights)
    want_m, want_b = cases.restated_counts(name)
    np.testing.assert_array_equal(match, want_m)
    np.testing.assert_array_equal(both, want_b)


def test_host_counts_do_not_depend_on_the_threads_or_the_stride():
    case = cases.count_case("rows65")
    one = engine_mod.msa_boot_counts_host(case.rows, 70, case.weights, threads=1)
    padded = np.full((65, 96), ord("A"), dtype=np.uint8)  # bytes past the columns are not read as columns
    padded[:, :70] = case.rows
    for got in (engine_mod.msa_boot_counts_host(case.rows, 70, case.weights, threads=7), engine_mod.msa_boot_counts_host(padded, 70, case.weights)):
        np.testing.assert_array_equal(got[0], one[0])
        np.testing.assert_array_equal(got[1], one[1])


def test_unit_weights_give_the_pair_counts_meaning():
    rows = cases.alignment(9, 130, 21)
    match, both = engine_mod.msa_boot_counts_host(rows, 130, np.ones((1, 130), dtype=np.uint8))
    want_m, want_b = counts_matrix(rows)  # the checker of pa_msa_pair_counts
    np.testing.assert_array_equal(match[0], want_m)
    np.testing.assert_array_equal(both[0], want_b)


def run_identities(rows: np.ndarray) -> np.ndarray:
    """The identity matrix an external-alignment-hip run of these rows records: ``pa_msa_metrics`` of the pair counts, 1.0
    on the diagonal."""
    m, b = counts_matrix(rows)
    n = (rows != cases.GAP).sum(axis=1).astype(np.uint64)
    identity = engine_mod.msa_metrics(m, b, n[:, None], n[None, :])[0].reshape(m.shape)
    np.fill_diagonal(identity, 1.0)
    return identity


def test_unit_weight_distances_are_the_runs_distances_bit_for_bit():
    rows = cases.alignment(9, 130, 22)
    match, both = engine_mod.msa_boot_counts_host(rows, 130, np.ones((1, 130), dtype=np.uint8))
    D = engine_mod.msa_boot_distances_host(match, both)[0]
    want = tree_mod.run_distances(run_identities(rows))
    np.testing.assert_array_equal(D.view(np.uint64), want.view(np.uint64))
    assert (D > 0).sum() > 50  # not a matrix of zeros
    got, ref = engine_mod.nj_tree_host(D), engine_mod.nj_tree_host(want)
    for a, b in zip(got[:3], ref[:3]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["all_gap", "weights_max255", "rows65"])
def test_host_distances_equal_the_restatement(name):
    match, both = cases.restated_counts(name)
    D = engine_mod.msa_boot_distances_host(match, both, 0.75)
    for r in range(len(match)):
        want = cases.distances(match[r], both[r], 0.75)
        np.testing.assert_array_equal(D[r].view(np.uint64), want.view(np.uint64))
    if name == "all_gap":
        assert D[0, 1, 4] == 0.75 and D[0, 4, 1] == 0.75 and D[0, 1, 1] == 0.0  # no aligned column: `missing`


def test_the_strided_counts_reach_the_second_trip():
    """The conditions on the hand-built counts of ``tests/test_gpu_bootstrap.py``, from the constants of the sources, and
    the twin against the restatement on the matrices with rows without a residue."""
    counts, trip = cases.strided_counts(), cases.stride_cells()
    reps, n, _ = counts.match.shape
    assert (reps, n) == (cases.STRIDED_REPLICATES, cases.STRIDED_ROWS) == (5, 230)
    assert (reps - 1) * n * n < trip < reps * n * n < 2 * trip  # one launch, whose lanes loop once
    a, b = counts.all_gap[reps - 1]
    assert min((reps - 1) * n * n + i * n + j for i, j in ((a, b), (b, a), (a, 0), (b, 0))) >= trip  # both rows, whole
    assert max(1 * n * n + i * n + j for i, j in ((3, 7), (7, 3))) < trip and counts.all_gap[1] == (3, 7)
    residues = counts.both.diagonal(axis1=1, axis2=2).astype(np.int64)
    assert (counts.both <= np.minimum(residues[:, :, None], residues[:, None, :])).all() and (counts.match <= counts.both).all()
    np.testing.assert_array_equal(counts.match, counts.match.transpose(0, 2, 1))
    np.testing.assert_array_equal(counts.both, counts.both.transpose(0, 2, 1))
    assert sorted(np.argwhere(residues == 0).tolist()) == [[1, 3], [1, 7], [reps - 1, a], [reps - 1, b]]
    D = engine_mod.msa_boot_distances_host(counts.match, counts.both, 0.75)
    assert np.argwhere(D == 0.75).tolist() == [[1, 3, 7], [1, 7, 3], [reps - 1, a, b], [reps - 1, b, a]]
    for r in (1, reps - 1):
        np.testing.assert_array_equal(D[r].view(np.uint64), cases.distances(counts.match[r], counts.both[r], 0.75).view(np.uint64))


def test_the_tied_alignment_ties_on_more_than_one_tile():
    """The condition of ``tests/test_tree_host.py`` on the matrices the device pipeline test joins: of the joins made
    while more than kTile nodes are live, at least a third are tied.  Counted here: 23 or 24 of 52 in each."""
    rows = cases.tied_alignment()
    n, n_cols = rows.shape
    k_tile = tree_cases.kernel_constants()["kTile"]
    assert n == 180 > k_tile
    w = np.concatenate([np.ones((1, n_cols), dtype=np.uint8), engine_mod.msa_boot_weights(0, n_cols, 0, 3)])
    D = engine_mod.msa_boot_distances_host(*engine_mod.msa_boot_counts_host(rows, n_cols, w))
    for what, d in zip(("unweighted", "replicate 0", "replicate 1", "replicate 2"), D):
        tied, joins = tree_cases.tied_share(tree_cases.tied_pairs_per_join(d), n)
        print(f"identity, {what}: {tied} of {joins} joins on more than one tile are tied")
        assert joins == n - k_tile and 3 * tied >= joins, what


# ------------------------------------------------------------------ support
def _tables(trees) -> np.ndarray:
    return np.stack([np.asarray(t.child, dtype=np.uint32) for t in trees])


@pytest.mark.parametrize(("n", "n_cols", "seed"), cases.SUPPORT_ALIGNMENTS)
def test_support_equals_the_count_of_equal_sets(n, n_cols, seed):
    r = cases.restated(n, n_cols, seed)
    got = engine_mod.tree_support(n, r.reference.child, _tables(r.trees))
    assert got.tolist() == r.support
    labelled = r.support[:-1]  # the last node made stands for the last edge: another node's edge, or a leaf's
    assert min(labelled) < cases.SUPPORT_REPLICATES and max(labelled) > min(labelled)  # intermediate supports
    assert len({c for c in cases.node_clades(n, r.reference.child) if not cases.is_trivial(c, n)}) == n - 3


@pytest.mark.parametrize(("n", "n_cols", "seed"), cases.SUPPORT_ALIGNMENTS)
def test_host_pipeline_makes_the_restatements_trees(n, n_cols, seed):
    from pyani_plus_amd import bootstrap as bootstrap_mod

    r = cases.restated(n, n_cols, seed)
    trees = bootstrap_mod.replicate_trees(r.rows, n_cols, cases.SUPPORT_REPLICATES, 0)
    for got, want in zip(trees, r.trees):
        np.testing.assert_array_equal(got.child, want.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), want.length.view(np.uint64))
        assert got.last == want.last and got.last_len == want.last_len


def caterpillar(n: int) -> np.ndarray:
    """((((0, 1), 2), 3), ...): join t takes the node made before it and leaf t + 2; leaves n - 1 and the last node remain."""
    return np.array([[0, 1]] + [[t + 1, n + t - 1] for t in range(1, n - 2)], dtype=np.uint32)


def balanced(n: int) -> np.ndarray:
    """Neighbours joined round by round."""
    live, child = list(range(n)), []
    while len(live) > 2:
        a, b = live.pop(0), live.pop(0)
        child.append([min(a, b), max(a, b)])
        live.append(n + len(child) - 1)
    return np.array(child, dtype=np.uint32)


@pytest.mark.parametrize("make", [caterpillar, balanced])
@pytest.mark.parametrize("n", [4, 5, 16, 33])
def test_a_tree_against_itself_has_full_support(make, n):
    table = make(n)
    assert table.shape == (n - 2, 2)
    got = engine_mod.tree_support(n, table, np.stack([table] * 7))
    assert got.tolist() == [7] * (n - 2)
    sets = [{c for c in cases.node_clades(n, table) if not cases.is_trivial(c, n)}] * 7
    assert cases.support(n, table, sets) == [7] * (n - 2)


def test_one_nearest_neighbour_interchange_drops_one_count():
    n = 8
    ref = caterpillar(n)  # join 2 makes node 10 = (9, 3) with 9 = (8, 2): the clades {0,1}, {0,1,2}, {0,1,2,3}, ... as complements
    other = ref.copy()
    other[1], other[2] = (3, 8), (2, 9)  # leaves 2 and 3 change places across the edge above node 9
    reps = np.stack([ref, other, ref])
    got = engine_mod.tree_support(n, ref, reps)
    sets = [{c for c in cases.node_clades(n, t) if not cases.is_trivial(c, n)} for t in reps]
    assert got.tolist() == cases.support(n, ref, sets)
    assert sorted(got.tolist()) == [2] + [3] * (n - 3) and got[1] == 2  # the edge above node 9 alone


def test_support_of_four_leaves():
    ref = np.array([[0, 1], [2, 3]], dtype=np.uint32)  # 01 | 23
    reps = np.array([[[0, 1], [2, 3]], [[2, 3], [0, 1]], [[0, 2], [1, 3]], [[1, 2], [0, 3]], [[0, 1], [2, 4]]], dtype=np.uint32)
    # the last: ((0, 1), 2) and 3 -- the same split 01 | 23
    assert engine_mod.tree_support(4, ref, reps).tolist() == [3, 3]
    assert engine_mod.tree_support(4, ref, reps[:0]).tolist() == [0, 0]


def test_support_does_not_depend_on_the_numbering_of_the_joins():
    r = cases.restated(*cases.SUPPORT_ALIGNMENTS[1])
    n = 12
    D = tree_cases.random_additive_tree(n, 3).D
    other = tree_cases.neighbour_joining(D[::-1, ::-1][np.ix_(range(n), range(n))])  # some other tree over the same leaves
    got = engine_mod.tree_support(n, other.child, _tables(r.trees))
    assert got.tolist() == cases.support(n, other.child, [cases.clades(n, t) for t in r.trees])


# ------------------------------------------------------------------ refusals
def _status(fn, *args) -> tuple[int, str]:
    lib = _capi.load_library()
    status = getattr(lib, fn)(*args)
    return status, _capi.last_error(lib)


def test_refusals_of_the_counts_and_distances():
    rows = np.ascontiguousarray(cases.alignment(4, 40, 1))
    w = np.ones((2, 40), dtype=np.uint8)
    m, b = np.zeros((2, 4, 4), dtype=np.uint32), np.zeros((2, 4, 4), dtype=np.uint32)
    d = np.zeros((2, 4, 4))
    assert _status("pa_msa_boot_counts_host", None, 40, 4, 40, w.ctypes.data, 2, m.ctypes.data, b.ctypes.data, 0) == (
        _capi.PA_E_INVALID, "pa_msa_boot_counts_host: null argument")
    assert _status("pa_msa_boot_counts_host", rows.ctypes.data, 40, 4, 40, w.ctypes.data, 2, None, b.ctypes.data, 0)[0] == _capi.PA_E_INVALID
    assert _status("pa_msa_boot_counts_host", rows.ctypes.data, 32, 4, 40, w.ctypes.data, 2, m.ctypes.data, b.ctypes.data, 0) == (
        _capi.PA_E_INVALID, "pa_msa_boot_counts_host: row stride 32 below the 40 columns")
    w[1, 5] = 3
    assert _status("pa_msa_boot_counts_host", rows.ctypes.data, 40, 4, 40, w.ctypes.data, 2, m.ctypes.data, b.ctypes.data, 0) == (
        _capi.PA_E_INVALID, "pa_msa_boot_counts_host: the weights of replicate 1 add up to 42, not to the 40 columns")
    assert _status("pa_msa_boot_distances_host", None, b.ctypes.data, 4, 2, 1.0, d.ctypes.data, 0) == (
        _capi.PA_E_INVALID, "pa_msa_boot_distances_host: null argument")
    for missing in (-0.5, float("nan"), float("inf")):
        assert _status("pa_msa_boot_distances_host", m.ctypes.data, b.ctypes.data, 4, 2, missing, d.ctypes.data, 0)[0] == _capi.PA_E_INVALID
    assert _status("pa_msa_boot_weights", 0, 40, 0, 2, None) == (_capi.PA_E_INVALID, "pa_msa_boot_weights: null argument")
    assert _status("pa_msa_boot_weights", 0, 1 << 32, 0, 1, w.ctypes.data)[0] == _capi.PA_E_INVALID
    with pytest.raises(ValueError, match="weights of shape"):
        engine_mod.msa_boot_counts_host(rows, 40, np.ones((2, 39), dtype=np.uint8))


def test_refusals_of_the_support():
    ref = np.array([[0, 1], [2, 3]], dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint32)
    assert _status("pa_tree_support", 4, None, 0, None, out.ctypes.data) == (_capi.PA_E_INVALID, "pa_tree_support: null argument")
    assert _status("pa_tree_support", 4, ref.ctypes.data, 1, None, out.ctypes.data)[0] == _capi.PA_E_INVALID
    assert _status("pa_tree_support", 4, ref.ctypes.data, 0, None, None)[0] == _capi.PA_E_INVALID
    for n in (0, 3, 65536):
        status, message = _status("pa_tree_support", n, ref.ctypes.data, 0, None, out.ctypes.data)
        assert status == _capi.PA_E_INVALID and message == f"pa_tree_support: {n} leaves; 4 to 65535 (fewer have no internal edge)"
    with pytest.raises(_capi.HipBackendError, match="join 1 of the reference tree"):
        engine_mod.tree_support(4, np.array([[0, 1], [1, 2]], dtype=np.uint32), np.empty((0, 2, 2), dtype=np.uint32))  # leaf 1 twice
    with pytest.raises(_capi.HipBackendError, match="join 0 of replicate 1"):
        engine_mod.tree_support(4, ref, np.array([ref, [[0, 4], [2, 3]]], dtype=np.uint32))  # node 4 before it is made


def test_a_weight_past_the_limit_names_the_replicate_and_the_column(monkeypatch):
    tools = _capi.load_library(tools=True)
    whole = engine_mod.msa_boot_weights(0, 97, 0, 50)
    assert whole.max() >= 4
    monkeypatch.setenv("PA_BOOT_WEIGHT_LIMIT", "3")
    np.testing.assert_array_equal(engine_mod.msa_boot_weights(0, 97, 0, 50), whole)  # the product library does not read it
    first = next(r for r in range(50) if whole[r].max() > 3)
    # the column of that replicate whose fourth hit comes first in the order of the draws
    hits, column = np.zeros(97, dtype=int), None
    base = cases.fin((cases.fin(0) + first) & cases.MASK)
    for t in range(97):
        c = (cases.fin((base + t) & cases.MASK) * 97) >> 64
        hits[c] += 1
        if hits[c] > 3:
            column = c
            break
    with pytest.raises(_capi.HipBackendError) as err:
        engine_mod.msa_boot_weights(0, 97, 0, 50, lib=tools)
    assert err.value.status == _capi.PA_E_INVALID
    assert f"replicate {first} draws column {column} more than 3 times" in str(err.value)
