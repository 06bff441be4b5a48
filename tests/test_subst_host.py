"""phylo-run without a GPU: the code table, the rule's logarithm against ``decimal``, the host twins of the counts and of
the distances against the restatement of ``tests/subst_cases.py``, the hand-built edges of the rule, and the refusals.

Measured here (worst case of ``pa_subst_log_host`` against the logarithm at 50 digits, in ulp of the true value): 0.748
over the quotients a/b, 0.748 over the uniform sample, 0.700 over the values 1 - u 2^-k; the condition is 4."""

from __future__ import annotations

import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd import engine as engine_mod
from tests import bootstrap_cases
from tests import subst_cases as cases
from tests import tree_cases

MAX_LOG_ULP = 4.0


# ------------------------------------------------------------------ the code table
def test_the_code_table_is_the_restatements():
    got = engine_mod.subst_code_table()
    assert got.dtype == np.uint8 and got.shape == (256,)
    np.testing.assert_array_equal(got, cases.code_table())
    assert _capi.PA_SUBST_BITS == 3 and int(got.max()) < 1 << _capi.PA_SUBST_BITS and got[ord("-")] == 0  # noqa: PLR2004
    assert sorted(set(got.tolist())) == [0, 4, 5, 6, 7] and int((got != 0).sum()) == 10  # noqa: PLR2004


# ------------------------------------------------------------------ the logarithm
def _ulp_errors(x: np.ndarray) -> np.ndarray:
    """|L(x) - ln x| in ulp of ln x, ln x from ``decimal`` at 50 digits."""
    getcontext().prec = 50
    got = engine_mod.subst_log_host(x)
    out = np.zeros(len(x))
    for k, (value, mine) in enumerate(zip(x.tolist(), got.tolist())):
        true = Decimal(value).ln()
        if true == 0:
            assert mine == 0.0
            continue
        ulp = Decimal(math.ulp(float(true)))
        out[k] = float(abs(Decimal(mine) - true) / ulp)
    return out


def test_the_logarithm_is_within_four_ulp_of_the_true_value():
    quotients = np.array([a / b for b in range(1, 200) for a in range(1, b + 1)])
    uniform = np.random.default_rng(69).random(20_000)
    uniform = uniform[uniform > 0]
    rng = np.random.default_rng(80)
    near_one = np.array([1.0 - u * 2.0**-k for k in range(1, 50) for u in rng.random(50) if u > 0])
    assert len(quotients) == 199 * 200 // 2 and len(near_one) >= 49 * 49
    worst = {}
    for name, sample in (("a/b", quotients), ("uniform", uniform), ("1 - u 2^-k", near_one)):
        errors = _ulp_errors(sample)
        worst[name] = float(errors.max())
        print(f"L against decimal, {name}: {len(sample)} values, worst {worst[name]:.3f} ulp at {sample[int(errors.argmax())]!r}")
    assert max(worst.values()) <= MAX_LOG_ULP, worst


def test_the_logarithm_of_one_and_of_what_is_no_positive_number():
    got = engine_mod.subst_log_host(np.array([1.0, 0.0, -0.0, -1.0, math.inf, math.nan, 5e-324, 2.0]))
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert got[1] == -math.inf and got[2] == -math.inf and math.isnan(got[3]) and got[4] == math.inf and math.isnan(got[5])
    assert abs(got[6] - math.log(5e-324)) <= 2 * math.ulp(got[6]) and abs(got[7] - math.log(2.0)) <= math.ulp(got[7])


# ------------------------------------------------------------------ counts
def test_the_two_restatements_of_the_counts_agree():
    """The pair-and-column loop against the numpy form the larger cases use."""
    for name in ("rows2", "cols33", "cols257_weighted", "weights_nb8"):
        case = cases.count_case(name)
        for r in range(1 if case.weights is None else len(case.weights)):
            w = None if case.weights is None else case.weights[r]
            for a, b in zip(cases.counts(case.rows, w), cases.counts_fast(case.rows, w)):
                np.testing.assert_array_equal(a, b)


def test_the_cases_cover_what_they_name():
    assert {c.rows.shape[0] for c in cases.count_cases()} >= {1, 2, 5, 63, 64, 65, 130}
    assert {c.rows.shape[1] for c in cases.count_cases()} >= {0, 1, 31, 32, 33, 255, 256, 257, cases.SPLIT_COLUMNS}
    assert cases.count_case("weights_nb1").weights.max() == 1 and cases.count_case("weights_nb8").weights.max() == 255  # noqa: PLR2004
    assert (cases.count_case("weights_one_column").weights != 0).sum() == 1
    assert len(cases.count_case("batch_plus_one").weights) == _capi.PA_MSA_BOOT_BATCH + 1
    mix = set(cases.count_case("cols257").rows.ravel().tolist())
    assert mix >= set(b"acgtUuN-RY")  # lower case, U, N, IUPAC letters and the gap
    for compute_units in (1, 64, 256, 304):
        assert cases.split_of("split", compute_units).splits > 1 and cases.split_of("split_weighted", compute_units).splits > 1
    v, s, t = cases.restated_counts("rows130")
    assert (s > 0).sum() > 1000 and (t > 0).sum() > 1000 and (v.diagonal(axis1=1, axis2=2) > 0).all()  # noqa: PLR2004


@pytest.mark.parametrize("name", [c.name for c in cases.count_cases()])
def test_host_counts_equal_the_restatement(name):
    case = cases.count_case(name)
    got = engine_mod.msa_subst_counts_host(case.rows, case.rows.shape[1], case.weights)
    for mine, want in zip(got, cases.restated_counts(name)):
        assert mine.dtype == np.uint32
        np.testing.assert_array_equal(mine, want)
    valid, ts, tv = got
    np.testing.assert_array_equal(valid, valid.transpose(0, 2, 1))
    assert not ts.diagonal(axis1=1, axis2=2).any() and not tv.diagonal(axis1=1, axis2=2).any()


def test_unit_weights_equal_the_unweighted_call():
    case = cases.count_case("weights_nb1")
    for a, b in zip(engine_mod.msa_subst_counts_host(case.rows, 300, case.weights), engine_mod.msa_subst_counts_host(case.rows, 300)):
        np.testing.assert_array_equal(a, b)


def test_host_counts_do_not_depend_on_the_threads_or_on_what_follows_the_columns():
    case = cases.count_case("rows65_weighted")
    one = engine_mod.msa_subst_counts_host(case.rows, 70, case.weights, threads=1)
    padded = np.full((65, 96), ord("A"), dtype=np.uint8)  # residues past the columns are not read as columns
    padded[:, :70] = case.rows
    for got in (engine_mod.msa_subst_counts_host(case.rows, 70, case.weights, threads=7), engine_mod.msa_subst_counts_host(padded, 70, case.weights),
                engine_mod.msa_subst_counts_host(padded, 70, case.weights[:1])):  # fmt: skip
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a, b[: len(a)])
    for a, b in zip(engine_mod.msa_subst_counts_host(padded, 70), cases.restated_counts("rows65")):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ distances
@pytest.mark.parametrize("model", list(cases.MODELS))
@pytest.mark.parametrize("name", ["rows2", "rows65_weighted", "cols0", "cols1_weighted", "cols257", "weights_nb8", "weights_one_column"])
def test_host_distances_equal_the_restatement(name, model):
    valid, ts, tv = cases.restated_counts(name)
    D, undefined = engine_mod.subst_distances_host(valid, ts, tv, model, 2.5)
    assert D.shape == valid.shape and undefined.shape == (len(valid), 2) and undefined.dtype == np.uint64
    for r in range(len(valid)):
        cases.assert_distances(D[r], undefined[r], cases.distances(valid[r], ts[r], tv[r], model, 2.5), f"{name}, {model}, matrix {r}")
        np.testing.assert_array_equal(D[r].view(np.uint64), D[r].T.view(np.uint64))
        engine_mod.nj_tree_host(D[r])  # opens with pa_check_distance_matrix_host: finite, not negative, symmetric, zero diagonal
    if name == "cols0":
        assert undefined.tolist() == [[10, 0]] and (D[0][~np.eye(5, dtype=bool)] == 2.5).all()  # noqa: PLR2004


def test_the_distances_take_logarithms_somewhere():
    valid, ts, tv = cases.restated_counts("rows65_weighted")
    for model in ("jc69", "k80"):
        want = cases.distances(valid[0], ts[0], tv[0], model, 2.5)
        assert (~want.exact).sum() > 3000 and want.undefined[0] == 0 and want.undefined[1] < 50  # noqa: PLR2004


@pytest.mark.parametrize("model", list(cases.MODELS))
def test_the_edges_of_the_rule(model):
    valid, ts, tv = cases.edge_counts()
    D, undefined = engine_mod.subst_distances_host(valid, ts, tv, model, 7.0, threads=3)
    want = cases.distances(valid[0], ts[0], tv[0], model, 7.0)
    cases.assert_distances(D[0], undefined[0], want, model)
    engine_mod.nj_tree_host(D[0])  # pa_check_distance_matrix_host passes
    row = D[0, 0]
    assert row[1] == 7.0 and row[2] == 0.0 and not np.signbit(row[2])  # no column; no difference: +0.0  # noqa: PLR2004
    saturated = {"p": [], "jc69": [3], "k80": [3, 4, 5, 6, 7]}[model]
    assert [k for k in range(2, 10) if row[k] == 7.0] == saturated and want.undefined == (1, len(saturated))  # noqa: PLR2004
    if model == "jc69":
        assert row[4] == pytest.approx(-0.75 * math.log(3 / 9003), rel=1e-12) and row[4] > 6  # a just above 0  # noqa: PLR2004
    if model == "k80":
        assert row[8] == pytest.approx(-0.5 * math.log(1 / 8001) - 0.25 * math.log(1 - 4000 / 8001), rel=1e-9)  # a just above 0
    if model == "p":
        assert row[3] == 0.75 and row[6] == 0.6  # noqa: PLR2004


def test_the_undefined_pairs_are_counted_per_matrix():
    valid, ts, tv = (np.concatenate([x, x, x]) for x in cases.edge_counts())
    valid[1] = 0  # the second matrix: no pair shares a column
    ts[2], tv[2] = 0, 0  # the third: no pair differs
    D, undefined = engine_mod.subst_distances_host(valid, ts, tv, "k80", 1.0)
    assert undefined.tolist() == [[1, 5], [45, 0], [1, 0]]
    assert (D[1][~np.eye(10, dtype=bool)] == 1.0).all() and not D[2][valid[2] > 0].any()


def test_the_strided_counts_reach_the_second_trip_and_the_second_launch():
    """The conditions on the hand-built counts of ``tests/test_gpu_subst.py``, from the constants of the sources."""
    counts, trip, batch = cases.strided_counts(), bootstrap_cases.stride_cells(), cases.distance_batch()
    reps, n, _ = counts.valid.shape
    assert (reps, n) == (cases.STRIDED_REPLICATES, cases.STRIDED_ROWS) == (5, 257) and batch == 4  # noqa: PLR2004
    assert batch < reps < 2 * batch and (batch - 1) * n * n < trip < batch * n * n < 2 * trip  # one launch loops, once; one follows
    first_row = (trip - (batch - 1) * n * n) // n + 1  # the first row of matrix 3 that is on the second trip whole
    assert first_row == 250 and batch * n * n - trip == 2052 and (batch * n * n - trip) % 64 == 4  # the last wave: four lanes  # noqa: PLR2004
    strided = cases.strided_cells_of(counts, first_row)
    assert len(strided) == 2 * 5 and min(strided) >= trip and max(strided) < batch * n * n  # noqa: PLR2004
    late = [kind for (i, _j), kind in counts.planted[batch - 1] if i >= first_row]
    assert late.count(cases.NO_COLUMNS) == 3 and late.count(cases.SATURATED) == 2  # noqa: PLR2004
    assert all(any(i < first_row for (i, _j), _kind in of) for of in counts.planted)  # and the first trip of every matrix
    for kind in (0, 1):
        assert len({row[kind] for row in counts.undefined("k80")}) == reps  # every matrix another number of each kind
    for x in (counts.valid, counts.ts, counts.tv):
        np.testing.assert_array_equal(x, x.transpose(0, 2, 1))


@pytest.mark.parametrize("model", list(cases.MODELS))
def test_the_planted_pairs_are_the_undefined_pairs_of_the_twin(model):
    counts = cases.strided_counts()
    D, undefined = engine_mod.subst_distances_host(counts.valid, counts.ts, counts.tv, model, 0.75)
    assert undefined.tolist() == counts.undefined(model)
    for r, of in enumerate(counts.planted):
        for (i, j), kind in of:
            assert (D[r, i, j] == 0.75) == (model != "p" or kind == cases.NO_COLUMNS) and D[r, j, i] == D[r, i, j]  # noqa: PLR2004
    assert (D == 0.75).sum() == 2 * int(undefined.sum())  # noqa: PLR2004
    for n, reps in ((3, 27), (2, 9)):
        small = cases.small_counts(n)
        assert len(small.valid) == reps and n * n * cases.distance_batch() <= 64  # a wave spans a whole launch  # noqa: PLR2004
        D, undefined = engine_mod.subst_distances_host(small.valid, small.ts, small.tv, model, 0.75)
        assert undefined.tolist() == small.undefined(model)
        for r in range(reps):
            cases.assert_distances(D[r], undefined[r], cases.distances(small.valid[r], small.ts[r], small.tv[r], model, 0.75), f"{model}, {n}, {r}")
    three = cases.small_counts(3).undefined("k80")
    assert len({tuple(x) for x in three}) == 10 and three[0] == [0, 0] and three[13] == [3, 0] and three[26] == [0, 3]  # noqa: PLR2004
    assert sum(x != [0, 0] for x in three[1:4]) == 3  # undefined pairs in the matrices that do not lead the first wave  # noqa: PLR2004


def test_the_tied_alignment_ties_on_more_than_one_tile():
    """The condition of ``tests/test_tree_host.py`` on the matrices the device pipeline test joins: of the joins made
    while more than kTile nodes are live, at least a third are tied.  Counted here: 23 to 27 of 52 in each."""
    rows = cases.tied_alignment()
    n, n_cols = rows.shape
    assert n == 180 > tree_cases.kernel_constants()["kTile"]  # noqa: PLR2004
    w = engine_mod.msa_boot_weights(0, n_cols, 0, 3)
    for model in ("p", "k80"):
        plain, _ = engine_mod.subst_distances_host(*engine_mod.msa_subst_counts_host(rows, n_cols), model, 3.0)
        drawn, _ = engine_mod.subst_distances_host(*engine_mod.msa_subst_counts_host(rows, n_cols, w), model, 3.0)
        for what, D in (("unweighted", plain[0]), *((f"replicate {r}", drawn[r]) for r in range(3))):
            tied, joins = tree_cases.tied_share(tree_cases.tied_pairs_per_join(D), n)
            print(f"{model}, {what}: {tied} of {joins} joins on more than one tile are tied")
            assert joins == n - tree_cases.kernel_constants()["kTile"] and 3 * tied >= joins, (model, what)


def test_the_tree_of_the_host_distances_is_the_restatements():
    rows = cases.alignment(9, 130, 21)
    for model in cases.MODELS:
        D, _undefined = engine_mod.subst_distances_host(*engine_mod.msa_subst_counts_host(rows, 130), model, 3.0)
        want = cases.pipeline(rows, model, 3.0)
        child, length, last, last_len = engine_mod.nj_tree_host(D[0])
        cases.assert_same_tree(9, tree_cases.Joins(child, length, (int(last[0]), int(last[1])), last_len), want.reference, model)


def test_the_replicate_loop_takes_the_substitution_step():
    from pyani_plus_amd import bootstrap as bootstrap_mod
    from pyani_plus_amd import substitution

    rows = cases.alignment(9, 130, 22)
    want = cases.pipeline(rows, "p", 3.0, replicates=6, seed=5)  # p: no logarithm, so the trees are the restatement's bit for bit
    trees = bootstrap_mod.replicate_trees(rows, 130, 6, 5, 3.0, step=substitution.replicate_step("p"))
    for got, restated in zip(trees, want.trees):
        np.testing.assert_array_equal(got.child, restated.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), np.asarray(restated.length).view(np.uint64))
    identity = bootstrap_mod.replicate_trees(rows, 130, 6, 5, 3.0)  # the default is what it was: 1 - identity
    again = bootstrap_mod.replicate_trees(rows, 130, 6, 5, 3.0, step=bootstrap_mod.IDENTITY_STEP)
    r = [bootstrap_cases.distances(*bootstrap_cases.counts(rows, w), 3.0) for w in bootstrap_cases.weights(5, 130, 0, 6)]
    for a, b, d in zip(identity, again, r):
        np.testing.assert_array_equal(a.child, b.child)
        np.testing.assert_array_equal(a.child, engine_mod.nj_tree_host(d)[0])
    assert any(not np.array_equal(a.length, b.length) for a, b in zip(identity, trees))


# ------------------------------------------------------------------ refusals
def _status(fn, *args) -> tuple[int, str]:
    lib = _capi.load_library()
    status = getattr(lib, fn)(*args)
    return status, _capi.last_error(lib)


def test_refusals_of_the_counts():
    rows = np.ascontiguousarray(cases.alignment(4, 40, 1))
    w = np.ones((2, 40), dtype=np.uint8)
    out = [np.zeros((2, 4, 4), dtype=np.uint32) for _ in range(3)]
    p = [x.ctypes.data for x in out]
    fn = "pa_msa_subst_counts_host"
    assert _status(fn, None, 40, 4, 40, w.ctypes.data, 2, *p, 0) == (_capi.PA_E_INVALID, f"{fn}: null argument")
    for k in range(3):
        q = list(p)
        q[k] = None
        assert _status(fn, rows.ctypes.data, 40, 4, 40, w.ctypes.data, 2, *q, 0) == (_capi.PA_E_INVALID, f"{fn}: null argument")
    assert _status(fn, rows.ctypes.data, 40, 4, 40, None, 2, *p, 0) == (_capi.PA_E_INVALID, f"{fn}: 2 replicates without weights; 1 without them")
    assert _status(fn, rows.ctypes.data, 1 << 32, 4, 1 << 32, w.ctypes.data, 2, *p, 0) == (_capi.PA_E_INVALID, f"{fn}: 4294967296 columns (at most 2^32 - 1)")
    assert _status(fn, rows.ctypes.data, 40, 65536, 40, w.ctypes.data, 2, *p, 0) == (_capi.PA_E_INVALID, f"{fn}: 65536 rows; at most 65535")
    assert _status(fn, rows.ctypes.data, 32, 4, 40, w.ctypes.data, 2, *p, 0) == (_capi.PA_E_INVALID, f"{fn}: row stride 32 below the 40 columns")
    w[1, 5] = 3
    assert _status(fn, rows.ctypes.data, 40, 4, 40, w.ctypes.data, 2, *p, 0) == (
        _capi.PA_E_INVALID, f"{fn}: the weights of replicate 1 add up to 42, not to the 40 columns")
    w[1, 5], w[1, 6] = 0, 1  # all weights at most 1, another sum
    assert _status(fn, rows.ctypes.data, 40, 4, 40, w.ctypes.data, 2, *p, 0) == (
        _capi.PA_E_INVALID, f"{fn}: the weights of replicate 1 add up to 39, not to the 40 columns")
    # no-ops: no rows, no replicates
    assert _status(fn, None, 40, 0, 40, None, 1, None, None, None, 0)[0] == _capi.PA_OK
    assert _status(fn, None, 40, 4, 40, None, 0, None, None, None, 0)[0] == _capi.PA_OK
    with pytest.raises(ValueError, match="weights of shape"):
        engine_mod.msa_subst_counts_host(rows, 40, np.ones((2, 39), dtype=np.uint8))
    assert _status("pa_subst_code", None) == (_capi.PA_E_INVALID, "pa_subst_code: null argument")
    assert _status("pa_subst_log_host", None, 1, None) == (_capi.PA_E_INVALID, "pa_subst_log_host: null argument")
    assert _status("pa_subst_log_host", None, 0, None)[0] == _capi.PA_OK


def test_refusals_of_the_distances():
    v, s, t = (np.zeros((2, 4, 4), dtype=np.uint32) for _ in range(3))
    d, u = np.zeros((2, 4, 4)), np.zeros((2, 2), dtype=np.uint64)
    fn = "pa_subst_distances_host"
    good = [v.ctypes.data, s.ctypes.data, t.ctypes.data, 4, 2, 2, 1.0, d.ctypes.data, u.ctypes.data, 0]
    for k in (0, 1, 2, 7, 8):
        bad = list(good)
        bad[k] = None
        assert _status(fn, *bad) == (_capi.PA_E_INVALID, f"{fn}: null argument")
    for model in (-1, 3):
        bad = list(good)
        bad[5] = model
        assert _status(fn, *bad) == (_capi.PA_E_INVALID, f"{fn}: unknown model {model} (0: p, 1: jc69, 2: k80)")
    for missing in (-0.5, float("nan"), float("inf")):
        bad = list(good)
        bad[6] = missing
        assert _status(fn, *bad) == (_capi.PA_E_INVALID, f"{fn}: the distance of a pair without columns must be finite and not negative")
    assert _status(fn, *good)[0] == _capi.PA_OK and u.tolist() == [[6, 0], [6, 0]]
    assert _status(fn, None, None, None, 4, 0, 2, 1.0, None, None, 0)[0] == _capi.PA_OK  # no replicates
    assert _status(fn, None, None, None, 0, 2, 2, 1.0, None, u.ctypes.data, 0)[0] == _capi.PA_OK and not u.any()  # no rows
    with pytest.raises(ValueError, match="unknown substitution model 'tn93'"):
        engine_mod.subst_distances_host(v, s, t, "tn93")
    with pytest.raises(ValueError, match="counts of shapes"):
        engine_mod.subst_distances_host(v, s[:1], t)


# ------------------------------------------------------------------ the host code under sanitizers
def test_host_twins_under_sanitizers():
    """AddressSanitizer + UBSan over ``subst_host.cpp`` in a stand-alone CPU program: random rows of nucleotides in both
    cases, IUPAC letters and gaps, with and without weights, in exact-size buffers, the counts checked against the plain
    loop and the undefined pairs against the ``missing`` cells."""
    import shutil
    import subprocess
    from pathlib import Path

    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    script = Path(__file__).resolve().parent / "tools" / "sanitize" / "run_subst.sh"
    done = subprocess.run(["bash", str(script), "100"], capture_output=True, text=True, timeout=600, check=False)
    assert done.returncode == 0 and "sanitizer runs clean" in done.stdout, done.stdout[-2000:] + done.stderr[-2000:]
    assert "MISMATCH" not in done.stdout
