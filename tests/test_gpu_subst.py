"""phylo-run on the MI355X: the three counts against the host twin and the restatement (exactly: they are integers), the
distances and the undefined pairs against the twin's bits, a matrix straight into ``pa_nj``, the command against the host
path's bytes, and the other entry points of the alignment's planes in the same context.  The shapes are
``tests/subst_cases.py``'s: the smallest that reach each seam."""

from __future__ import annotations

import logging

import numpy as np
import pytest

from pyani_plus_amd import _capi, rundb
from pyani_plus_amd import engine as engine_mod
from pyani_plus_amd.engine import HipEngine, LoadedMSA
from tests import bootstrap_cases
from tests import subst_cases as cases
from tests.msa_checker import counts_matrix

pytestmark = pytest.mark.gpu

LOGGER = logging.getLogger("test")


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def loaded(rows: np.ndarray) -> LoadedMSA:
    n, length = rows.shape
    stride = max(32, (length + 31) // 32 * 32)
    padded = np.full((n, stride), ord("A"), dtype=np.uint8)  # residues past the columns: the pack must not count them
    padded[:, :length] = rows
    hist = np.bincount(rows.ravel(), minlength=256).astype(np.uint64)
    return LoadedMSA("", [f"r{i}".encode() for i in range(n)], np.full(n, length, np.uint64), hist, padded, length)


def u32(tensor) -> np.ndarray:
    return tensor.cpu().numpy().view(np.uint32)


def test_the_split_case_splits(engine):
    cus = engine.device_info()["compute_units"]
    for name in ("split", "split_weighted"):
        assert cases.count_case(name).rows.shape == (cases.SPLIT_ROWS, cases.SPLIT_COLUMNS) and cases.split_of(name, cus).splits > 1
    assert cases.split_of("rows130", cus).splits == 1 and _capi.PA_MSA_BOOT_BATCH == cases.BATCH


@pytest.mark.parametrize("name", [c.name for c in cases.count_cases()])
def test_device_counts_equal_the_twin_and_the_restatement(engine, name):
    case = cases.count_case(name)
    dm = engine.msa_subst_upload(loaded(case.rows))
    assert dm.bits == _capi.PA_SUBST_BITS
    got = engine.msa_subst_counts(dm, case.weights)
    twin = engine_mod.msa_subst_counts_host(case.rows, case.rows.shape[1], case.weights)
    for mine, host, want in zip(got, twin, cases.restated_counts(name)):
        np.testing.assert_array_equal(u32(mine), host)
        np.testing.assert_array_equal(u32(mine), want)


def test_unit_weights_equal_the_unweighted_call(engine):
    case = cases.count_case("weights_nb1")
    dm = engine.msa_subst_upload(loaded(case.rows))
    for a, b in zip(engine.msa_subst_counts(dm, case.weights), engine.msa_subst_counts(dm)):
        np.testing.assert_array_equal(u32(a), u32(b))


def test_two_calls_on_the_same_buffers_give_the_same(engine):
    """The split form adds into its output with atomics: the call itself has to clear it."""
    t = engine.torch
    for name in ("split", "split_weighted", "rows130_weighted"):
        case = cases.count_case(name)
        dm = engine.msa_subst_upload(loaded(case.rows))
        w = None if case.weights is None else np.ascontiguousarray(case.weights)
        n, reps = dm.n_rows, 1 if w is None else len(w)
        out = [t.full((reps, n, n), -1, dtype=t.int32, device=engine.device) for _ in range(3)]
        for _ in range(2):
            engine._check(engine.lib.pa_msa_subst_counts(engine.ctx, dm.planes.data_ptr(), n, dm.n_cols, None if w is None else w.ctypes.data, reps,
                                                         *(x.data_ptr() for x in out)), "pa_msa_subst_counts")  # fmt: skip
            for mine, want in zip(out, cases.restated_counts(name)):
                np.testing.assert_array_equal(u32(mine), want)


@pytest.mark.parametrize("model", list(cases.MODELS))
@pytest.mark.parametrize("name", ["rows2", "rows65_weighted", "rows130", "cols0", "cols257_weighted", "weights_nb8", "batch_plus_one"])
def test_device_distances_have_the_twins_bits(engine, name, model):
    case = cases.count_case(name)
    dm = engine.msa_subst_upload(loaded(case.rows))
    D, undefined = engine.subst_distances(*engine.msa_subst_counts(dm, case.weights), model, 0.75)
    twin, twin_undefined = engine_mod.subst_distances_host(*cases.restated_counts(name), model, 0.75)
    np.testing.assert_array_equal(D.cpu().numpy().view(np.uint64), twin.view(np.uint64))
    np.testing.assert_array_equal(undefined, twin_undefined)
    if name == "cols0":
        assert undefined.tolist() == [[10, 0]]


@pytest.mark.parametrize("model", list(cases.MODELS))
def test_the_edges_of_the_rule_on_the_device(engine, model):
    t = engine.torch
    counts = [np.concatenate([x] * 6) for x in cases.edge_counts()]  # six matrices: a second launch of the distances
    counts[0][4] = 0  # the fifth: no pair shares a column
    d_counts = [t.from_numpy(x.view(np.int32)).to(engine.device) for x in counts]
    D, undefined = engine.subst_distances(*d_counts, model, 7.0)
    twin, twin_undefined = engine_mod.subst_distances_host(*counts, model, 7.0)
    np.testing.assert_array_equal(D.cpu().numpy().view(np.uint64), twin.view(np.uint64))
    np.testing.assert_array_equal(undefined, twin_undefined)
    saturated = {"p": 0, "jc69": 1, "k80": 5}[model]
    assert undefined.tolist() == [[1, saturated]] * 4 + [[45, 0]] + [[1, saturated]]
    cases.assert_distances(twin[0], twin_undefined[0], cases.distances(counts[0][0], counts[1][0], counts[2][0], model, 7.0), model)


def planted_distances_on_the_device(engine, counts, model):
    """Hand-built counts uploaded as they are: the twin's bits, the twin's undefined pairs, and the planted numbers."""
    t = engine.torch
    host = [np.array(x) for x in (counts.valid, counts.ts, counts.tv)]
    D, undefined = engine.subst_distances(*(t.from_numpy(x.view(np.int32)).to(engine.device) for x in host), model, 0.75)
    twin, twin_undefined = engine_mod.subst_distances_host(*host, model, 0.75)
    np.testing.assert_array_equal(D.cpu().numpy().view(np.uint64), twin.view(np.uint64))
    np.testing.assert_array_equal(undefined, twin_undefined)
    assert undefined.tolist() == counts.undefined(model)


@pytest.mark.parametrize("model", list(cases.MODELS))
def test_the_distances_past_the_first_trip_of_a_launch(engine, model):
    """Four matrices of 257 x 257 are more cells than a launch has lanes: the last rows of the fourth are written, and
    their undefined pairs voted on, on the second trip (tests/test_subst_host.py holds the conditions on the counts)."""
    planted_distances_on_the_device(engine, cases.strided_counts(), model)


@pytest.mark.parametrize("model", list(cases.MODELS))
@pytest.mark.parametrize("n", [3, 2])
def test_the_vote_of_a_wave_that_spans_four_matrices(engine, n, model):
    planted_distances_on_the_device(engine, cases.small_counts(n), model)


def test_a_matrix_goes_straight_into_the_joins(engine):
    case = cases.count_case("rows65_weighted")
    dm = engine.msa_subst_upload(loaded(case.rows))
    D, _undefined = engine.subst_distances(*engine.msa_subst_counts(dm, case.weights), "k80", 3.0)
    twin, _ = engine_mod.subst_distances_host(*cases.restated_counts("rows65_weighted"), "k80", 3.0)
    for r in range(len(case.weights)):
        got, want = engine.nj_tree_inplace(D[r]), engine_mod.nj_tree_host(twin[r])
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert got[2].tolist() == want[2].tolist() and got[3] == want[3]


def test_the_refusals_of_the_device_entry_points(engine):
    case = cases.count_case("cols33_weighted")
    dm = engine.msa_subst_upload(loaded(case.rows))
    bad = case.weights.copy()
    bad[2, 0] += 1
    with pytest.raises(_capi.HipBackendError, match="pa_msa_subst_counts: the weights of replicate 2 add up to 34, not to the 33 columns"):
        engine.msa_subst_counts(dm, bad)
    with pytest.raises(ValueError, match="planes of 2 bits"):
        engine.msa_subst_counts(engine.msa_upload(loaded(np.frombuffer(b"ACG-ACGA", dtype=np.uint8).reshape(2, 4))))
    valid, ts, tv = engine.msa_subst_counts(dm, case.weights)
    with pytest.raises(_capi.HipBackendError, match="finite and not negative"):
        engine.subst_distances(valid, ts, tv, "k80", float("nan"))
    with pytest.raises(ValueError, match="unknown substitution model"):
        engine.subst_distances(valid, ts, tv, "tn93")
    lib, p = engine.lib, [x.data_ptr() for x in (valid, ts, tv)]
    u = np.zeros((3, 2), dtype=np.uint64)
    d = engine.torch.empty((3, 5, 5), dtype=engine.torch.float64, device=engine.device)
    assert lib.pa_msa_subst_counts(engine.ctx, None, 5, 33, case.weights.ctypes.data, 3, *p) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_msa_subst_counts: null argument"
    assert lib.pa_msa_subst_counts(engine.ctx, dm.planes.data_ptr(), 5, 33, None, 3, *p) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_msa_subst_counts: 3 replicates without weights; 1 without them"
    assert lib.pa_msa_subst_counts(engine.ctx, dm.planes.data_ptr(), 65536, 33, None, 1, *p) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_msa_subst_counts: 65536 rows; at most 65535"
    assert lib.pa_msa_subst_counts(engine.ctx, dm.planes.data_ptr(), 5, 1 << 32, None, 1, *p) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_msa_subst_counts: 4294967296 columns (at most 2^32 - 1)"
    assert lib.pa_subst_distances(engine.ctx, *p, 5, 3, 3, 1.0, d.data_ptr(), u.ctypes.data) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_subst_distances: unknown model 3 (0: p, 1: jc69, 2: k80)"
    assert lib.pa_subst_distances(engine.ctx, *p, 5, 3, 2, 1.0, None, u.ctypes.data) == _capi.PA_E_INVALID
    assert lib.pa_subst_distances(engine.ctx, *p, 5, 3, 2, 1.0, d.data_ptr(), None) == _capi.PA_E_INVALID
    assert _capi.last_error(lib) == "pa_subst_distances: null argument"
    assert lib.pa_msa_subst_counts(engine.ctx, None, 0, 33, None, 1, None, None, None) == _capi.PA_OK  # no rows, no replicates: nothing to do
    assert lib.pa_msa_subst_counts(engine.ctx, None, 5, 33, None, 0, None, None, None) == _capi.PA_OK
    assert lib.pa_subst_distances(engine.ctx, None, None, None, 5, 0, 2, 1.0, None, None) == _capi.PA_OK


def test_the_other_counts_of_the_planes_share_the_context(engine):
    """``pa_msa_pair_counts`` and ``pa_msa_boot_counts`` read the same three-bit planes and the same workspace: larger
    inputs first, then smaller ones on the workspace the larger left, each result what it is alone."""
    for name, reps in (("rows130_weighted", 2), ("cols257_weighted", 3), ("batch_plus_one", cases.BATCH + 1), ("cols33_weighted", 3)):
        case = cases.count_case(name)
        rows, n_cols = np.asarray(case.rows), case.rows.shape[1]
        dm = engine.msa_subst_upload(loaded(rows))
        coded = cases.code_table()[rows]
        as_bytes = np.where(coded == 0, ord("-"), coded + ord("0")).astype(np.uint8)  # what the planes say: a gap or one of four residues
        want_pairs, want_plain = counts_matrix(as_bytes), cases.counts_fast(rows)
        want_boot = [bootstrap_cases.counts(as_bytes, case.weights[r]) for r in range(reps)]
        for _ in range(2):
            subst = engine.msa_subst_counts(dm, case.weights)
            boot = engine.msa_boot_counts(dm, case.weights)
            pairs = engine.msa_pair_counts(dm, symmetric=True)
            plain = engine.msa_subst_counts(dm)
            for mine, want in zip(subst, cases.restated_counts(name)):
                np.testing.assert_array_equal(u32(mine), want)
            for mine, want in zip(plain, want_plain):
                np.testing.assert_array_equal(u32(mine)[0], want)
            for k in range(2):
                np.testing.assert_array_equal(u32(pairs[k]), want_pairs[k])
                np.testing.assert_array_equal(u32(boot[k]), np.stack([w[k] for w in want_boot]).astype(np.uint32))
        np.testing.assert_array_equal(u32(subst[0]), u32(boot[1]))  # V is B of the same planes


def test_the_trees_of_the_device_are_the_hosts(engine):
    from pyani_plus_amd import bootstrap as bootstrap_mod
    from pyani_plus_amd import substitution

    rows = cases.alignment(12, 300, 12)
    dm = engine.msa_subst_upload(loaded(rows))
    step = substitution.replicate_step("k80")
    device = bootstrap_mod.replicate_trees(rows, 300, cases.BATCH + 2, 0, 3.0, engine=engine, device_msa=dm, step=step)
    host = bootstrap_mod.replicate_trees(rows, 300, cases.BATCH + 2, 0, 3.0, step=step)
    assert len(device) == cases.BATCH + 2
    for got, want in zip(device, host):
        np.testing.assert_array_equal(got.child, want.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), want.length.view(np.uint64))
        assert got.last == want.last and got.last_len == want.last_len


def test_the_trees_of_the_device_are_the_hosts_where_ties_decide_on_two_tiles(engine):
    """180 rows, every row three times: device-made matrices with ties go into the joins in place, on more than one scan
    tile (tests/test_subst_host.py counts the tied joins)."""
    from pyani_plus_amd import bootstrap as bootstrap_mod
    from pyani_plus_amd import substitution

    rows = cases.tied_alignment()
    n_cols = rows.shape[1]
    dm = engine.msa_subst_upload(loaded(rows))
    step = substitution.replicate_step("k80")
    device = bootstrap_mod.replicate_trees(rows, n_cols, cases.BATCH + 2, 0, 3.0, engine=engine, device_msa=dm, step=step)
    host = bootstrap_mod.replicate_trees(rows, n_cols, cases.BATCH + 2, 0, 3.0, step=step)
    assert len(device) == len(host) == cases.BATCH + 2
    for got, want in zip(device, host):
        np.testing.assert_array_equal(got.child, want.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), want.length.view(np.uint64))
        assert got.last == want.last and got.last_len == want.last_len


@pytest.mark.parametrize("replicates", [0, 40])
def test_the_command_on_the_device_writes_the_host_paths_bytes(engine, tmp_path, replicates):
    from tests.test_bootstrap_command import NAMES
    from tests.test_phylo_command import write_run

    rows = cases.alignment(9, 64, 13, alphabet=b"ACGTacgtN", mutate=0.2)
    db, _aln = write_run(tmp_path, rows, NAMES)
    host = rundb.phylo_run(db, tmp_path / "host", replicates=replicates, seed=4, keep_trees=True)
    device = rundb.phylo_run(db, tmp_path / "device", replicates=replicates, seed=4, keep_trees=True, engine=engine)
    assert [p.name for p in host] == [p.name for p in device] and len(host) == (5 if replicates else 2)
    for a, b in zip(host, device):
        assert a.read_bytes() == b.read_bytes()
    if replicates:
        supports = [int(line.split("\t")[3]) for line in host[3].read_text().split("\n")[1:-1]]
        assert len(supports) == 6 and min(supports) < replicates  # noqa: PLR2004
