"""bootstrap-run on the MI355X: the weighted pair counts against the host twin and the restatement (exactly: they are
integers), the distances against the twin's bits, the command against the host path's bytes, and the unweighted pair
counts left as they were.  The shapes are ``tests/bootstrap_cases.py``'s: the smallest at which the kernel can go wrong."""

from __future__ import annotations

import logging

import numpy as np
import pytest

from pyani_plus_amd import _capi, rundb
from pyani_plus_amd import engine as engine_mod
from pyani_plus_amd.engine import HipEngine, LoadedMSA, msa_code_table
from tests import bootstrap_cases as cases
from tests.msa_checker import NumpyMsaEngine, counts_matrix

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
    padded = np.full((n, stride), cases.GAP, dtype=np.uint8)
    padded[:, :length] = rows
    hist = np.bincount(rows.ravel(), minlength=256).astype(np.uint64)
    return LoadedMSA("", [f"r{i}".encode() for i in range(n)], np.full(n, length, np.uint64), hist, padded, length)


def u32(tensor) -> np.ndarray:
    return tensor.cpu().numpy().view(np.uint32)


def test_the_cases_cover_what_they_name():
    assert _capi.PA_MSA_BOOT_BATCH == cases.BATCH
    assert len(cases.count_case("batch_plus_one").weights) == cases.BATCH + 1
    for bits in (1, 2, 4, 5, 6, 7, 8):
        assert msa_code_table(loaded(cases.count_case(f"bits{bits}").rows).histogram)[1] == bits
    assert msa_code_table(loaded(cases.count_case("rows65").rows).histogram)[1] == 3  # ACGT: every other case
    assert cases.count_case("weights_max1").weights.max() == 1 and cases.count_case("weights_max255").weights.max() == 255
    assert 3 <= max(int(cases.count_case(f"rows{n}").weights.max()) for n in (1, 4, 63, 64, 65, 130)) <= 7


@pytest.mark.parametrize("name", [c.name for c in cases.count_cases()])
def test_device_counts_equal_the_twin_and_the_restatement(engine, name):
    case = cases.count_case(name)
    dm = engine.msa_upload(loaded(case.rows))
    match, both = engine.msa_boot_counts(dm, case.weights)
    twin_m, twin_b = engine_mod.msa_boot_counts_host(case.rows, case.rows.shape[1], case.weights)
    want_m, want_b = cases.restated_counts(name)
    for got, twin, want in ((u32(match), twin_m, want_m), (u32(both), twin_b, want_b)):
        np.testing.assert_array_equal(got, twin)
        np.testing.assert_array_equal(got, want)


def test_two_calls_on_the_same_buffers_give_the_same(engine):
    """The split form adds into its output with atomics: the call itself has to clear it."""
    for name in ("split", "rows130"):
        case = cases.count_case(name)
        dm = engine.msa_upload(loaded(case.rows))
        w = np.ascontiguousarray(case.weights)
        n, reps = dm.n_rows, len(w)
        t = engine.torch
        match = t.full((reps, n, n), -1, dtype=t.int32, device=engine.device)
        both = t.full((reps, n, n), -1, dtype=t.int32, device=engine.device)
        first = None
        for _ in range(2):
            engine._check(engine.lib.pa_msa_boot_counts(engine.ctx, dm.planes.data_ptr(), n, dm.n_cols, dm.bits, w.ctypes.data, reps, match.data_ptr(),
                                                        both.data_ptr()), "pa_msa_boot_counts")  # fmt: skip
            got = (u32(match).copy(), u32(both).copy())
            if first is None:
                first = got
        want = cases.restated_counts(name)
        for a, b, c in zip(first, got, want):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("name", ["all_gap", "weights_max255", "rows65", "batch_plus_one"])
def test_device_distances_have_the_twins_bits(engine, name):
    case = cases.count_case(name)
    dm = engine.msa_upload(loaded(case.rows))
    match, both = engine.msa_boot_counts(dm, case.weights)
    D = engine.msa_boot_distances(match, both, 0.75).cpu().numpy()
    twin = engine_mod.msa_boot_distances_host(*cases.restated_counts(name), 0.75)
    np.testing.assert_array_equal(D.view(np.uint64), twin.view(np.uint64))
    if name == "all_gap":
        assert D[0, 1, 4] == 0.75 and D[1, 4, 1] == 0.75  # two rows without residues: `missing`


def test_the_distances_past_the_first_trip_of_the_launch(engine):
    """Five matrices of 230 x 230 are more cells than the launch has lanes: the last rows of the fifth, two of them
    without a residue, are written on the second trip (tests/test_bootstrap_host.py holds the conditions on the counts)."""
    t = engine.torch
    counts = cases.strided_counts()
    reps = len(counts.match)
    match, both = (t.from_numpy(np.array(x).view(np.int32)).to(engine.device) for x in (counts.match, counts.both))
    D = engine.msa_boot_distances(match, both, 0.75).cpu().numpy()
    twin = engine_mod.msa_boot_distances_host(counts.match, counts.both, 0.75)
    np.testing.assert_array_equal(D.view(np.uint64), twin.view(np.uint64))
    a, b = counts.all_gap[reps - 1]
    assert np.argwhere(D == 0.75).tolist() == [[1, 3, 7], [1, 7, 3], [reps - 1, a, b], [reps - 1, b, a]]  # `missing`, there alone


def test_the_refusals_of_the_device_entry_points(engine):
    case = cases.count_case("cols33")
    dm = engine.msa_upload(loaded(case.rows))
    bad = case.weights.copy()
    bad[2, 0] += 1
    with pytest.raises(_capi.HipBackendError, match="the weights of replicate 2 add up to 34, not to the 33 columns"):
        engine.msa_boot_counts(dm, bad)
    match, both = engine.msa_boot_counts(dm, case.weights)
    with pytest.raises(_capi.HipBackendError, match="finite and not negative"):
        engine.msa_boot_distances(match, both, float("nan"))
    assert engine.lib.pa_msa_boot_counts(engine.ctx, None, 5, 33, dm.bits, case.weights.ctypes.data, 3, match.data_ptr(), both.data_ptr()) == _capi.PA_E_INVALID
    assert engine.lib.pa_msa_boot_distances(engine.ctx, match.data_ptr(), both.data_ptr(), 5, 3, 1.0, None) == _capi.PA_E_INVALID


def test_pair_counts_after_a_boot_call_are_what_they_were(engine):
    case = cases.count_case("rows130")
    dm = engine.msa_upload(loaded(case.rows))
    before = [u32(x).copy() for x in engine.msa_pair_counts(dm, symmetric=True)]
    engine.msa_boot_counts(dm, case.weights)
    after = [u32(x) for x in engine.msa_pair_counts(dm, symmetric=True)]
    want = counts_matrix(np.asarray(case.rows))
    for a, b, c in zip(before, after, want):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    part = [u32(x) for x in engine.msa_pair_counts(dm, (3, 70), (60, 130))]  # the form with two ranges
    for a, c in zip(part, want):
        np.testing.assert_array_equal(a, c[3:70, 60:130])


def test_the_trees_of_the_device_are_the_hosts(engine):
    from pyani_plus_amd import bootstrap as bootstrap_mod

    n, n_cols, seed = cases.SUPPORT_ALIGNMENTS[1]
    r = cases.restated(n, n_cols, seed)
    dm = engine.msa_upload(loaded(r.rows))
    trees = bootstrap_mod.replicate_trees(r.rows, n_cols, cases.SUPPORT_REPLICATES, 0, engine=engine, device_msa=dm)
    for got, want in zip(trees, r.trees):
        np.testing.assert_array_equal(got.child, want.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), want.length.view(np.uint64))
        assert got.last == want.last and got.last_len == want.last_len


def test_the_trees_of_the_device_are_the_hosts_where_ties_decide_on_two_tiles(engine):
    """180 rows, every row three times: device-made matrices with ties go into the joins in place, on more than one scan
    tile (tests/test_bootstrap_host.py counts the tied joins)."""
    from pyani_plus_amd import bootstrap as bootstrap_mod

    rows = cases.tied_alignment()
    n_cols = rows.shape[1]
    dm = engine.msa_upload(loaded(rows))
    device = bootstrap_mod.replicate_trees(rows, n_cols, cases.BATCH + 2, 0, engine=engine, device_msa=dm)
    host = bootstrap_mod.replicate_trees(rows, n_cols, cases.BATCH + 2, 0)
    assert len(device) == len(host) == cases.BATCH + 2
    for got, want in zip(device, host):
        np.testing.assert_array_equal(got.child, want.child)
        np.testing.assert_array_equal(got.length.view(np.uint64), want.length.view(np.uint64))
        assert got.last == want.last and got.last_len == want.last_len


def test_the_command_on_the_device_writes_the_host_paths_bytes(engine, tmp_path):
    from tests.test_bootstrap_command import NAMES, stem

    rows = cases.alignment(9, 64, 13)
    fasta = tmp_path / "genomes"
    fasta.mkdir()
    for name, row in zip(NAMES, rows):
        (fasta / name).write_bytes(b">" + stem(name).encode() + b"\n" + bytes(row[row != cases.GAP]) + b"\n")
    aln = tmp_path / "nine.aln.fasta"
    aln.write_bytes(b"".join(b">" + stem(name).encode() + b"\n" + bytes(row) + b"\n" for name, row in zip(NAMES, rows)))
    db = tmp_path / "runs.sqlite"
    assert rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp_path / "t", logger=LOGGER, engine=NumpyMsaEngine()).status == "Done"
    host = rundb.bootstrap_run(db, tmp_path / "host", replicates=40, seed=4, keep_trees=True)
    device = rundb.bootstrap_run(db, tmp_path / "device", replicates=40, seed=4, keep_trees=True, engine=engine)
    assert [p.name for p in host] == [p.name for p in device] and len(host) == 3
    for a, b in zip(host, device):
        assert a.read_bytes() == b.read_bytes()
    supports = [int(line.split("\t")[3]) for line in host[1].read_text().split("\n")[1:-1]]
    assert len(supports) == 6 and min(supports) < 40
