"""ordinate-run without a GPU: the host twins of the tall product and of the centring against the numpy restatement of
the contract (tests/pcoa_cases.py) bit for bit, the eigen-solver against ``numpy.linalg.eigh``, its certificate, shift,
iteration limit and sign rule, ``ordination.pcoa``, and ``rundb.ordinate_run`` with its command line on the fixture
sets' finished runs."""

from __future__ import annotations

import re
import shutil
import sqlite3

import numpy as np
import pytest

from pyani_plus_amd import ordination, rundb
from pyani_plus_amd._capi import PA_E_INVALID, PA_E_NOCONVERGE, HipBackendError
from pyani_plus_amd.engine import gower_center_host, mul_tall_host, symm_top_eigs_host
from tests import pcoa_cases as pc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN, distance_check_cases, distance_refusal


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ the product twin
def test_the_sizes_cover_the_chunking():
    k = pc.kernel_constants()["kChunk"]
    assert k & (k - 1) == 0, "kChunk is a power of two"
    assert {1, 2, 63, 64, 65, k - 1, k, k + 1, 2 * k + 1} == set(pc.product_sizes())
    assert pc.PRODUCT_WIDTHS == (1, 2, 3, 11, 17, 32)


@pytest.mark.parametrize("p", pc.PRODUCT_WIDTHS)
@pytest.mark.parametrize("n", pc.product_sizes())
def test_product_twin_equals_the_restatement(n, p):
    A, Q = pc.product_input(n, p)
    got = mul_tall_host(A, Q, 1)
    assert got.shape == (n, p) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(pc.product_restated(n, p)))
    assert np.array_equal(bits(mul_tall_host(A, Q, 5)), bits(got)), "the number of threads shows in the result"


def test_the_product_input_shows_the_order_of_the_additions():
    k = pc.kernel_constants()["kChunk"]
    n = 2 * k + 1
    A, Q = pc.product_input(n, 11)
    assert not np.array_equal(bits(pc.mul_tall(A, Q, k // 2)), bits(pc.product_restated(n, 11)))


def test_product_refusals():
    A, Q = pc.product_input(3, 2)
    with pytest.raises(HipBackendError, match="33 columns") as err:
        mul_tall_host(np.zeros((40, 40)), np.zeros((40, 33)))
    assert err.value.status == PA_E_INVALID
    with pytest.raises(HipBackendError, match="0 rows"):
        mul_tall_host(np.zeros((0, 0)), np.zeros((0, 1)))
    with pytest.raises(ValueError, match="square"):
        mul_tall_host(np.zeros((3, 4)), Q)
    with pytest.raises(ValueError, match="block of shape"):
        mul_tall_host(A, np.zeros((4, 2)))


# ------------------------------------------------------------------ the centring twin
@pytest.mark.parametrize("n", pc.CENTRING_SIZES)
def test_centring_twin_equals_the_restatement(n):
    D = pc.random_distances(n, 300 + n)
    before = D.copy()
    B, trace, fro2 = gower_center_host(D, 3)
    want = pc.gower_center(D)
    assert np.array_equal(bits(D), bits(before)), "the matrix was modified"
    assert np.array_equal(bits(B), bits(want.B))
    assert np.array_equal(bits(B), bits(B.T)), "B is not bitwise symmetric"
    assert bits(trace) == bits(want.trace) and bits(fro2) == bits(want.fro2)
    B1, trace1, fro21 = gower_center_host(D, 1)
    assert np.array_equal(bits(B1), bits(B)) and bits(trace1) == bits(trace) and bits(fro21) == bits(fro2)


@pytest.mark.parametrize("what,D,cell", pc.invalid_matrices(), ids=[w for w, _, _ in pc.invalid_matrices()])
def test_centring_refuses_and_names_the_cell(what, D, cell):
    with pytest.raises(HipBackendError, match=rf"pa_gower_center_host: D\[{cell[0]},{cell[1]}\]") as err:
        gower_center_host(D)
    assert err.value.status == PA_E_INVALID
    good = pc.random_distances(3, 1)
    assert np.array_equal(bits(gower_center_host(good)[0]), bits(pc.gower_center(good).B))  # a good call works afterwards


@pytest.mark.parametrize("name,D,cell,count", distance_check_cases(), ids=[c[0] for c in distance_check_cases()])
def test_centring_names_the_first_cell_and_counts_them_all(name, D, cell, count):
    with pytest.raises(HipBackendError) as err:
        gower_center_host(D)
    assert err.value.status == PA_E_INVALID and str(err.value).endswith(distance_refusal("pa_gower_center_host", "D", cell, count))


# ------------------------------------------------------------------ the solver
def test_start_block_is_the_stated_mix():
    values = pc.start_block(7, 3)
    assert (np.abs(values) < 1).all() and len(np.unique(values)) == 21
    assert values[0, 0] == pc.start_value(0) and values[6, 2] == pc.start_value(6 * 3 + 2)
    # the header states the same mix: its three constants and three shifts, in this order
    text = (pc.ROOT / "pyani_plus_amd" / "csrc" / "pcoa_rule.h").read_text()
    body = text[text.index("double start_value(uint64_t index)") :]
    body = body[: body.index("}")]
    constants = [int(x, 16) for x in re.findall(r"0x([0-9A-F]{16})ULL", body)]
    assert constants == [0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB]
    assert [int(x) for x in re.findall(r"z >> (\d+)", body)] == [30, 27, 31, 12] and "0x1p-51" in body


def solve(name: str, k: int, **kwargs):
    c = pc.case(name)
    return symm_top_eigs_host(c.B, k, c.fro2, **kwargs)


def check_against_eigh(name: str, k: int, result) -> None:
    values, vectors, residuals, info = result
    scale = pc.spectral_scale(name)
    want = pc.eigh_top(name, k)
    errors = np.abs(values - want)
    print(f"{name} k={k}: info {info}, eigenvalue error / max|lambda| {errors.max() / max(scale, 1e-300):.3e}, "
          f"residual / max|lambda| {residuals.max() / max(scale, 1e-300):.3e}")
    assert values.shape == (k,) and vectors.shape == (len(pc.case(name).B), k) and residuals.shape == (k,)
    assert (np.diff(values) <= 0).all(), "not descending"
    assert (errors <= 1e-9 * scale).all()
    assert (residuals <= pc.TOL * scale).all()
    assert pc.sign_rule_holds(vectors)
    # the reported residuals are the pairs' own
    B = pc.case(name).B
    true = np.linalg.norm(B @ vectors - vectors * values[None, :], axis=0)
    assert (np.abs(true - residuals) <= 1e-12 * max(scale, 1.0)).all()
    assert 1 <= info[0] <= min(info[1], pc.PHASE1_CAP)


@pytest.mark.parametrize("name,k", pc.SOLVES, ids=[f"{n}-k{k}" for n, k in pc.SOLVES])
def test_solver_against_eigh(name, k):
    check_against_eigh(name, k, solve(name, k))


def test_euclidean_points_come_back():
    c = pc.case("euclid130x4")
    values, vectors, _residuals, info = solve("euclid130x4", 4)
    assert (values > 0).all()
    assert info[2] == 0.0  # four positive eigenvalues and nothing else: certified without a shift
    result = ordination.pcoa(c.D, 4)
    assert np.array_equal(bits(result.eigenvalues), bits(values))
    again = pc.pairwise(result.coordinates)  # rotation-free: equal eigenvalues cannot break it
    assert np.abs(again - c.D).max() <= 1e-8 * c.D.max()
    assert abs(result.proportions.sum() - 1.0) <= 1e-9  # the four axes carry the whole trace


def test_clustered_matrix_is_certified_with_three_axes_and_shifted_with_two():
    _v, _x, _r, info3 = solve("ani800", 3)
    assert info3[2] == 0.0 and info3[0] == info3[1] < pc.PHASE1_CAP
    _v, _x, _r, info2 = solve("ani800", 2)
    assert info2[2] > 0.0 and info2[1] > info2[0]
    top = pc.eigh_top("ani800", 3)
    assert top[2] > 0.9 * top[1], "the case no longer has a third eigenvalue comparable to the second"


def test_noise_reaches_the_cap_of_phase_one():
    _v, _x, _r, info = solve("noise400", 3)
    assert info[0] == pc.PHASE1_CAP and info[1] > pc.PHASE1_CAP and info[2] > 0.0


def test_adversarial_spectrum_returns_no_negative_eigenvalue():
    values, _x, _r, info = solve("adversarial300", 4)
    assert abs(values[3] - 1.0) <= 1e-9 * pc.spectral_scale("adversarial300") and values[3] > 0
    assert info[2] > 5.0  # the shift covers the thirty eigenvalues near -5.5


def test_iteration_limit_is_a_failure_of_its_own():
    with pytest.raises(HipBackendError, match=r"no convergence in 3 iterations.*worst residual of the first 3 pairs is [0-9.e+-]+") as err:
        solve("noise400", 3, max_iter=3)
    assert err.value.status == PA_E_NOCONVERGE
    check_against_eigh("two", 2, solve("two", 2))  # a good call works afterwards


def test_solver_refusals():
    B = pc.case("random9").B
    for k in (0, 10, 25):
        with pytest.raises(HipBackendError, match="eigenpairs") as err:
            symm_top_eigs_host(np.zeros((30, 30)) if k == 25 else B, k, 1.0)
        assert err.value.status == PA_E_INVALID
    with pytest.raises(HipBackendError, match="tolerance"):
        symm_top_eigs_host(B, 2, 1.0, tol=0.0)
    with pytest.raises(HipBackendError, match="not finite"):
        symm_top_eigs_host(np.full((4, 4), np.nan), 2, 1.0)


def test_threads_do_not_show_in_the_solver():
    c = pc.case("ani800")
    one = symm_top_eigs_host(c.B, 3, c.fro2, threads=1)
    five = symm_top_eigs_host(c.B, 3, c.fro2, threads=5)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(one[:3], five[:3])) and one[3] == five[3]


# ------------------------------------------------------------------ ordination.pcoa
def test_pcoa_small_and_refusals():
    one = ordination.pcoa(np.zeros((1, 1)), 1)
    assert one.coordinates.shape == (1, 1) and one.coordinates[0, 0] == 0.0 and not (one.eigenvalues > 0).any()
    assert one.proportions[0] == 0.0
    two = ordination.pcoa(np.array([[0.0, 0.5], [0.5, 0.0]]), 2)
    assert abs(two.eigenvalues[0] - 0.125) <= 1e-15 and abs(abs(two.coordinates[0, 0]) - 0.25) <= 1e-15
    assert (two.coordinates[:, 1] == 0.0).all()  # the second eigenvalue is 0 (to rounding): zeros, never a NaN
    with pytest.raises(ValueError, match="3 dimensions for 2 genomes"):
        ordination.pcoa(np.zeros((2, 2)), 3)
    with pytest.raises(ValueError, match="square"):
        ordination.pcoa(np.zeros((2, 3)))
    # negative eigenvalues count in the trace: the proportions of the positive axes are upper bounds
    D = pc.case("noise400").D
    full = np.linalg.eigvalsh(pc.case("noise400").B)
    res = ordination.pcoa(D, 3)
    assert full.min() < 0 and abs(res.trace - full.sum()) <= 1e-9 * np.abs(full).sum()
    assert (res.proportions >= res.eigenvalues / full[full > 0].sum()).all()


# ------------------------------------------------------------------ rundb.ordinate_run
@pytest.fixture(scope="module")
def run_dbs(tmp_path_factory):
    out = {}
    for name, (scaled, _genomes) in FIXTURE_SETS.items():
        tmp = tmp_path_factory.mktemp(f"ordinate_{name}")
        db = tmp / "run.sqlite"
        run = rundb.run_sourmash_hip(GOLDEN / name, db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp)
        assert run.status == "Done"
        out[name] = db
    return out


def read_table(path) -> tuple[list[str], list[list[str]]]:
    lines = path.read_text().split("\n")
    assert lines[-1] == ""
    return lines[0].split("\t"), [x.split("\t") for x in lines[1:-1]]


@pytest.mark.parametrize("name", list(FIXTURE_SETS))
def test_ordinate_run_tables(run_dbs, tmp_path, name):
    n = len(FIXTURE_SETS[name][1])
    k = min(2, n)
    stems = sorted(rundb.filename_stem(f) for f in FIXTURE_SETS[name][1].values())
    written = rundb.ordinate_run(run_dbs[name], tmp_path / "out", dimensions=k)
    assert written == [tmp_path / "out" / "sourmash-hip_identity_pcoa.tsv", tmp_path / "out" / "sourmash-hip_identity_pcoa_eigenvalues.tsv"]
    header, rows = read_table(written[0])
    assert header == ["genome"] + [f"PC{c + 1}" for c in range(k)]
    assert [r[0] for r in rows] == stems
    coordinates = np.array([[float(x) for x in r[1:]] for r in rows])
    assert all(repr(float(x)) == x for r in rows for x in r[1:])  # the values round-trip
    header, rows = read_table(written[1])
    assert header == ["component", "eigenvalue", "proportion_of_trace", "cumulative", "residual"]
    assert [r[0] for r in rows] == [f"PC{c + 1}" for c in range(k)]
    values, shares, cumulative = (np.array([float(r[c]) for r in rows]) for c in (1, 2, 3))
    running = 0.0
    for share, total in zip(shares.tolist(), cumulative.tolist()):
        running = running + share
        assert total == running
    assert (np.diff(values) <= 0).all() and values[0] > 0
    # the coordinates are the eigenvectors scaled: a column's squared norm is its eigenvalue
    for c in range(k):
        if values[c] > 0:
            assert abs((coordinates[:, c] ** 2).sum() - values[c]) <= 1e-12 * values[0]
    by_md5 = rundb.ordinate_run(run_dbs[name], tmp_path / "md5", dimensions=k, label="md5")
    assert [r[0] for r in read_table(by_md5[0])[1]] == sorted(FIXTURE_SETS[name][1])


def test_ordinate_run_command_line_and_figure(run_dbs, tmp_path, capsys):
    db = run_dbs["bacterial_example"]
    host = rundb.ordinate_run(db, tmp_path / "api")
    assert rundb.main(["ordinate-run", "-d", str(db), "-o", str(tmp_path / "cli"), "--formats", "tsv,png"]) == 0
    printed = capsys.readouterr().out.split()
    stem = tmp_path / "cli" / "sourmash-hip_identity_pcoa"
    assert printed == [f"{stem}.tsv", f"{stem}_eigenvalues.tsv", f"{stem}.png"]
    assert [p.read_bytes() for p in host] == [(tmp_path / "cli" / p.name).read_bytes() for p in host]
    assert (tmp_path / "cli" / "sourmash-hip_identity_pcoa.png").read_bytes().startswith(b"\x89PNG")
    one_axis = rundb.ordinate_run(db, tmp_path / "one", dimensions=1, formats=("png",))
    assert [p.name for p in one_axis] == ["sourmash-hip_identity_pcoa.png"] and one_axis[0].stat().st_size > 0


def test_ordinate_run_with_pairs_that_have_no_identity(run_dbs, tmp_path, caplog):
    """A fastANI-style run: some pairs have no identity in either direction."""
    db = tmp_path / "sparse.sqlite"
    shutil.copy(run_dbs["bacterial_example"], db)
    a, b = sorted(FIXTURE_SETS["bacterial_example"][1])[:2]
    with sqlite3.connect(db) as conn:
        conn.execute("UPDATE comparisons SET identity=NULL WHERE (query_hash=? AND subject_hash=?) OR (query_hash=? AND subject_hash=?)", (a, b, b, a))
        conn.execute("UPDATE runs SET df_identity=NULL, df_cov_query=NULL, df_aln_length=NULL, df_sim_errors=NULL, df_hadamard=NULL")
    conn.close()
    assert rundb.main(["ordinate-run", "-d", str(db), "-o", str(tmp_path / "half"), "--missing", "0.5", "--dimensions", "2", "--label", "md5"]) == 0
    assert "1 of 6 genome pairs have no identity in either direction" in caplog.text
    half = read_table(tmp_path / "half" / "sourmash-hip_identity_pcoa.tsv")[1]
    rundb.ordinate_run(db, tmp_path / "one", missing=1.0, dimensions=2, label="md5")
    one = read_table(tmp_path / "one" / "sourmash-hip_identity_pcoa.tsv")[1]
    assert [r[0] for r in half] == [r[0] for r in one] and half != one  # the distance of the missing pair shows


def test_ordinate_run_messages(run_dbs, tmp_path):
    db = run_dbs["viral_example"]
    with pytest.raises(SystemExit, match=f"Database {tmp_path / 'none.sqlite'} does not exist"):
        rundb.ordinate_run(tmp_path / "none.sqlite", tmp_path)
    with pytest.raises(SystemExit, match="Unexpected label scheme 'name'"):
        rundb.ordinate_run(db, tmp_path, label="name")
    with pytest.raises(SystemExit, match="must be finite and not negative"):
        rundb.ordinate_run(db, tmp_path, missing=-1.0)
    with pytest.raises(SystemExit, match="4 dimensions for 3 genomes"):
        rundb.ordinate_run(db, tmp_path, dimensions=4)
    with pytest.raises(SystemExit, match="Expected 1 to 24 dimensions"):
        rundb.ordinate_run(db, tmp_path, dimensions=0)
    with pytest.raises(SystemExit):
        rundb.main(["ordinate-run", "-d", str(db), "-o", str(tmp_path), "--label", "name"])
    with sqlite3.connect(db) as conn:
        stems = [rundb.filename_stem(r[0]) for r in conn.execute("SELECT fasta_filename FROM runs_genomes")]
    assert len(set(stems)) == len(stems)
    assert not list(tmp_path.glob("*.tsv"))


def test_ordinate_run_refuses_what_tree_run_refuses(run_dbs, tmp_path):
    """An incomplete run and an identity above 1, with tree-run's messages."""
    db = tmp_path / "partial.sqlite"
    shutil.copy(run_dbs["viral_example"], db)
    with sqlite3.connect(db) as conn:
        conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.close()
    for call in (rundb.ordinate_run, rundb.tree_run):
        with pytest.raises(SystemExit, match=r"has 8 of 3\^2=9 comparisons, 1 needed"):
            call(db, tmp_path)
    above = tmp_path / "above.sqlite"
    shutil.copy(run_dbs["viral_example"], above)
    with sqlite3.connect(above) as conn:
        conn.execute("UPDATE comparisons SET identity=1.25 WHERE query_hash != subject_hash")
        conn.execute("UPDATE runs SET df_identity=NULL, df_cov_query=NULL, df_aln_length=NULL, df_sim_errors=NULL, df_hadamard=NULL")
    conn.close()
    with pytest.raises(SystemExit, match="An identity above 1 gives a negative distance: no ordination is defined"):
        rundb.ordinate_run(above, tmp_path)
    with pytest.raises(SystemExit, match="An identity above 1 gives a negative distance: no tree is defined"):
        rundb.tree_run(above, tmp_path)
