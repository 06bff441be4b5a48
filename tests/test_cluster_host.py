"""plot-run without a GPU: the host row distances against a numpy restatement (and scipy's ``pdist`` where scipy is
installed), ``pa_linkage_average`` against scipy's ``linkage`` / ``dendrogram`` and against the golden leaves, the heatmap
tables of the viral fixture byte for byte, and ``rundb.plot_run`` end to end with its messages."""

from __future__ import annotations

import logging
import sqlite3
import sys
from io import StringIO

import numpy as np
import pytest

from pyani_plus_amd import cluster, rundb
from pyani_plus_amd._capi import HipBackendError
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN
from tests.plot_run_cases import case_matrix, distance_inputs, filled, load_cases, matrix_md5, numpy_distances, same_bits

CASES = load_cases()
PLOTS = GOLDEN / "viral_example" / "plots"
HEATMAP_SCORES = (("identity", 0), ("query_cov", 0), ("hadamard", 0), ("tANI", -5))
PLOT_NAMES = sorted(
    [f"sourmash-hip_{s}_heatmap.tsv" for s, _ in HEATMAP_SCORES] + [f"sourmash-hip_{s}_scatter.tsv" for s in ("query_cov", "tANI")]
)


# ------------------------------------------------------------------ distances
@pytest.mark.parametrize("shape", [(2, 2), (3, 3), (9, 1), (64, 64), (65, 65), (130, 257), (257, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_distances_equal_the_numpy_restatement(shape):
    for name, x in distance_inputs(*shape):
        got = cluster.row_distances(x)
        same_bits(got, numpy_distances(x))
        same_bits(cluster.row_distances(x, threads=1), got)
        if name == "duplicated":
            assert got[0] == 0.0 and not np.signbit(got[0])  # rows 0 and 1 are equal: +0.0


@pytest.mark.parametrize("n", (7, 8, 9, 17))
def test_host_distances_around_the_eight_pairs_side_by_side(n):
    """A row's pairs run eight at a time: fewer than eight, exactly eight, one more, and two groups and one, with one
    column, sixteen and seventeen."""
    for m in (1, 16, 17):
        for _name, x in distance_inputs(n, m):
            got = cluster.row_distances(x)
            same_bits(got, numpy_distances(x))
            same_bits(cluster.row_distances(x, threads=1), got)


def test_host_distances_small_inputs_and_arguments():
    assert cluster.row_distances(np.zeros((0, 4))).shape == (0,)
    assert cluster.row_distances(np.zeros((1, 4))).shape == (0,)
    same_bits(cluster.row_distances(np.ones((3, 0))), np.zeros(3))
    with pytest.raises(ValueError, match="two dimensions"):
        cluster.row_distances(np.zeros(5))
    with pytest.raises(ValueError, match="condensed distances for 4 observations"):
        cluster.linkage_average(np.zeros(5), 4)
    with pytest.raises(ValueError, match="infinite"):
        cluster.cluster_order(np.array([[0.0, np.inf], [1.0, 0.0]]), 0)
    with pytest.raises(ValueError, match="65537 rows; at most 65536"):
        cluster.row_distances(np.zeros((65537, 0)))
    # finite cells do not make finite distances: 1e200 squared overflows, and the linkage refuses the result
    far = cluster.row_distances(np.array([[0.0, 0.0], [1e200, 0.0], [0.0, 1.0]]))
    assert np.isinf(far[0]) and far[1] == 1.0
    for bad in (far, np.array([1.0, np.nan, 2.0])):
        with pytest.raises(HipBackendError, match="pa_linkage_average: distance . of 3 is not finite") as caught:
            cluster.linkage_average(bad, 3)
        assert caught.value.status == -1  # PA_E_INVALID
    with pytest.raises(HipBackendError, match="a merged distance is not finite"):
        cluster.linkage_average(np.array([1e-300, 1.7e308, 1.7e308, 1.7e308, 1.7e308, 1e-300]), 4)


@pytest.mark.parametrize("shape", [(3, 3), (40, 40), (97, 64), (130, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_distances_and_linkage_equal_scipy(shape):
    pytest.importorskip("scipy")
    from scipy.cluster.hierarchy import dendrogram, linkage
    from scipy.spatial.distance import pdist

    for _name, x in distance_inputs(*shape):
        d = cluster.row_distances(x)
        same_bits(d, pdist(x, "euclidean"))
        z, leaves = cluster.linkage_average(d, len(x))
        want = linkage(x, method="average", metric="euclidean")
        same_bits(z, want)  # all four columns as bit patterns
        assert leaves.tolist() == dendrogram(want, no_plot=True)["leaves"]


def test_linkage_does_not_touch_its_input():
    x = next(iter(distance_inputs(20, 7)))[1]
    d = cluster.row_distances(x)
    before = d.copy()
    cluster.linkage_average(d, 20)
    same_bits(d, before)


# ------------------------------------------------------------------ golden leaves
def test_the_golden_file_covers_what_it_should():
    assert {c["synth"]["n"] for c in CASES} == {2, 3, 63, 64, 65, 130, 257, 1000}
    assert max(c["tied"] for c in CASES) > 1000 and any(c["tied"] == 0 for c in CASES)
    assert {c["na_fill"] for c in CASES if c["synth"].get("nan_frac")} == {0, -5}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_gives_the_leaves_of_scipy(case):
    assert matrix_md5(case_matrix(case)) == case["md5"], "the generator drifted"
    x = filled(case)
    z, leaves = cluster.linkage_average(cluster.row_distances(x), len(x))
    assert leaves.tolist() == case["leaves"]
    n = len(x)
    assert z.shape == (n - 1, 4) and z[-1, 3] == n and np.all(np.diff(z[:, 2]) >= 0)
    assert np.array_equal(cluster.cluster_order(case_matrix(case), case["na_fill"]), leaves)


def test_one_and_two_observations():
    z, leaves = cluster.linkage_average(np.empty(0), 1)
    assert z.shape == (0, 4) and leaves.tolist() == [0]
    assert cluster.cluster_order(np.array([[1.0]]), 0).tolist() == [0]
    z, leaves = cluster.linkage_average(np.array([0.25]), 2)
    assert z.tolist() == [[0.0, 1.0, 0.25, 2.0]] and leaves.tolist() == [0, 1]
    z, leaves = cluster.linkage_average(np.empty(0), 0)
    assert z.shape == (0, 4) and leaves.shape == (0,)


# ------------------------------------------------------------------ heatmap tables
def read_table(path):
    import pandas as pd

    # the round-trip parser: the default one reads 0.9962077560000001 as 0.996207756
    return pd.read_csv(path, sep="\t", index_col=0, float_precision="round_trip")


@pytest.mark.parametrize(("score", "na_fill"), HEATMAP_SCORES)
def test_heatmap_table_of_the_viral_export(score, na_fill, tmp_path):
    frame = read_table(GOLDEN / "viral_example" / "export" / f"sourmash_{score}.tsv")
    assert list(frame.index) == sorted(frame.index) and list(frame.columns) == list(frame.index)
    out = tmp_path / "table.tsv"
    cluster.heatmap_table(frame, na_fill).to_csv(out, sep="\t")
    assert out.read_bytes() == (PLOTS / f"sourmash_{score}_heatmap.tsv").read_bytes()


def test_heatmap_table_keeps_the_nans():
    import pandas as pd

    x = case_matrix(next(c for c in CASES if c["name"] == "nan-fill-5-n65"))
    labels = [f"g{i:02d}" for i in range(len(x))]
    table = cluster.heatmap_table(pd.DataFrame(x, index=labels, columns=labels), -5)
    assert int(table.isna().to_numpy().sum()) == int(np.isnan(x).sum()) > 0
    assert list(table.index) == list(table.columns) and sorted(table.index) == labels


# ------------------------------------------------------------------ rundb.plot_run
@pytest.fixture(scope="module")
def viral_db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plot_run_db")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp)
    assert run.status == "Done"
    return db


def check_against_the_fixtures(outdir) -> None:
    for score, _fill in HEATMAP_SCORES:
        assert (outdir / f"sourmash-hip_{score}_heatmap.tsv").read_bytes() == (PLOTS / f"sourmash_{score}_heatmap.tsv").read_bytes(), score
    for score in ("query_cov", "tANI"):  # the reference's own test compares these as sorted lines
        got = (outdir / f"sourmash-hip_{score}_scatter.tsv").read_text().split("\n")
        assert sorted(got) == sorted((PLOTS / f"sourmash_{score}_scatter.tsv").read_text().split("\n")), score


def test_plot_run_writes_the_tables(viral_db, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    written = rundb.plot_run(viral_db, tmp_path / "out")
    assert sorted(p.name for p in written) == PLOT_NAMES and all(p.parent == tmp_path / "out" for p in written)
    assert "does not exist, making it." in caplog.text and "Plotting 9/9 tANI vs identity sourmash-hip comparisons" in caplog.text
    assert f"Wrote 6 images to {tmp_path / 'out'}/sourmash-hip_*.*" in caplog.text
    check_against_the_fixtures(tmp_path / "out")
    # the four tables of one run are clustered each on its own: the viral fixture's identity table has another order
    orders = {score: read_table(tmp_path / "out" / f"sourmash-hip_{score}_heatmap.tsv").index.tolist() for score, _ in HEATMAP_SCORES}
    assert orders["identity"] != orders["hadamard"] and sorted(orders["identity"]) == sorted(orders["hadamard"])
    # other labels, and the command line form
    by_md5 = rundb.plot_run(viral_db, tmp_path / "md5", label="md5")
    assert sorted(read_table(by_md5[-1]).index) == sorted(FIXTURE_SETS["viral_example"][1])
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli")]) == 0
    check_against_the_fixtures(tmp_path / "cli")


def test_plot_run_messages(viral_db, tmp_path, monkeypatch):
    with pytest.raises(SystemExit, match=f"Database {tmp_path / 'none.sqlite'} does not exist"):
        rundb.plot_run(tmp_path / "none.sqlite", tmp_path)
    with pytest.raises(SystemExit, match="Unexpected label scheme 'name'"):
        rundb.plot_run(viral_db, tmp_path, label="name")
    with pytest.raises(SystemExit, match="has no run-id 7"):
        rundb.plot_run(viral_db, tmp_path, run_id=7)
    with monkeypatch.context() as patch:
        patch.setitem(sys.modules, "matplotlib", None)  # ``import matplotlib`` raises ImportError
        with pytest.raises(SystemExit, match=r"Image formats \(png\) need matplotlib, which cannot be imported"):
            rundb.plot_run(viral_db, tmp_path, formats=("tsv", "png"))
        assert len(rundb.plot_run(viral_db, tmp_path / "tables_only")) == 6
    copy = tmp_path / "copy.sqlite"
    copy.write_bytes(viral_db.read_bytes())
    conn = sqlite3.connect(copy)
    conn.execute("UPDATE runs_genomes SET fasta_filename = 'OP073605.fna' WHERE fasta_filename = 'MGV-GENOME-0264574.fas'")
    conn.commit()
    with pytest.raises(SystemExit, match="Duplicate filename stems, consider using MD5 labelling."):
        rundb.plot_run(copy, tmp_path)
    assert len(rundb.plot_run(copy, tmp_path / "dup", label="md5")) == 6
    conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.commit()
    conn.close()
    with pytest.raises(SystemExit, match=r"run-id 1 has 8 of 3\^2=9 comparisons, 1 needed"):
        rundb.plot_run(copy, tmp_path, label="md5")


def test_plot_run_single_genome(tmp_path):
    fasta = tmp_path / "one"
    fasta.mkdir()
    (fasta / "OP073605.fasta").write_bytes((GOLDEN / "viral_example" / "OP073605.fasta").read_bytes())
    db = tmp_path / "one.sqlite"
    assert rundb.run_sourmash_hip(fasta, db, cache=tmp_path / "cache", scaled=300, engine=OracleEngine(), temp=tmp_path).status == "Done"
    written = rundb.plot_run(db, tmp_path / "out")
    assert (tmp_path / "out" / "sourmash-hip_tANI_heatmap.tsv").read_text() == "\tOP073605\nOP073605\t-0.0\n"
    assert len(written) == 6


def test_plot_run_figures(viral_db, tmp_path):
    pytest.importorskip("matplotlib")
    written = rundb.plot_run(viral_db, tmp_path / "out", formats=("tsv", "png"))
    pngs = [p for p in written if p.suffix == ".png"]
    assert sorted(p.name for p in pngs) == sorted(f"sourmash-hip_{s}_heatmap.png" for s, _ in HEATMAP_SCORES)
    assert all(p.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and p.stat().st_size > 1000 for p in pngs)
    check_against_the_fixtures(tmp_path / "out")
    assert rundb.main(["plot-run", "-d", str(viral_db), "-o", str(tmp_path / "cli"), "--formats", "tsv,png"]) == 0
    assert len(list((tmp_path / "cli").glob("*.png"))) == 4


def test_plot_run_with_null_comparisons(viral_db, tmp_path, caplog):
    """Comparisons without a result, as fastANI leaves them: the nulls warning, the scatter tables without those rows,
    and a clustering all the same; with every comparison NULL nothing can be plotted."""
    import pandas as pd

    copy = tmp_path / "nulls.sqlite"
    copy.write_bytes(viral_db.read_bytes())
    conn = sqlite3.connect(copy)
    ids = [r[0] for r in conn.execute("SELECT comparison_id FROM comparisons WHERE query_hash != subject_hash ORDER BY comparison_id LIMIT 2")]
    conn.execute(f"UPDATE comparisons SET identity = NULL, cov_query = NULL WHERE comparison_id IN ({ids[0]}, {ids[1]})")
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")  # rebuilt from the table
    conn.commit()
    caplog.set_level(logging.INFO)
    written = rundb.plot_run(copy, tmp_path / "out")
    assert sorted(p.name for p in written) == PLOT_NAMES
    for name in ("identity", "query_cov", "hadamard", "tANI"):
        assert f"{name} matrix contains 2 nulls (out of 3²=9 sourmash-hip comparisons)" in caplog.text
    assert "Plotting 7/9 Query coverage vs identity sourmash-hip comparisons" in caplog.text
    assert len((tmp_path / "out" / "sourmash-hip_tANI_scatter.tsv").read_text().split("\n")) == 1 + 7 + 1
    table = pd.read_csv(StringIO((tmp_path / "out" / "sourmash-hip_tANI_heatmap.tsv").read_text()), sep="\t", index_col=0)
    assert int(table.isna().to_numpy().sum()) == 2 and sorted(table.index) == sorted(table.columns)
    # the order is that of the matrix with its nulls counted as -5
    frame = table.sort_index(axis=0).sort_index(axis=1)
    assert list(frame.index[cluster.cluster_order(frame.to_numpy(dtype=float), -5)]) == list(table.index)
    conn.execute("UPDATE comparisons SET identity = NULL, cov_query = NULL")
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.commit()
    conn.close()
    caplog.clear()
    assert rundb.plot_run(copy, tmp_path / "none") == []
    assert "No valid identity, Query coverage values from sourmash-hip run" in caplog.text and "Cannot plot tANI as all NA" in caplog.text


def test_plot_run_of_a_fixture_run_with_null_comparisons(tmp_path, caplog):
    """The bad_alignments fixture set: its two genomes share nothing, both comparisons between them are NULL."""
    scaled, _genomes = FIXTURE_SETS["bad_alignments"]
    db = tmp_path / "bad.sqlite"
    assert rundb.run_sourmash_hip(GOLDEN / "bad_alignments", db, cache=tmp_path / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp_path).status == "Done"
    written = rundb.plot_run(db, tmp_path / "out")
    assert sorted(p.name for p in written) == PLOT_NAMES
    assert "identity matrix contains 2 nulls (out of 2²=4 sourmash-hip comparisons)" in caplog.text
    assert (tmp_path / "out" / "sourmash-hip_identity_heatmap.tsv").read_text() == (
        "\tMGV-GENOME-0264574\tMGV-GENOME-0357962\nMGV-GENOME-0264574\t1.0\t\nMGV-GENOME-0357962\t\t1.0\n"
    )
    assert (tmp_path / "out" / "sourmash-hip_tANI_heatmap.tsv").read_text().split("\n")[1] == "MGV-GENOME-0264574\t-0.0\t"


def test_scatter_table_with_a_zero_hadamard_product(viral_db, tmp_path, caplog):
    copy = tmp_path / "zero.sqlite"
    copy.write_bytes(viral_db.read_bytes())
    conn = sqlite3.connect(copy)
    conn.execute("UPDATE comparisons SET cov_query = 0.0 WHERE comparison_id = (SELECT MIN(comparison_id) FROM comparisons WHERE query_hash != subject_hash)")
    conn.execute("UPDATE runs SET df_identity = NULL, df_cov_query = NULL, df_hadamard = NULL")
    conn.commit()
    conn.close()
    rundb.plot_run(copy, tmp_path / "out")
    assert "1 sourmash-hip comparisons have a zero Hadamard product" in caplog.text
    assert sum(line.split("\t")[1] == "inf" for line in (tmp_path / "out" / "sourmash-hip_tANI_scatter.tsv").read_text().split("\n")[1:-1]) == 1
    assert "tANI matrix contains 1 nulls" in caplog.text
