"""classify without a GPU: the host edge list, the clique pass, the TSV and ``rundb.classify``.

Against the reference only where a comparison means something (tests/golden/classify/make_classify_golden.py): the
rows as a map from member set to values, on inputs without tied scores.  Row order, member order and the result on
tied scores are this project's definitions and are checked against a literal restatement written here."""

from __future__ import annotations

import logging
import math
import sqlite3
import sys
from pathlib import Path

import numpy as np
import pytest

from pyani_plus_amd import _capi, rundb
from pyani_plus_amd import classify as cl
from pyani_plus_amd.synth import synth_classify_matrices
from tests.classify_cases import base_matrices, load_cases, matrices_md5
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN

REFERENCE = Path("/root/reference")
CASES = load_cases()
AGGS = ("min", "max", "mean")


def case_input(case: dict):
    """(labels, score, cov) of a golden case, with the checks that the rebuilt input is the one the reference saw."""
    labels, ident, cov = base_matrices(case["source"])
    assert matrices_md5(ident, cov) == case["md5"], "the rebuilt matrices are not the ones of the golden case"
    score = ident if case["mode"] == "identity" else cl.tani_scores(ident * cov)
    # in tANI mode this pins pa_classify_tani_host to the reference's per-cell math.log, bit for bit
    assert matrices_md5(score) == case["score_md5"]
    return labels, score, cov


def as_map(rows) -> dict:
    out = {frozenset(r.members): (r.n_nodes, *(None if v is None else repr(float(v)) for v in (r.max_cov, r.min_score, r.max_score))) for r in rows}
    assert len(out) == len(rows), "a member set was recorded twice"
    return out


def check_our_order(rows) -> None:
    """Members ascending; a superset row before its subset rows."""
    sets = [set(r.members) for r in rows]
    for r in rows:
        assert r.members == sorted(r.members) and r.n_nodes == len(r.members)
    for a in range(len(rows)):
        for b in range(a + 1, len(rows)):
            assert not sets[a] < sets[b], (rows[a].members, rows[b].members)


def test_the_golden_file_covers_what_it_should():
    names = {c["name"] for c in CASES}
    assert len(names) == len(CASES) >= 40
    assert {c["source"]["synth"]["n"] for c in CASES if "synth" in c["source"]} >= {1, 2, 3, 16, 60, 200}
    assert {(c["coverage_edges"], c["score_edges"]) for c in CASES} >= {(a, b) for a in AGGS for b in AGGS}
    assert {c["cov_min"] for c in CASES} >= {0.0, 0.5, 1.0} and {c["mode"] for c in CASES} == {"identity", "tANI"}
    assert any(c["components"] > 1 and c["n_edges"] == 0 for c in CASES) and any(c["components"] > 1 and c["n_edges"] for c in CASES)
    fixtures = {(c["source"]["fixture"], c["source"]["method"], c["mode"]) for c in CASES if "fixture" in c["source"]}
    assert len(fixtures) == 10
    # the case made for it: the graph's lowest edge lies inside a component that is a clique from the start
    low = next(c for c in CASES if c["name"] == "synth-n24-lowest-edge-in-clique")
    assert low["components"] > 1
    top = [r for r in low["rows"] if r["raw"][0] > 1 and r["raw"][2] == r["raw"][3]]
    assert top, "no top-level clique whose own lowest edge is the lowest of the graph"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_equals_the_reference(case):
    labels, score, cov = case_input(case)
    kwargs = {"coverage_edges": case["coverage_edges"], "score_edges": case["score_edges"], "cov_min": case["cov_min"]}
    rows = cl.classify_matrices(labels, score, cov, engine=None, **kwargs)
    want = {frozenset(r["members"]): tuple(r["raw"]) for r in case["rows"]}
    assert as_map(rows) == want
    e_i, _e_j, _e_s, _e_c = cl.edges_host(score, cov, **kwargs)
    assert len(e_i) == case["n_edges"]
    check_our_order(rows)
    # the TSV: header, and field by field after sorting both by sorted members
    text = cl.classify_tsv(rows, case["mode"])
    lines = text.split("\n")
    assert lines[0] == case["header"] and lines[-1] == "" and len(lines) == len(rows) + 2
    got = sorted((sorted(f[4].split(",")), f[:4]) for f in (line.split("\t") for line in lines[1:-1]))
    assert got == [(r["members"], r["tsv"]) for r in case["rows"]]
    # in our order the members of a line are as listed in the row
    assert [line.split("\t")[4] for line in lines[1:-1]] == [",".join(r.members) for r in rows]
    # a second run gives the same bytes
    assert cl.classify_tsv(cl.classify_matrices(labels, score, cov, engine=None, **kwargs), case["mode"]) == text


# ------------------------------------------------------------------ the defined result on tied scores
def _py_agg(name: str, a: float, b: float) -> float:
    if name == "min":
        return min([a, b])
    if name == "max":
        return max([a, b])
    return float(np.mean([a, b]))


def _components(nodes: set, edges: list) -> list[set]:
    adj = {v: set() for v in nodes}
    for _s, i, j, _c in edges:
        adj[i].add(j)
        adj[j].add(i)
    seen, out = set(), []
    for v in sorted(nodes):
        if v in seen:
            continue
        comp, todo = {v}, [v]
        while todo:
            for y in adj[todo.pop()]:
                if y not in comp:
                    comp.add(y)
                    todo.append(y)
        seen |= comp
        out.append(comp)
    return out


def brute_force(labels, score, cov, coverage_edges, score_edges, cov_min) -> dict:
    """The defined rule, literally: build the edges as the reference does, remove them one by one in (score, i, j)
    order, recompute the components after every removal, recurse into them when there are several."""
    n = len(labels)
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            c = _py_agg(coverage_edges, cov[j, i], cov[i, j])
            s = _py_agg(score_edges, score[j, i], score[i, j])
            if not math.isnan(c) and not math.isnan(s) and c > cov_min:
                edges.append((float(s), i, j, float(c)))
    out = {}

    def record(nodes, es, formed_by):
        if len(es) == len(nodes) * (len(nodes) - 1) // 2:
            key = frozenset(labels[k] for k in nodes)
            if key not in out:
                vals = (min((e[3] for e in es), default=None), formed_by, min((e[0] for e in es), default=None))
                out[key] = (len(nodes), *(None if v is None else repr(float(v)) for v in vals))

    def inside(es, comp):
        return [e for e in es if e[1] in comp and e[2] in comp]

    def recurse(nodes, es, formed_by):
        record(nodes, es, formed_by)
        if len(nodes) == 1:
            return
        es = sorted(es, key=lambda e: (e[0], e[1], e[2]))
        while es:
            formed_by = es.pop(0)[0]
            comps = _components(nodes, es)
            if len(comps) > 1:
                for comp in comps:
                    recurse(comp, inside(es, comp), formed_by)
                return

    everything = set(range(n))
    comps = _components(everything, edges)
    if len(comps) != 1:
        lowest = min((e[0] for e in edges), default=None)
        for comp in comps:
            record(comp, inside(edges, comp), lowest)
    recurse(everything, edges, None)
    return out


@pytest.mark.parametrize("n", [2, 3, 5, 8, 12])
@pytest.mark.parametrize("nan_frac", [0.0, 0.08])
def test_tied_scores_follow_the_defined_rule(n, nan_frac):
    for seed in range(12):
        labels, ident, cov = synth_classify_matrices(n, seed, groups=2, nan_frac=nan_frac, decimals=2)
        cov = np.round(cov, 1)
        # duplicate genomes: identity 1.0 in both directions with the genome before
        if n >= 3:
            ident[1, 0] = ident[0, 1] = 1.0
            cov[1, 0] = cov[0, 1] = 1.0
            ident[2:, 1], ident[1, 2:] = ident[2:, 0], ident[0, 2:]
        for ca, sa, cov_min in (("min", "mean", 0.5), ("max", "min", 0.5), ("mean", "max", 0.3)):
            rows = cl.classify_matrices(labels, ident, cov, coverage_edges=ca, score_edges=sa, cov_min=cov_min)
            assert as_map(rows) == brute_force(labels, ident, cov, ca, sa, cov_min), (seed, ca, sa)
            check_our_order(rows)


def test_tied_scores_in_tani_mode_with_both_zeros():
    """-0.0 and 0.0 are one score: the pairs holding them are removed in (i, j) order."""
    labels = ["a", "b", "c", "d"]
    score = np.full((4, 4), -0.5)
    score[0, 1] = score[1, 0] = 0.0
    score[2, 3] = score[3, 2] = -0.0
    score[0, 2] = score[2, 0] = -0.0
    score[1, 3] = score[3, 1] = 0.0
    cov = np.ones((4, 4))
    e_i, e_j, e_s, _e_c = cl.edges_host(score, cov, score_edges="min", coverage_edges="min", cov_min=0.5)
    assert list(zip(e_i.tolist(), e_j.tolist())) == [(0, 3), (1, 2), (0, 1), (0, 2), (1, 3), (2, 3)]
    assert [math.copysign(1.0, x) for x in e_s[2:]] == [1.0, -1.0, 1.0, -1.0]  # the values stay as computed
    rows = cl.classify_matrices(labels, score, cov, score_edges="min")
    assert as_map(rows) == brute_force(labels, score, cov, "min", "min", 0.5)


def test_min_and_max_keep_the_argument_order_of_the_reference():
    """min([nan, x]) is nan and min([x, nan]) is x: with [M[j,i], M[i,j]] a NaN below the diagonal removes the edge
    and a NaN above it is passed over; the mean is NaN for either."""
    nan = float("nan")
    upper = np.array([[1.0, nan], [0.9, 1.0]])  # M[i,j] is NaN
    lower = np.array([[1.0, 0.9], [nan, 1.0]])  # M[j,i] is NaN
    full = np.array([[1.0, 0.8], [0.9, 1.0]])
    for agg in ("min", "max"):
        assert [len(x) for x in cl.edges_host(upper, full, score_edges=agg)] == [1] * 4
        assert cl.edges_host(upper, full, score_edges=agg)[2].tolist() == [0.9]
        assert len(cl.edges_host(lower, full, score_edges=agg)[0]) == 0
        assert cl.edges_host(full, upper, coverage_edges=agg)[3].tolist() == [0.9]
        assert len(cl.edges_host(full, lower, coverage_edges=agg)[0]) == 0
    assert len(cl.edges_host(upper, full, score_edges="mean")[0]) == 0 and len(cl.edges_host(lower, full, score_edges="mean")[0]) == 0
    assert [x.tolist() for x in cl.edges_host(full, full, score_edges="min", coverage_edges="max", cov_min=0.0)[2:]] == [[0.8], [0.9]]
    assert cl.edges_host(full, full, score_edges="mean")[2].tolist() == [float(np.mean([0.9, 0.8]))]
    # the threshold is strict
    assert len(cl.edges_host(full, full, cov_min=0.8)[0]) == 0 and len(cl.edges_host(full, full, cov_min=0.7999)[0]) == 1
    rows = cl.classify_matrices(["a", "b"], lower, full, score_edges="min")
    assert [(r.n_nodes, r.max_cov, r.min_score, r.max_score, r.members) for r in rows] == [(1, None, None, None, ["a"]), (1, None, None, None, ["b"])]


def test_arguments_are_checked():
    full = np.ones((2, 2))
    with pytest.raises(ValueError, match="Unknown score aggregator 'median'"):
        cl.classify_matrices(["a", "b"], full, full, score_edges="median")
    with pytest.raises(ValueError, match="Unknown coverage aggregator"):
        cl.edges_host(full, full, coverage_edges="")
    with pytest.raises(ValueError, match="3 labels"):
        cl.classify_matrices(["a", "b", "c"], full, full)
    lib = _capi.load_library()
    count = _capi.C.c_uint64(0)
    assert lib.pa_classify_edges_host(full.ctypes.data, full.ctypes.data, 2, 7, 0, 0.5, 1, None, None, None, None, _capi.C.byref(count)) == -1
    assert b"aggregators" in lib.pa_last_error()
    # room for fewer edges than there are: the count comes back with PA_E_CAPACITY
    assert lib.pa_classify_edges_host(full.ctypes.data, full.ctypes.data, 2, 0, 0, 0.5, 0, None, None, None, None, _capi.C.byref(count)) == _capi.PA_E_CAPACITY
    assert count.value == 1
    # pa_classify_cliques wants the edges in removal order
    e_i, e_j = np.array([0, 0], dtype=np.uint32), np.array([1, 2], dtype=np.uint32)
    with pytest.raises(_capi.HipBackendError, match="lower score"):
        cl.cliques_from_edges(["a", "b", "c"], e_i, e_j, np.array([0.9, 0.8]), np.array([1.0, 1.0]))
    with pytest.raises(_capi.HipBackendError, match="of 2 nodes"):
        cl.cliques_from_edges(["a", "b"], e_i, e_j, np.array([0.8, 0.9]), np.array([1.0, 1.0]))


def test_row_order_on_a_small_example():
    """Two species and a singleton, separate from the start: the three top-level rows first, then each tree."""
    labels = ["a", "b", "c", "d", "e", "f"]
    score = np.full((6, 6), 0.5)
    cov = np.zeros((6, 6))
    for grp in ((0, 2, 4), (1, 3)):
        for x in grp:
            for y in grp:
                cov[x, y] = 0.9
    for (x, y), s in {(0, 2): 0.99, (0, 4): 0.95, (2, 4): 0.96, (1, 3): 0.97}.items():
        score[x, y] = score[y, x] = s
    rows = cl.classify_matrices(labels, score, cov)
    assert [(r.members, r.min_score, r.max_score) for r in rows] == [
        (["a", "c", "e"], 0.95, 0.95), (["b", "d"], 0.95, 0.97), (["f"], 0.95, None),
        (["a", "c"], 0.96, 0.99), (["a"], 0.99, None), (["c"], 0.99, None), (["e"], 0.96, None),
        (["b"], 0.97, None), (["d"], 0.97, None),
    ]  # fmt: skip
    assert cl.classify_tsv(rows).split("\n")[:2] == ["n_nodes\tmax_cov\tmin_identity\tmax_identity\tmembers", "3\t0.9\t0.95\t0.95\ta,c,e"]


# ------------------------------------------------------------------ rundb.classify
@pytest.fixture(scope="module")
def fixture_db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("classify_db")
    scaled, _genomes = FIXTURE_SETS["bacterial_example"]
    db = tmp / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "bacterial_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp)
    assert run.status == "Done"
    return db


def test_rundb_classify_writes_the_table(fixture_db, tmp_path, caplog):
    caplog.set_level(logging.INFO)
    out = rundb.classify(fixture_db, tmp_path / "out")
    assert out == tmp_path / "out" / "sourmash-hip_classify.tsv" and out.is_file()
    assert "does not exist, making it." in caplog.text and "Run 1 has 16 comparisons across 4 genomes." in caplog.text
    lines = out.read_text().split("\n")
    assert lines[0] == "n_nodes\tmax_cov\tmin_identity\tmax_identity\tmembers"
    # the same matrices as the golden case of this fixture set (the database holds them rounded to 10 decimals, the
    # TSV to 7: compare the structure and the rounded fields)
    case = next(c for c in CASES if c["name"] == "bacterial_example-sourmash-identity-cov0.5")
    got = sorted((sorted(f[4].split(",")), f[0]) for f in (line.split("\t") for line in lines[1:-1]))
    assert got == [(r["members"], r["tsv"][0]) for r in case["rows"]]
    tani = rundb.classify(fixture_db, tmp_path / "tani", mode="tANI", label="md5", cov_min=0.0, coverage_edges="max", score_edges="min")
    t_lines = tani.read_text().split("\n")
    assert t_lines[0] == "n_nodes\tmax_cov\tmin_-tANI\tmax_-tANI\tmembers"
    assert set(t_lines[1].split("\t")[4].split(",")) == set(FIXTURE_SETS["bacterial_example"][1])
    by_name = rundb.classify(fixture_db, tmp_path / "names", label="filename")
    assert by_name.read_text().split("\n")[1].split("\t")[4] == "NC_002696.fasta.gz,NC_010338.fna.gz,NC_011916.fas.gz,NC_014100.fna.gz"
    # the command line form
    assert rundb.main(["classify", "-d", str(fixture_db), "-o", str(tmp_path / "cli"), "--mode", "tANI", "--cov-min", "0.0", "--label", "md5",
                       "--coverage-edges", "max", "--score-edges", "min"]) == 0  # fmt: skip
    assert (tmp_path / "cli" / "sourmash-hip_classify.tsv").read_text() == tani.read_text()


def test_rundb_classify_messages(fixture_db, tmp_path):
    with pytest.raises(SystemExit, match=f"Database {tmp_path / 'none.sqlite'} does not exist"):
        rundb.classify(tmp_path / "none.sqlite", tmp_path)
    with pytest.raises(SystemExit, match="Unexpected label scheme 'name'"):
        rundb.classify(fixture_db, tmp_path, label="name")
    with pytest.raises(SystemExit, match="Unknown score aggregator 'median': expected one of min, max, mean"):
        rundb.classify(fixture_db, tmp_path, score_edges="median")
    with pytest.raises(SystemExit, match="Unknown coverage aggregator"):
        rundb.classify(fixture_db, tmp_path, coverage_edges="sum")
    with pytest.raises(SystemExit, match="Unknown classify mode"):
        rundb.classify(fixture_db, tmp_path, mode="hadamard")
    with pytest.raises(SystemExit, match="has no run-id 7"):
        rundb.classify(fixture_db, tmp_path, run_id=7)
    # an incomplete run, and duplicate stems, in a copy of the database
    copy = tmp_path / "copy.sqlite"
    copy.write_bytes(fixture_db.read_bytes())
    conn = sqlite3.connect(copy)
    conn.execute("UPDATE runs_genomes SET fasta_filename = 'NC_002696.fna' WHERE fasta_filename = 'NC_010338.fna.gz'")
    conn.commit()
    with pytest.raises(SystemExit, match="Duplicate filename stems, consider using MD5 labelling."):
        rundb.classify(copy, tmp_path)
    assert rundb.classify(copy, tmp_path, label="md5").is_file()
    conn.execute("DELETE FROM comparisons WHERE comparison_id = (SELECT MAX(comparison_id) FROM comparisons)")
    conn.commit()
    conn.close()
    with pytest.raises(SystemExit, match=r"run-id 1 has 15 of 4\^2=16 comparisons, 1 needed"):
        rundb.classify(copy, tmp_path, label="md5")


def test_rundb_classify_single_genome(tmp_path, caplog):
    fasta = tmp_path / "one"
    fasta.mkdir()
    (fasta / "OP073605.fasta").write_bytes((GOLDEN / "viral_example" / "OP073605.fasta").read_bytes())
    db = tmp_path / "one.sqlite"
    assert rundb.run_sourmash_hip(fasta, db, cache=tmp_path / "cache", scaled=300, engine=OracleEngine(), temp=tmp_path).status == "Done"
    caplog.set_level(logging.INFO)
    out = rundb.classify(db, tmp_path)
    assert "Run 1 has 1 comparison across 1 genome. Reporting single clique." in caplog.text
    assert out.read_text() == "n_nodes\tmax_cov\tmin_identity\tmax_identity\tmembers\n1\t\t\t\tOP073605\n"


@pytest.mark.skipif(not (REFERENCE / "pyani_plus" / "classify.py").is_file(), reason="the reference checkout is not here")
@pytest.mark.parametrize("mode", ["identity", "tANI"])
def test_rundb_classify_equals_the_reference_on_the_same_database(fixture_db, mode, tmp_path):
    """The reference's ORM reads ``run.identities`` / ``run.cov_query`` / ``run.tani`` of the database this project
    wrote, its classify functions run on them, and ``compute_classify_output`` writes its TSV: same rows as ours."""
    import datetime

    pytest.importorskip("sqlalchemy")
    pytest.importorskip("networkx")
    old_flag, old_path = sys.dont_write_bytecode, list(sys.path)
    sys.dont_write_bytecode = True
    if not hasattr(datetime, "UTC"):
        datetime.UTC = datetime.timezone.utc
    sys.path.append(str(REFERENCE))
    try:
        import networkx as nx
        from pyani_plus import classify as ref_classify
        from pyani_plus import db_orm
    except ImportError as err:
        pytest.skip(f"the reference does not import here: {err}")
    finally:
        sys.path[:] = old_path
        sys.dont_write_bytecode = old_flag
    ref_out = tmp_path / "ref"
    ref_out.mkdir()
    with db_orm.connect_to_db(logging.getLogger("classify"), fixture_db) as session:
        run = db_orm.load_run(session, None, check_complete=True)
        matrix = run.identities if mode == "identity" else run.tani.where(run.tani.isna(), run.tani * -1)
        score = run.relabelled_matrix(matrix, "stem")
        cov = run.relabelled_matrix(run.cov_query, "stem")
        graph = ref_classify.construct_graph(cov, score, ref_classify.AGG_FUNCS["min"], ref_classify.AGG_FUNCS["mean"], 0.5)
        initial = ref_classify.find_initial_cliques(graph) if len(list(nx.connected_components(graph))) != 1 else []
        unique = ref_classify.get_unique_cliques(initial, ref_classify.find_cliques_recursively(graph))
        suffix = "identity" if mode == "identity" else "-tANI"
        ref_classify.compute_classify_output(unique, run.configuration.method, ref_out, {"min_score": f"min_{suffix}", "max_score": f"max_{suffix}"})
    ours = rundb.classify(fixture_db, tmp_path / "ours", mode=mode).read_text().split("\n")
    theirs = (ref_out / "sourmash-hip_classify.tsv").read_text().split("\n")
    assert ours[0] == theirs[0] and len(ours) == len(theirs)

    def canon(lines):
        return sorted((sorted(f[4].split(",")), f[:4]) for f in (line.split("\t") for line in lines[1:-1]))

    assert canon(ours) == canon(theirs)
