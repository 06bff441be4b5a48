"""tree-run without a GPU: ``pa_nj_host`` against the numpy restatement of the contract (tests/tree_cases.py) bit for
bit and against the trees that generated the additive cases, its refusals, the distances of a run, UPGMA, the Newick
writer read back by a small parser, and ``rundb.tree_run`` with its command line on a small finished run."""

from __future__ import annotations

import logging
import sys

import numpy as np
import pytest

from pyani_plus_amd import rundb, tree
from pyani_plus_amd._capi import PA_E_INVALID, HipBackendError
from pyani_plus_amd.engine import nj_tree_host
from tests import tree_cases as tc
from tests.fake_engine import OracleEngine
from tests.helpers import FIXTURE_SETS, GOLDEN, distance_check_cases, distance_refusal

RESTATED = [c.name for c in tc.cases() if len(c.D) <= tc.RESTATED_UP_TO]
ADDITIVE = [c.name for c in tc.cases() if c.edges is not None]


def same_table(got, want) -> None:
    """(child, length, last, last_len) twice: the same integers and the same bits."""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), np.asarray(want[1]).view(np.uint64))
    if len(got[0]) or want[2] is not None:
        assert tuple(int(x) for x in got[2]) == tuple(want[2])
        assert np.float64(got[3]).view(np.uint64) == np.float64(want[3]).view(np.uint64)


# ------------------------------------------------------------------ the twin
def test_the_cases_cover_the_tiling():
    k = tc.kernel_constants()
    sizes = {len(c.D) for c in tc.cases()}
    assert {1, 2, 3, 4, 5} <= sizes and max(sizes) == tc.LARGEST == 513
    for edge in (k["kTile"], k["kThreads"]):
        assert {edge - 1, edge, edge + 1} <= sizes
    assert k["kThreads"] % k["kTile"] == 0


@pytest.mark.parametrize("threads", [1, 3, 16])
@pytest.mark.parametrize("name", RESTATED)
def test_twin_equals_the_restatement(name, threads):
    case = tc.case(name)
    before = case.D.copy()
    got = nj_tree_host(case.D, threads)
    assert np.array_equal(case.D.view(np.uint64), before.view(np.uint64)), "the matrix was modified"
    want = tc.restated(name)
    if len(case.D) == 1:
        assert got[0].shape == (0, 2) and got[1].shape == (0, 2)
        return
    same_table(got, want)


def test_twin_at_the_largest_size_whatever_the_threads():
    for name in (f"random{tc.LARGEST}", f"additive{tc.LARGEST}"):
        D = tc.case(name).D
        one = nj_tree_host(D, 1)
        for threads in (3, 16):
            same_table(nj_tree_host(D, threads), one)


@pytest.mark.parametrize("name", ADDITIVE)
def test_additive_cases_give_back_their_tree(name):
    case = tc.case(name)
    n = len(case.D)
    child, length, last, last_len = nj_tree_host(case.D, 3)
    got = tc.joins_bipartitions(n, child, length, last, last_len)
    assert got == case.edges  # the same bipartitions, the same lengths with ==
    if n <= tc.RESTATED_UP_TO:
        want = tc.restated(name)
        assert tc.joins_bipartitions(n, *want) == case.edges


def test_negative_lengths_are_kept():
    for name in (c.name for c in tc.cases() if c.name.startswith("random") and len(c.D) >= 5):
        _child, length, _last, _last_len = nj_tree_host(tc.case(name).D)
        assert (length < 0).any(), name


def test_ties_go_by_node_id():
    child, length, last, _ = nj_tree_host(tc.all_equal(33))
    assert tuple(child[0]) == (0, 1) and tuple(length[0]) == (0.25, 0.25)
    same_table(nj_tree_host(tc.all_equal(33), 3), tc.restated("all_equal33"))
    assert int(last[1]) == 2 * 33 - 3  # the last node made is one end of the last edge


TIE_NAMES = [c.name for c in tc.tie_cases()]


def test_the_tie_counter_counts_the_pairs_at_the_smallest_score():
    assert tc.tied_pairs_per_join(tc.all_equal(5)) == [10, 6, 3]  # every live pair, join after join: 5, 4 and 3 nodes
    # random distances do not tie on more than one tile (with four nodes left or three, scores are equal but for rounding)
    assert tc.tied_share(tc.tied_pairs_per_join(tc.case("random257").D), 257) == (0, 257 - tc.kernel_constants()["kTile"])
    tied: list[int] = []
    joins = tc.neighbour_joining(tc.case("duplicated9").D, tied)
    assert len(tied) == len(joins.child) and np.array_equal(joins.child, tc.restated("duplicated9").child)


@pytest.mark.parametrize("threads", [1, 3, 16])
@pytest.mark.parametrize("name", TIE_NAMES)
def test_twin_equals_the_restatement_where_ties_decide(name, threads):
    same_table(nj_tree_host(tc.tie_case(name).D, threads), tc.tie_restated(name)[0])


@pytest.mark.parametrize("name", TIE_NAMES)
def test_the_tie_cases_tie_on_more_than_one_tile(name):
    """A condition on the inputs, counted by the restatement alone: of the joins made while more than kTile nodes are
    live, at least a third have more than one pair at the smallest score; every one of them where all distances are equal.
    Counted here: all_equal257 129 of 129, copies258x86 65 of 130 (114 of 256 overall), copies130x65 1 of 2."""
    n = len(tc.tie_case(name).D)
    tied, joins = tc.tied_share(tc.tie_restated(name)[1], n)
    print(f"{name}: {tied} of {joins} joins on more than one tile are tied")
    assert joins == n - tc.kernel_constants()["kTile"] > 0
    assert 3 * tied >= joins
    if name.startswith("all_equal"):
        assert tied == joins
    else:
        assert (tc.tie_case(name).D == 0.0).sum() > n  # d = 0 between the copies of a genome


def test_the_far_tile_case_is_won_past_the_first_trip_over_the_candidates():
    k = tc.kernel_constants()
    far = tc.far_tile_case()
    n = len(far.D)
    assert (far.nt - 1) ** 2 <= k["kThreads"] < far.nt**2
    tiles = [(n - t + k["kTile"] - 1) // k["kTile"] for t in range(n - 2)]  # a side, join by join
    assert tiles[:3] == [far.nt, far.nt, far.nt - 1]  # exactly two joins with candidates past the workgroup's lanes
    child = tc.far_tile_twin()[0]
    assert tuple(child[0]) == far.first[0] == (2040, 2045) and tuple(child[1]) == far.first[1] == (2030, 2035)
    for t, (lo, hi) in enumerate(far.first):
        # join 0 puts its node into slot 2040 and the last slot's into 2045: the leaves of join 1 are where they were
        ti, tj = lo // k["kTile"], hi // k["kTile"]
        assert ti * tiles[t] + tj == far.candidate >= k["kThreads"], t


def test_small_n():
    child, length, last, last_len = nj_tree_host(np.zeros((1, 1)))
    assert child.shape == (0, 2) and length.shape == (0, 2)
    child, length, last, last_len = nj_tree_host(np.array([[0.0, 0.375], [0.375, 0.0]]))
    assert child.shape == (0, 2) and tuple(last) == (0, 1) and last_len == 0.375


@pytest.mark.parametrize("what,D,cell", tc.invalid_matrices(), ids=[w for w, _, _ in tc.invalid_matrices()])
def test_invalid_matrices_are_refused(what, D, cell):
    with pytest.raises(HipBackendError, match=rf"pa_nj_host: D\[{cell[0]},{cell[1]}\]") as err:
        nj_tree_host(D)
    assert err.value.status == PA_E_INVALID


@pytest.mark.parametrize("name,D,cell,count", distance_check_cases(), ids=[c[0] for c in distance_check_cases()])
def test_a_refusal_names_the_first_cell_and_counts_them_all(name, D, cell, count):
    with pytest.raises(HipBackendError) as err:
        nj_tree_host(D)
    assert err.value.status == PA_E_INVALID and str(err.value).endswith(distance_refusal("pa_nj_host", "D", cell, count))


def test_no_nodes_is_refused():
    with pytest.raises(HipBackendError, match="0 nodes") as err:
        nj_tree_host(np.zeros((0, 0)))
    assert err.value.status == PA_E_INVALID
    with pytest.raises(ValueError, match="square"):
        nj_tree_host(np.zeros((3, 4)))


# ------------------------------------------------------------------ distances of a run
def test_run_distances(caplog):
    nan = np.nan
    ident = np.array([[1.0, 0.9, nan, nan], [0.8, 1.0, 0.75, nan], [0.5, nan, nan, -0.25], [nan, nan, -0.125, 1.0]])
    with caplog.at_level(logging.WARNING):
        d = tree.run_distances(ident, missing=2.0)
    want = np.array(
        [[0.0, 1.0 - 0.5 * (0.9 + 0.8), 0.5, 2.0], [0.0, 0.0, 0.25, 2.0], [0.0, 0.0, 0.0, 1.0 - 0.5 * (-0.25 + -0.125)], [0.0, 0.0, 0.0, 0.0]]
    )
    want = want + want.T
    assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
    assert d[2, 3] > 1.0  # a TETRA-style negative identity is a distance above 1
    assert "2 of 6 genome pairs have no identity in either direction" in caplog.text
    assert np.array_equal(d, d.T) and d.flags.c_contiguous
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert tree.run_distances(np.array([[nan, 0.5], [0.25, 1.0]]))[0, 1] == 0.625
    assert caplog.text == ""
    assert tree.run_distances(np.array([[1.0, nan], [nan, 1.0]]))[0, 1] == 1.0  # the default for a missing pair
    import pandas as pd

    frame = pd.DataFrame(ident, index=list("abcd"), columns=list("abcd"))
    assert np.array_equal(tree.run_distances(frame, missing=2.0), d)
    with pytest.raises(ValueError, match="square"):
        tree.run_distances(np.zeros((2, 3)))


# ------------------------------------------------------------------ Newick
def parse_newick(text: str):
    """(children, label, length) of every node, the root last: a parser with its own stack."""
    assert text.endswith(";")
    nodes: list[dict] = []
    stack: list[list[int]] = []
    at = 0
    pending: list[int] | None = None  # the children of the group just closed
    while text[at] != ";":
        ch = text[at]
        if ch == "(":
            stack.append([])
            at += 1
            continue
        if ch == ",":
            at += 1
            continue
        if ch == ")":
            pending = stack.pop()
            at += 1
            if text[at] not in ":,);":
                raise AssertionError("inner nodes carry no label here")
        label = None
        if pending is None:
            if text[at] == "'":
                end = at + 1
                parts = []
                while True:
                    nxt = text.index("'", end)
                    parts.append(text[end:nxt])
                    if text[nxt + 1 : nxt + 2] == "'":
                        parts.append("'")
                        end = nxt + 2
                    else:
                        at = nxt + 1
                        break
                label = "".join(parts)
            else:
                end = at
                while text[end] not in ":,)":
                    end += 1
                label, at = text[at:end], end
        length = None
        if text[at] == ":":
            end = at + 1
            while text[end] not in ",);":
                end += 1
            length, at = float(text[at + 1 : end]), end
        nodes.append({"children": pending or [], "label": label, "length": length})
        pending = None
        if stack:
            stack[-1].append(len(nodes) - 1)
    return nodes


def newick_bipartitions(text: str, labels: list[str]) -> dict[frozenset, float]:
    nodes = parse_newick(text)
    index = {name: i for i, name in enumerate(labels)}
    below: list[frozenset] = []
    out: dict[frozenset, float] = {}
    n = len(labels)
    for node in nodes:  # children come before their parent
        leaves = frozenset([index[node["label"]]]) if not node["children"] else frozenset().union(*(below[c] for c in node["children"]))
        below.append(leaves)
        if node["length"] is not None:
            side = tc._side(leaves, n)
            out[side] = out.get(side, 0.0) + node["length"]  # the two halves of a two-leaf tree are one edge
    assert below[-1] == frozenset(range(n))
    return out


def test_newick_quoting_and_small_trees():
    assert tree.quote_label("NC_002696.2-a") == "NC_002696.2-a"
    assert tree.quote_label("E. coli") == "'E. coli'" and tree.quote_label("it's(1)") == "'it''s(1)'" and tree.quote_label("") == "''"
    one = tree.neighbour_joining(np.zeros((1, 1)))
    assert tree.newick(one, ["A"]) == "(A);"
    two = tree.neighbour_joining(np.array([[0.0, 0.375], [0.375, 0.0]]))
    assert tree.newick(two, ["A", "B b"]) == "(A:0.1875,'B b':0.1875);"
    with pytest.raises(ValueError, match="3 labels for 2 leaves"):
        tree.newick(two, ["A", "B", "C"])


def test_newick_has_a_trifurcated_root_and_keeps_the_bits():
    D = np.array([[0.0, 0.3, 0.5, 0.6], [0.3, 0.0, 0.6, 0.5], [0.5, 0.6, 0.0, 0.9], [0.6, 0.5, 0.9, 0.0]])
    table = tree.neighbour_joining(D)
    text = tree.newick(table, ["a", "b", "c", "d"])
    nodes = parse_newick(text)
    assert len(nodes[-1]["children"]) == 3 and nodes[-1]["length"] is None
    assert nodes[nodes[-1]["children"][2]]["length"] == table.last_len  # the other remaining node carries the last edge
    for name in ("random129", "additive130", "duplicated9", "all_equal33"):
        case = tc.case(name)
        n = len(case.D)
        labels = [f"g{i}" if i % 3 else f"genome {i}'s" for i in range(n)]
        table = tree.neighbour_joining(case.D)
        got = newick_bipartitions(tree.newick(table, labels), labels)
        want = tc.joins_bipartitions(n, table.child, table.length, table.last, table.last_len)
        assert got.keys() == want.keys()
        assert all(np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64) for k in want), name
        if case.edges is not None:
            assert got == case.edges


def test_newick_of_a_caterpillar_does_not_recurse():
    n = 5000
    # join t hangs leaf t + 2 on the node made before it: a tree n - 2 levels deep
    child = np.array([(0, 1)] + [(t + 1, n + t - 1) for t in range(1, n - 2)], dtype=np.uint32)
    length = np.full((n - 2, 2), 0.5)
    table = tree.JoinTable(n, child, length, (n - 1, 2 * n - 3), 0.25, False)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(200)
    try:
        text = tree.newick(table, [f"L{i}" for i in range(n)])
    finally:
        sys.setrecursionlimit(limit)
    assert text.count("(") == n - 2 and text.count(",") == n - 1 and text.endswith(f",L{n - 1}:0.25);")
    nodes = parse_newick(text)
    assert sum(1 for x in nodes if not x["children"]) == n


# ------------------------------------------------------------------ UPGMA
def ultrametric(n: int, seed: int):
    """A random rooted binary tree with distinct dyadic node heights: (D, {clade: height})."""
    rng = np.random.default_rng(seed)
    heights = np.sort(rng.choice(np.arange(1, 4097), size=n - 1, replace=False)) / 1024.0
    clades = [frozenset([i]) for i in range(n)]
    D = np.zeros((n, n))
    made = {}
    for h in heights:
        i, j = sorted(rng.choice(len(clades), size=2, replace=False))
        x, y = clades[i], clades[j]
        for a in x:
            for b in y:
                D[a, b] = D[b, a] = 2.0 * h
        clades = [c for k, c in enumerate(clades) if k not in (i, j)] + [x | y]
        made[x | y] = float(h)
    return D, made


@pytest.mark.parametrize("n", [2, 3, 9, 64])
def test_upgma_gives_back_the_heights_of_an_ultrametric_matrix(n):
    D, made = ultrametric(n, 40 + n)
    table = tree.upgma(D)
    assert table.rooted and table.child.shape == (n - 1, 2) and table.last is None
    below = {i: frozenset([i]) for i in range(n)}
    height = {i: 0.0 for i in range(n)}
    got = {}
    for t in range(n - 1):
        a, b = (int(x) for x in table.child[t])
        below[n + t] = below[a] | below[b]
        height[n + t] = height[a] + float(table.length[t, 0])
        assert height[n + t] == height[b] + float(table.length[t, 1])  # ultrametric: both children reach the same height
        got[below[n + t]] = height[n + t]
    assert got == made
    labels = [f"u{i}" for i in range(n)]
    nodes = parse_newick(tree.newick(table, labels))
    assert len(nodes[-1]["children"]) == 2 and sum(1 for x in nodes if not x["children"]) == n
    assert tree.newick(tree.upgma(np.zeros((1, 1))), ["A"]) == "(A);"


# ------------------------------------------------------------------ rundb.tree_run
@pytest.fixture(scope="module")
def viral_db(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tree_run_db")
    scaled, _genomes = FIXTURE_SETS["viral_example"]
    db = tmp / "run.sqlite"
    run = rundb.run_sourmash_hip(GOLDEN / "viral_example", db, cache=tmp / "cache", scaled=scaled, engine=OracleEngine(), temp=tmp)
    assert run.status == "Done"
    return db


def leaf_labels(text: str) -> list[str]:
    return sorted(x["label"] for x in parse_newick(text.strip()) if not x["children"])


def test_tree_run_and_its_command_line(viral_db, tmp_path, capsys):
    stems = sorted(p.stem for p in (GOLDEN / "viral_example").iterdir() if p.suffix in rundb.FASTA_EXTENSIONS)
    written = rundb.tree_run(viral_db, tmp_path / "out")
    assert written == tmp_path / "out" / "sourmash-hip_identity_nj.nwk"
    text = written.read_text()
    assert text.endswith(";\n") and text.count("\n") == 1 and leaf_labels(text) == stems
    assert len(parse_newick(text.strip())[-1]["children"]) == 3
    by_md5 = rundb.tree_run(viral_db, tmp_path / "out", label="md5")
    assert leaf_labels(by_md5.read_text()) == sorted(FIXTURE_SETS["viral_example"][1])
    upgma = rundb.tree_run(viral_db, tmp_path / "out", method="upgma")
    assert upgma.name == "sourmash-hip_identity_upgma.nwk" and leaf_labels(upgma.read_text()) == stems
    assert len(parse_newick(upgma.read_text().strip())[-1]["children"]) == 2
    assert rundb.main(["tree-run", "-d", str(viral_db), "-o", str(tmp_path / "cli")]) == 0
    assert capsys.readouterr().out.strip() == str(tmp_path / "cli" / "sourmash-hip_identity_nj.nwk")
    assert (tmp_path / "cli" / "sourmash-hip_identity_nj.nwk").read_bytes() == text.encode()
    assert rundb.main(["tree-run", "-d", str(viral_db), "-o", str(tmp_path / "cli"), "--method", "upgma", "--missing", "0.5"]) == 0
    assert (tmp_path / "cli" / "sourmash-hip_identity_upgma.nwk").read_bytes() == upgma.read_bytes()


def test_tree_run_messages(viral_db, tmp_path):
    with pytest.raises(SystemExit, match="Unknown tree method 'ml'"):
        rundb.tree_run(viral_db, tmp_path, method="ml")
    with pytest.raises(SystemExit):
        rundb.main(["tree-run", "-d", str(viral_db), "-o", str(tmp_path), "--method", "ml"])
    with pytest.raises(SystemExit, match=f"Database {tmp_path / 'none.sqlite'} does not exist"):
        rundb.tree_run(tmp_path / "none.sqlite", tmp_path)
    with pytest.raises(SystemExit, match="Unexpected label scheme 'name'"):
        rundb.tree_run(viral_db, tmp_path, label="name")
    with pytest.raises(SystemExit, match="must be finite and not negative"):
        rundb.tree_run(viral_db, tmp_path, missing=-1.0)
    assert not list(tmp_path.glob("*.nwk"))
