"""GPU: the smallest inputs of every entry point, where a kernel's grid is one block, one block and a single element, or
nothing at all (an empty sketch, a subject tile without postings, a genome without a fragment).  Expectations come from
numpy or from the stand-alone oracle, never from the library."""

from __future__ import annotations

import math

import numpy as np
import pytest

import oracle
from pyani_plus_amd import _capi
from pyani_plus_amd.synth import arena_to_ascii, synth_arena_numpy

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------ pair counts
@pytest.fixture(scope="module")
def three_sketches():
    """[empty, 5 hashes, the same 5 plus 3 others] and their intersection sizes."""
    rng = np.random.default_rng(11)
    values = np.unique(rng.integers(1, 1 << 62, size=8, dtype=np.uint64))
    assert len(values) == 8
    five = np.sort(values[[0, 2, 3, 5, 7]])
    sketches = [np.empty(0, dtype=np.uint64), five, values]
    want = np.array([[len(np.intersect1d(a, b)) for b in sketches] for a in sketches], dtype=np.uint32)
    assert want.tolist() == [[0, 0, 0], [0, 5, 5], [0, 5, 8]]
    return sketches, want


@pytest.mark.parametrize("algo", [_capi.PA_PAIRS_AUTO, _capi.PA_PAIRS_BITROW, _capi.PA_PAIRS_MERGE])
def test_pair_counts_with_an_empty_sketch(engine, three_sketches, algo):
    sketches, want = three_sketches
    sk = engine.sketches_from_host(sketches)
    full = engine.pair_counts(sk, algo=algo).cpu().numpy().view(np.uint32)
    assert np.array_equal(full, want)
    # one subject column at a time: a tile without postings, then query postings after the tile, before it and both
    for s0, s1 in ((0, 1), (1, 2), (2, 3)):
        part = engine.pair_counts(sk, s_range=(s0, s1), algo=algo).cpu().numpy().view(np.uint32)
        assert np.array_equal(part, want[:, s0:s1]), (s0, s1)


# ------------------------------------------------------------------ classify
def edges_by_double_loop(score, cov, cov_min=0.5):
    """The edges of ``pa_classify_edges`` with the default aggregators (mean score, min coverage) in removal order."""
    n = len(score)
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            a, b = cov[j, i], cov[i, j]
            c = b if b < a else a  # Python's min([a, b])
            s = (score[j, i] + score[i, j]) / 2.0
            if not math.isnan(c) and not math.isnan(s) and c > cov_min:
                edges.append((s, i, j, c))
    edges.sort(key=lambda e: e[:3])
    return (np.array([e[1] for e in edges], dtype=np.uint32), np.array([e[2] for e in edges], dtype=np.uint32),
            np.array([e[0] for e in edges], dtype=np.float64), np.array([e[3] for e in edges], dtype=np.float64))  # fmt: skip


def classify_case(name):
    if name == "two genomes, NaN score":
        return np.array([[1.0, np.nan], [0.9, 1.0]]), np.array([[1.0, 0.8], [0.9, 1.0]])
    if name == "two genomes, one edge":
        return np.array([[1.0, 0.95], [0.9, 1.0]]), np.array([[1.0, 0.8], [0.9, 1.0]])
    rng = np.random.default_rng(65)  # 65 genomes: two tiles a side, the second diagonal tile a single element
    score = np.round(0.8 + 0.2 * rng.random((65, 65)), 3)  # rounded: equal scores occur, the tie rule decides
    cov = rng.random((65, 65))
    score[rng.random((65, 65)) < 0.1] = np.nan
    cov[rng.random((65, 65)) < 0.1] = np.nan
    return score, cov


@pytest.mark.parametrize("name", ["two genomes, NaN score", "two genomes, one edge", "65 genomes"])
def test_classify_edges_of_the_smallest_graphs(engine, name):
    score, cov = classify_case(name)
    want = edges_by_double_loop(score, cov)
    assert len(want[0]) == {"two genomes, NaN score": 0, "two genomes, one edge": 1}.get(name, len(want[0]))
    # 65 genomes: hundreds of edges, some into the last tile, fewer distinct scores than edges
    assert name != "65 genomes" or (len(want[0]) > 300 and (want[1] == 64).any() and len(np.unique(want[2])) < len(want[2]))
    got = engine.classify_edges(score, cov)
    for mine, theirs in zip(got, want):
        assert mine.dtype == theirs.dtype and np.array_equal(mine, theirs), name


# ------------------------------------------------------------------ run join, minimum and maximum, histogram
@pytest.mark.parametrize("n_rows", [1, 64, 65])
@pytest.mark.parametrize("common", ["none", "all"])
def test_run_join_of_few_rows(engine, n_rows, common):
    rng = np.random.default_rng(n_rows)
    ref = rng.random((3, 3))
    q = rng.integers(0, 3, size=n_rows).astype(np.uint32)
    s = rng.integers(0, 3, size=n_rows).astype(np.uint32)
    y = rng.random(n_rows)
    if common == "none":
        q[:] = NONE  # not a genome of the reference run
        want_x = np.empty(0)
        want_y = np.empty(0)
    else:
        want_x = ref[q.astype(np.int64), s.astype(np.int64)]
        want_y = y
    got = engine.run_join(ref, q, s, y)
    for mine, theirs in zip(got, (want_x, want_y, want_y - want_x)):
        assert mine.shape == theirs.shape and np.array_equal(mine, theirs)


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("bins", [1, 1024])
def test_minmax_and_histogram_of_few_values(engine, n, bins):
    v = np.random.default_rng(n).random(n)
    lo, hi = float(v.min()), float(v.max())
    assert engine.minmax(v) == (lo, hi, n)
    if lo == hi:  # numpy.histogram's range of a single value
        lo, hi = lo - 0.5, hi + 0.5
    edges = np.linspace(lo, hi, bins + 1)
    want = np.histogram(v, bins, range=(lo, hi))[0]
    assert int(want.sum()) == n
    got = engine.hist_uniform(v, edges)
    assert np.array_equal(got, want.astype(np.uint64))


# ------------------------------------------------------------------ sketches
@pytest.mark.parametrize("lengths", [[64], [5000, 0, 3000]], ids=["one genome of 64 bases", "the middle genome empty"])
def test_sketches_of_tiny_arenas(engine, lengths):
    k, scaled = 21, 2
    arena = synth_arena_numpy(len(lengths), lengths, n_species=1)
    texts = [arena_to_ascii(arena, g) for g in range(len(lengths))]
    want = [oracle.sketch_seq(t, k, scaled) for t in texts]
    assert all((len(w) > 0) == (n > 0) for w, n in zip(want, lengths))
    got = engine.sketch(engine.upload(arena), k, scaled).to_host()
    _dev, streamed = engine.sketch_streamed(engine.pin_arena(arena), k, scaled)
    for g, w in enumerate(want):
        assert np.array_equal(got[g], w), g
        assert np.array_equal(streamed.to_host()[g], w), g
    bottom = engine.sketch_bottom(engine.upload(arena), k, 1).to_host()
    for g, t in enumerate(texts):
        w = oracle.sketch_bottom_seq(t, k, 1)
        assert len(w) == (1 if lengths[g] else 0) and np.array_equal(bottom[g], w), g


# ------------------------------------------------------------------ fragment ANI
def test_fragment_ani_with_a_genome_that_yields_no_fragment(engine):
    from pyani_plus_amd.methods.fastani_hip import fastani_mean

    k, frag = 16, 3000
    arena = synth_arena_numpy(2, [3000, 2999], n_species=1)
    texts = [arena_to_ascii(arena, g) for g in range(2)]
    assert [len(t) for t in texts] == [3000, 2999]
    starts = np.ascontiguousarray(arena.genome_start[:-1])
    lens = np.array([len(t) for t in texts], dtype=np.uint32)
    genome = np.arange(2, dtype=np.uint32)
    want = {(q, r): oracle.fragani_pair([texts[q]], [texts[r]], k, frag, 0.0) for q in range(2) for r in range(2)}
    assert [want[q, 0][2] for q in range(2)] == [1, 0]  # fragments of the two genomes

    def check(total, matched, ident_sum, columns):
        for q in range(2):
            for at, r in enumerate(columns):
                ani, m, t = want[q, r]
                assert (int(total[q]), int(matched[q, at])) == (t, m), (q, r)
                assert m == 0 or float(fastani_mean(ident_sum[q, at], m)) == ani, (q, r)

    dev = engine.upload(arena)
    check(*engine.fragani(dev, starts, lens, genome, k, frag), columns=(0, 1))
    total, matched, ident_sum = engine.fragani(dev, starts, lens, genome, k, frag, ref_range=(1, 2), columns_only=True)
    assert matched.shape == (2, 1) == ident_sum.shape
    check(total, matched, ident_sum, columns=(1,))
