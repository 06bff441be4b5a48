"""The pair phase where random sketches do not reach: the in-loop flush of ``row_sum_kernel``'s bit-sliced counters, long
probe chains in the hash dictionary (over the end of the table, down to an empty slot), a radix dictionary that sorts
zero passes, and ``ani_kernel`` on odd shapes, unaligned rows, offsets and extreme sizes.

The cases come from tests/pair_phase_cases.py; tests/test_pair_phase_cases.py keeps them aimed at the kernel's constants.
Counts are exact against the oracle; the device ANI transform is within 1 ulp (rtol 2.3e-16) of ``ani_host``."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from tests import pair_phase_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


def _counts(engine, sk, q_range=None, s_range=None, algo=0) -> np.ndarray:
    return engine.pair_counts(sk, q_range, s_range, algo=algo).cpu().numpy().view(np.uint32)


@lru_cache(maxsize=None)
def _flush_oracle(tpr: int) -> np.ndarray:
    return oracle.pair_counts(cases.flush_case(tpr)[0], threads=8)


@pytest.mark.parametrize("tpr", sorted(cases.FLUSH_TILE))
def test_row_sums_across_counter_flushes(engine, tpr):
    """A query long enough for every lane to flush its counters twice inside the loop and go on adding, against subjects
    that tell a counter that was not reset, a lost carry into the upper planes and a dropped tail apart."""
    sketches, facts = cases.flush_case(tpr)
    n, i = len(sketches), facts["query"]
    want = _flush_oracle(tpr)
    assert np.array_equal(want[i], facts["row"])
    sk = engine.sketches_from_host(sketches)
    for algo in (1, 3):
        got = _counts(engine, sk, algo=algo)
        assert np.array_equal(got[i], want[i]), f"algo {algo}, the long query's row: columns {np.flatnonzero(got[i] != want[i])[:8]}"
        assert np.array_equal(got, want), f"algo {algo}"
        band = _counts(engine, sk, (i, i + 1), (0, n), algo=algo)
        assert np.array_equal(band, want[i : i + 1]), f"algo {algo}, one-row band: columns {np.flatnonzero(band[0] != want[i])[:8]}"
    merged = _counts(engine, sk, (i, i + 1), (0, n), algo=2)  # the per-pair merge: no counters, no dictionary
    assert np.array_equal(merged, want[i : i + 1])


def test_dictionary_with_clustered_keys(engine):
    """1 500 subject keys whose first probe is the last slot of the subject tile's table and 1 000 on its middle slot;
    queries with keys of those slots that no subject holds, with 0 and with 2^64 - 1."""
    sketches, facts = cases.clustered_case()
    n, ns = len(sketches), facts["n_subjects"]
    want = oracle.pair_counts(sketches)
    assert np.array_equal(want, cases.set_counts(sketches))
    sk = engine.sketches_from_host(sketches)
    n_post = int(sk.offsets_host()[ns])
    assert cases.dict_cap(n_post) == facts["cap"]  # the tile of the subjects alone is the one the keys were made for
    for q_range, s_range in (((0, n), (0, ns)), ((ns, n), (0, ns)), ((0, n), (0, n))):
        block = want[q_range[0] : q_range[1], s_range[0] : s_range[1]]
        for algo in (0, 3, 1, 2):
            got = _counts(engine, sk, q_range, s_range, algo=algo)
            assert np.array_equal(got, block), f"algo {algo}, queries {q_range} x subjects {s_range}"
    # the same tile through a dictionary built ahead from a copy of its postings
    postings = sk.hashes[:n_post].clone()
    for q_range in ((0, n), (ns, n)):
        engine.pair_dict_prepare(postings, n_post)
        got = _counts(engine, sk, q_range, (0, ns))
        assert np.array_equal(got, want[q_range[0] : q_range[1], :ns]), f"prepared dictionary, queries {q_range}"


def test_radix_dictionary_with_all_zero_keys(engine):
    """The OR of all keys is 0: the radix sort runs zero passes and the dictionary is its input."""
    sketches = [np.array(s, dtype=np.uint64) for s in ([0], [0], [], [0])]
    want = oracle.pair_counts(sketches)
    assert want.tolist() == [[1, 1, 0, 1], [1, 1, 0, 1], [0, 0, 0, 0], [1, 1, 0, 1]]
    sk = engine.sketches_from_host(sketches)
    assert np.array_equal(_counts(engine, sk, algo=1), want)
    assert np.array_equal(_counts(engine, sk, (1, 4), (0, 3), algo=1), want[1:4, 0:3])


def test_ani_shapes_offsets_and_extremes(engine):
    """Every entry of ``ani_cases``: 1 x 1 to 70 000 x 3, odd widths, windows at odd offsets, counts that start 4 bytes
    into their buffer, sizes from 1 to 2^32 + 5, k from 1 to 64.  Reference: ``ani_host`` (host libm) on the same counts."""
    from pyani_plus_amd.engine import DeviceSketches, ani_host

    t = engine.torch
    dummy = t.zeros(1, dtype=t.int64, device=engine.device)
    worst = (0.0, None)
    uploaded: dict[int, tuple] = {}
    for sizes, counts, q_range, s_range, k, misalign in cases.ani_cases():
        if id(counts) not in uploaded:  # one upload per shape, shared by its six k
            off = np.zeros(len(sizes) + 1, dtype=np.int64)
            np.cumsum(np.array(sizes, dtype=np.int64), out=off[1:])
            sk = DeviceSketches(dummy, t.from_numpy(off).to(engine.device), len(sizes), int(off[-1]))
            buffer = t.zeros(counts.size + misalign, dtype=t.int32, device=engine.device)
            view = buffer[misalign:].view(counts.shape)
            view.copy_(t.from_numpy(counts.view(np.int32)))
            assert view.data_ptr() == buffer.data_ptr() + 4 * misalign
            uploaded[id(counts)] = (sk, buffer, view)
        sk, _buffer, view = uploaded[id(counts)]
        q = np.array(sizes[q_range[0] : q_range[1]], dtype=np.uint64)
        s = np.array(sizes[s_range[0] : s_range[1]], dtype=np.uint64)
        ident, cov, null = ani_host(counts, q, s, k)
        assert np.array_equal(null, counts == 0)
        d_ident, d_cov = (x.cpu().numpy() for x in engine.ani(view, sk, k, q_range, s_range))
        what = f"{counts.shape[0]} x {counts.shape[1]} at ({q_range[0]}, {s_range[0]}), k = {k}, misalign {misalign}"
        assert d_ident.shape == d_cov.shape == counts.shape
        assert np.array_equal(np.isnan(d_ident), null) and np.array_equal(np.isnan(d_cov), null), what
        whole_q = counts == q[:, None]
        whole = whole_q & (counts == s[None, :])
        assert np.all(d_cov[whole_q] == 1.0) and np.all(d_ident[whole] == 1.0), what
        for name, got, ref in (("identity", d_ident, ident), ("cov_query", d_cov, cov)):
            rel = np.zeros(counts.shape)
            rel[~null] = np.abs(got[~null] - ref[~null]) / ref[~null]
            at = np.unravel_index(np.argmax(rel), rel.shape)
            if rel[at] > worst[0]:
                ulps = abs(int(got[at].view(np.int64)) - int(ref[at].view(np.int64)))
                worst = (float(rel[at]), f"{name} of {what}: count {counts[at]}, |Q| {q[at[0]]}, |S| {s[at[1]]}: device {got[at]!r}, host {ref[at]!r}, {ulps} ulp")
    print(f"largest relative difference {worst[0]:.3e}: {worst[1]}")
    assert worst[0] <= 2.3e-16, worst
