"""csrc/bottom_mash.hip where ten synthetic genomes do not reach: every launch shape of ``mash_tile_kernel`` from the
1024-thread block to the LDS launch of exactly the budget, ragged tiles and blocks that are no multiple of a wavefront,
lists cut by m, empty lists, the hashes 0 and 2^64 - 1, the lane of ``mash_pair_kernel`` in which the m-th union element
falls, ``mash_ani_kernel`` on a made grid, and a ``pa_sketch_bottom`` call that raises its threshold once and stops there.

The cases come from tests/mash_cases.py; tests/test_mash_cases.py keeps them aimed at the kernel file's constants and shows
which wrong kernel each would catch.  Counts are exact against the brute-force estimator and against
``oracle.mash_pairs``."""

from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from tests import mash_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


@lru_cache(maxsize=None)
def _expected(kind: str, key, m: int) -> tuple[np.ndarray, np.ndarray]:
    """The estimator over all pairs of a case, computed once: the brute-force matrices, equal to the oracle's."""
    sketches = {"ladder": lambda: cases.ladder_case(*key), "short": lambda: cases.short_case()[0], "wave": lambda: cases.wave_case()[0]}[kind]()
    common, denom = cases.brute_matrices(sketches, m)
    o_common, o_denom = oracle.mash_pairs(sketches, m)
    assert np.array_equal(common, o_common) and np.array_equal(denom, o_denom)
    common.setflags(write=False)
    denom.setflags(write=False)
    return common, denom


def _mash(engine, sk, m, q_range=None, s_range=None) -> tuple[np.ndarray, np.ndarray]:
    common, denom = engine.pair_mash(sk, m, q_range, s_range)
    return common.cpu().numpy().view(np.uint32), denom.cpu().numpy().view(np.uint32)


def _same(got, want, what: str) -> None:
    for name, g, w in zip(("common", "denom"), got, want):
        assert g.shape == w.shape, what
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.argwhere(g != w)[:6].tolist()}: {g[g != w][:6]} for {w[g != w][:6]}"


@pytest.mark.parametrize("run", cases.ladder_runs(), ids=lambda r: r[0])
def test_geometry_ladder(engine, run):
    """One sketch set per number of lists that fit in LDS: 2 x 2, 1 x 2 and 1 x 1 tiles, the launch whose dynamic LDS is
    the budget to the byte, the first length that goes to the wave kernel, and a 25 000-hash list cut by m at either side
    of that threshold."""
    name, length, edge, m = run
    sketches = cases.ladder_case(length, edge)
    want = _expected("ladder", (length, edge), m)
    sk = engine.sketches_from_host(sketches)
    _same(_mash(engine, sk, m), want, name)
    long = cases.LADDER_LONG  # the governing list as the only row, then as the only column
    _same(_mash(engine, sk, m, (long, long + 1), (0, 5)), tuple(w[long : long + 1] for w in want), f"{name}, its row")
    _same(_mash(engine, sk, m, (0, 5), (long, long + 1)), tuple(w[:, long : long + 1] for w in want), f"{name}, its column")


@pytest.mark.parametrize("m", cases.SHORT_MS)
def test_many_short_lists(engine, m):
    """70 sketches of 0..8 hashes of a pool of 40: 3 x 3 tiles of 32 x 32 (the 1024-thread block) with a ragged edge of
    6, windows at offsets, a block of 64 with 35 live threads; empty, identical, prefix and interleaved lists; 0 and
    2^64 - 1."""
    sketches, _pool = cases.short_case()
    want = _expected("short", None, m)
    sk = engine.sketches_from_host(sketches)
    for q_range, s_range in cases.SHORT_WINDOWS:
        block = tuple(w[q_range[0] : q_range[1], s_range[0] : s_range[1]] for w in want)
        _same(_mash(engine, sk, m, q_range, s_range), block, f"m = {m}, rows {q_range} x columns {s_range}")


@pytest.mark.parametrize("where", cases.WAVE_WHERE)
def test_wave_kernel_lanes(engine, where):
    """Two 20 000-hash lists sharing every third hash beside lists of 0, 1, 3 and 70: the m-th union element of the long
    pair on the last step of a lane's slice, on the first, and on an A step whose equal B element opens the next lane."""
    sketches, facts = cases.wave_case()
    m = facts["m"][where]
    assert cases.launch_plan(sketches, m)["path"] == "wave"
    want = _expected("wave", None, m)
    sk = engine.sketches_from_host(sketches)
    _same(_mash(engine, sk, m), want, f"m = {m} ({where}, lane {facts['lane'][where]})")
    a, b = cases.WAVE_A, cases.WAVE_B
    _same(_mash(engine, sk, m, (a, a + 1), (b, b + 1)), tuple(w[a : a + 1, b : b + 1] for w in want), f"m = {m}, the long pair alone")


def test_ani_mash_grid(engine):
    """common, denom in {0, 1, 2, 999, 1000, 2^32 - 1}, vectors of 1, 255, 256 and 257 entries, k in {1, 21, 31, 64}.
    NaN exactly where common or denom is 0, 1.0 exactly where they are equal; elsewhere against 1 + ln(2j / (1 + j)) / k at
    60 digits, in units of u = 2^-52 max(1, |ln(2j / (1 + j))| / k): the device may be as far off as the float64
    restatement with the host's libm (``oracle.mash_ani``) is at its worst, plus 2 u for the two ulp of the device log."""
    t = engine.torch
    grid = np.array(cases.ANI_GRID, dtype=np.uint64).astype(np.uint32)
    host_worst, device_worst = (0.0, None), (0.0, None)
    for k in cases.ANI_KS:
        host = oracle.mash_ani(grid[:, 0], grid[:, 1], k)
        for (c, d), v in zip(cases.ANI_GRID, host):
            if c and d and c != d:
                err = cases.ani_error_in_units(float(v), c, d, k)
                if err > host_worst[0]:
                    host_worst = (err, f"common {c}, denom {d}, k {k}: {float(v)!r}")
    for size in cases.ANI_SIZES:
        common, denom = cases.ani_vectors(size)
        d_common = t.from_numpy(common.view(np.int32)).to(engine.device)
        d_denom = t.from_numpy(denom.view(np.int32)).to(engine.device)
        for k in cases.ANI_KS:
            got = engine.ani_mash(d_common, d_denom, k).cpu().numpy()
            assert got.shape == (size,)
            null = (common == 0) | (denom == 0)
            assert np.array_equal(np.isnan(got), null), f"size {size}, k {k}: NaN at {np.flatnonzero(np.isnan(got) != null)[:6]}"
            equal = ~null & (common == denom)
            assert np.all(got[equal] == 1.0), f"size {size}, k {k}"
            for i in np.flatnonzero(~null & ~equal):
                c, d = int(common[i]), int(denom[i])
                err = cases.ani_error_in_units(float(got[i]), c, d, k)
                if err > device_worst[0]:
                    device_worst = (err, f"size {size}, entry {i}: common {c}, denom {d}, k {k}: {float(got[i])!r}")
    print(f"oracle.mash_ani: worst error {host_worst[0]:.4f} u ({host_worst[1]})")
    print(f"pa_ani_mash: worst error {device_worst[0]:.4f} u ({device_worst[1]})")
    assert host_worst[1] is not None and device_worst[1] is not None
    assert device_worst[0] <= host_worst[0] + 2.0, (device_worst, host_worst)


def test_sketch_bottom_raises_its_threshold_once(engine):
    """A 20 kb random genome sets the first threshold; a genome of 25 copies of a 2 kb unit holds too few hashes under it
    and enough under the next (tests/test_mash_cases.py counts them): the loop ends below the maximum threshold."""
    from pyani_plus_amd.engine import pack_genomes

    k, m = cases.ESCALATION_K, cases.ESCALATION_M
    genomes = cases.escalation_genomes()
    arena = pack_genomes(genomes, fasta=False)
    sk = engine.sketch_bottom(engine.upload(arena), k, m)
    want = [oracle.sketch_bottom_seq(g, k, m) for g in genomes]
    assert sk.total == 2 * m
    for g, (a, b) in enumerate(zip(sk.to_host(), want)):
        assert len(b) == m and np.array_equal(a, b), f"genome {g}: {len(a)} hashes"
    common, denom = _mash(engine, sk, m)
    o_common, o_denom = oracle.mash_pairs(want, m)
    assert np.array_equal(common, o_common) and np.array_equal(denom, o_denom)
