"""The two device primitives of csrc/radix_sort.hip, called directly: ``pa_radix_sort_pairs`` and ``pa_exclusive_scan_u32``.

Six pipelines stand on them (the global sketch sort, the radix pair dictionary, classify's edge sort, fragment ANI's
posting and hit sorts, the run join's group offsets, the bottom-sketch truncation) and see them only at the sizes and
key patterns those pipelines produce.  Here they run through the probes ``pa_tool_radix_sort_pairs`` and
``pa_tool_exclusive_scan_u32`` of ``libpyani_hip_tools.so``, which links the same ``radix_sort.o`` as the product library.

Every expectation is numpy's: a stable argsort of the selected bits for the sort (with ``vals = arange(n)`` that pins
stability), a 64-bit cumulative sum for the scan.  Everything is an integer: every comparison is ``np.array_equal``.
Each case asserts the properties of its own input that make it bite (fixed seeds).  Every device buffer carries ``PAD``
elements of a pattern behind its ``n`` elements, which must still be there afterwards."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from pyani_plus_amd import _capi

pytestmark = pytest.mark.gpu

TILE = 2048  # elements per workgroup of the sort's kernels, and values per workgroup of the scan's (kTile, kScanTile)
ROUND = 256  # tile sums per round of scan_sums_kernel (kScanThreads)
RADIX = 256
PAD = 8
FILL64, FILL32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
TOTAL_FILL = np.uint64(0x5A5A5A5A5A5A5A5A)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = [0, 1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * TILE + 1]
PATTERN_SIZES = [2049, 3 * TILE + 1]


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0, tools=True)
    yield eng
    eng.close()


# ------------------------------------------------------------------ plumbing
def _to_device(engine, a: np.ndarray, fill):
    """``a`` followed by PAD elements of ``fill``, on the device (u64 as int64, u32 as int32: the same bits)."""
    padded = np.concatenate([a, np.full(PAD, fill, dtype=a.dtype)])
    signed = np.int64 if a.dtype == np.uint64 else np.int32
    return engine.torch.from_numpy(padded.view(signed).copy()).to(engine.device)


def _to_host(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


class Pairs:
    """The sort's double buffers: half ``which`` holds (keys, vals), the other half a pattern."""

    def __init__(self, engine, keys: np.ndarray, vals: np.ndarray, which: int = 0):
        assert keys.dtype == np.uint64 and vals.dtype == np.uint32 and keys.shape == vals.shape and keys.ndim == 1
        self.engine, self.n, self.which = engine, len(keys), which
        blank_k, blank_v = np.full(self.n, FILL64, dtype=np.uint64), np.full(self.n, FILL32, dtype=np.uint32)
        self.d_keys = [_to_device(engine, keys if h == which else blank_k, FILL64) for h in (0, 1)]
        self.d_vals = [_to_device(engine, vals if h == which else blank_v, FILL32) for h in (0, 1)]

    def sort(self, lo: int, hi: int, by_val: bool = False) -> int:
        """One call of the primitive; returns its status.  ``self.which`` follows the call's ``*which``."""
        which = C.c_int(self.which)
        status = self.engine.lib.pa_tool_radix_sort_pairs(
            self.engine.ctx, self.d_keys[0].data_ptr(), self.d_keys[1].data_ptr(), self.d_vals[0].data_ptr(), self.d_vals[1].data_ptr(),
            self.n, lo, hi, int(by_val), C.byref(which),
        )
        assert which.value in (0, 1)
        self.which = which.value
        return status

    def host(self, half: int) -> tuple[np.ndarray, np.ndarray]:
        """Half ``half`` as the device holds it, after a check that nothing was written behind its n elements."""
        keys, vals = _to_host(self.d_keys[half], np.uint64), _to_host(self.d_vals[half], np.uint32)
        assert np.array_equal(keys[self.n :], np.full(PAD, FILL64)) and np.array_equal(vals[self.n :], np.full(PAD, FILL32)), "written past n"
        return keys[: self.n], vals[: self.n]

    def assert_untouched(self, keys: np.ndarray, vals: np.ndarray, which: int) -> None:
        assert self.which == which
        got_k, got_v = self.host(which)
        assert np.array_equal(got_k, keys) and np.array_equal(got_v, vals)
        other_k, other_v = self.host(which ^ 1)
        assert np.array_equal(other_k, np.full(self.n, FILL64)) and np.array_equal(other_v, np.full(self.n, FILL32))


def _field(x: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """Bits [lo, hi) of ``x`` (any unsigned width) as u64."""
    return (x.astype(np.uint64) >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)


def _expected(keys, vals, lo, hi, by_val=False):
    order = np.argsort(_field(vals if by_val else keys, lo, hi), kind="stable")
    return keys[order], vals[order]


def _check_sort(engine, keys, vals, lo, hi, by_val=False, which=0, what=""):
    want_k, want_v = _expected(keys, vals, lo, hi, by_val)
    pairs = Pairs(engine, keys, vals, which)
    status = pairs.sort(lo, hi, by_val)
    assert status == _capi.PA_OK, f"{what}: status {status}: {_capi.last_error(engine.lib)}"
    if len(keys) <= 1 or hi == lo:
        pairs.assert_untouched(keys, vals, which)
        return
    got_k, got_v = pairs.host(pairs.which)
    bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v), (
        f"{what}: n = {len(keys)}, bits [{lo}, {hi}), by_val = {by_val}, which = {which}: {len(bad)} elements differ, first at {bad[:4]}"
    )


def _random_keys(rng, n: int) -> np.ndarray:
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


def _iota(n: int) -> np.ndarray:
    return np.arange(n, dtype=np.uint32)


def _with_repeated_field(rng, x: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """``x`` with bits [lo, hi) drawn from a pool of len(x) / 3 random fields: equal fields between elements whose other
    bits stay random."""
    pool = _field(rng.integers(0, 2**64, size=max(len(x) // 3, 1), dtype=np.uint64), lo, hi)
    mask = np.uint64(((1 << (hi - lo)) - 1) << lo)
    field = (pool[rng.integers(0, len(pool), size=len(x))] << np.uint64(lo)).astype(np.uint64)
    return ((x.astype(np.uint64) & ~mask) | field).astype(x.dtype)


def _ties_are_out_of_order(x: np.ndarray, tiebreak: np.ndarray, lo: int, hi: int) -> bool:
    """Some two elements with equal bits [lo, hi) of ``x`` stand with the larger ``tiebreak`` first: a sort that looked
    at more than the field, or that was not stable, would put them the other way round."""
    order = np.argsort(_field(x, lo, hi), kind="stable")
    f, t = _field(x, lo, hi)[order], tiebreak[order]
    return bool(np.any((f[1:] == f[:-1]) & (t[1:] < t[:-1])))


# ------------------------------------------------------------------ sort
@pytest.mark.parametrize("which", [0, 1])
def test_sort_sizes(engine, which):
    """Every size around a wave row (64), a wave's slice (512) and a tile (2048), on full 64-bit keys: once random (all
    distinct), once drawn from three values (equal keys in every row, so the ranks inside a row and the carried counts
    are all in play).  ``n <= 1`` touches nothing."""
    rng = np.random.default_rng(20261 + which)
    three = np.array([0x0123456789ABCDEF, 0x0123456789ABCDEE, 0xFF00FF00FF00FF00], dtype=np.uint64)
    for n in SIZES:
        keys = _random_keys(rng, n)
        assert len(np.unique(keys)) == n
        _check_sort(engine, keys, _iota(n), 0, 64, which=which, what="random keys")
        few = three[rng.integers(0, 3, size=n)]
        assert n < 63 or len(np.unique(few)) == 3
        _check_sort(engine, few, _iota(n), 0, 64, which=which, what="three distinct keys")


@pytest.mark.parametrize("which", [0, 1])
def test_sort_of_an_empty_bit_range_touches_nothing(engine, which):
    """``bit_hi == bit_lo`` (and below it): no pass, ``which`` and both halves as they were."""
    rng = np.random.default_rng(20263)
    keys = _random_keys(rng, 2049)
    for lo, hi, by_val in ((0, 0, False), (16, 16, False), (64, 64, False), (24, 8, False), (8, 8, True)):
        pairs = Pairs(engine, keys, _iota(2049), which)
        assert pairs.sort(lo, hi, by_val) == _capi.PA_OK
        pairs.assert_untouched(keys, _iota(2049), which)


def _pattern(name: str, n: int):
    """(keys, bit_lo, bit_hi) of a key pattern, with the assertions that make it what its name says."""
    rng = np.random.default_rng([20264, n])
    rows = -(-n // 64)
    if name == "random":
        keys = _random_keys(rng, n)
        assert len(np.unique(keys)) == n
        return keys, 0, 64
    if name == "three_values":
        three = np.array([0x0123456789ABCDEF, 0x0123456789ABCDEE, 0xFF00FF00FF00FF00], dtype=np.uint64)
        keys = three[rng.integers(0, 3, size=n)]
        # every value several times in every full row of 64, hence in every wave's slice and every tile: equal keys
        # are ranked inside a row, carried from row to row, and ordered across waves and tiles
        full = keys[: (n // 64) * 64].reshape(-1, 64)
        assert all(((full == v).sum(axis=1) >= 5).all() for v in three)
        return keys, 0, 64
    if name == "all_equal":
        keys = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)  # one bucket holds each whole tile, in all 8 passes
        assert n > TILE
        return keys, 0, 64
    if name == "all_ones":
        keys = np.full(n, ALL_ONES, dtype=np.uint64)
        assert n % 64 != 0 and n % TILE != 0  # the last row has live lanes with digit 0xff beside dead lanes (key ~0)
        return keys, 0, 64
    if name in ("sorted", "reversed"):
        keys = np.sort(_random_keys(rng, n // 4)[rng.integers(0, n // 4, size=n)])
        assert len(np.unique(keys)) < n  # duplicates: equal keys keep their input order in both directions
        return (keys if name == "sorted" else keys[::-1].copy()), 0, 64
    if name == "top_byte":
        low = np.uint64(0x00C0FFEE12345678)
        keys = (rng.integers(0, 256, size=n, dtype=np.uint64) << np.uint64(56)) | low
        assert len(np.unique(keys >> np.uint64(56))) == 256 and np.all(keys & np.uint64(0x00FFFFFFFFFFFFFF) == low)
        return keys, 56, 64
    raise AssertionError(name)


@pytest.mark.parametrize("n", PATTERN_SIZES)
@pytest.mark.parametrize("name", ["random", "three_values", "all_equal", "all_ones", "sorted", "reversed", "top_byte"])
def test_sort_key_patterns(engine, name, n):
    keys, lo, hi = _pattern(name, n)
    assert n % TILE == 1  # the last tile holds one element: one live lane, 63 dead ones, and three waves without any
    _check_sort(engine, keys, _iota(n), lo, hi, which=n & 1, what=name)


@pytest.mark.parametrize("lo,hi", [(0, 8), (0, 16), (8, 24), (40, 64), (4, 12)])
def test_sort_bit_ranges(engine, lo, hi):
    """Only bits [lo, hi) order the result: the other bits are random, and elements that agree inside the range stay in
    input order whatever their other bits say."""
    n = 3 * TILE + 1
    rng = np.random.default_rng([20265, lo, hi])
    keys = _with_repeated_field(rng, _random_keys(rng, n), lo, hi)
    assert len(np.unique(_field(keys, lo, hi))) < n  # ties inside the range ...
    assert _ties_are_out_of_order(keys, keys, lo, hi)  # ... that a sort on more bits would have reordered
    assert len(np.unique(keys)) == n
    _check_sort(engine, keys, _iota(n), lo, hi, what="bit range")


@pytest.mark.parametrize("hi", [8, 16, 32])
def test_sort_by_value(engine, hi):
    """``by_val``: the digits come from the 32-bit values, and the keys travel with them."""
    n = 3 * TILE + 1
    rng = np.random.default_rng([20266, hi])
    vals = _with_repeated_field(rng, rng.integers(0, 2**32, size=n, dtype=np.uint32), 0, hi)
    keys = _random_keys(rng, n)
    assert vals.dtype == np.uint32 and len(np.unique(_field(vals, 0, hi))) < n
    assert _ties_are_out_of_order(vals, keys, 0, hi)
    # the keys' digits say something else than the values': a pass that read its digit from the key shows
    assert not np.array_equal(np.argsort(_field(keys, 0, hi), kind="stable"), np.argsort(_field(vals, 0, hi), kind="stable"))
    _check_sort(engine, keys, vals, 0, hi, by_val=True, what="by value")
    _check_sort(engine, keys, vals, 0, hi, by_val=True, which=1, what="by value")


def test_sort_by_key_then_by_value_is_genome_major(engine):
    """The sketch's composition (pa_sketch's global sort): all 64 bits of the hash, then 16 bits of the genome id, on the
    same double buffers.  The result is genome-major and hash-minor."""
    n, n_genomes = 3 * TILE + 1, 300
    rng = np.random.default_rng(20267)
    keys = _random_keys(rng, n // 2)[rng.integers(0, n // 2, size=n)]  # hashes shared between genomes
    vals = rng.integers(0, n_genomes, size=n, dtype=np.uint32)
    assert len(np.unique(vals)) == n_genomes > RADIX and len(np.unique(keys)) < n
    order = np.lexsort((keys, vals))
    pairs = Pairs(engine, keys, vals, 0)
    assert pairs.sort(0, 64) == _capi.PA_OK
    assert pairs.sort(0, 16, by_val=True) == _capi.PA_OK
    got_k, got_v = pairs.host(pairs.which)
    assert np.array_equal(got_v, vals[order]) and np.array_equal(got_k, keys[order])
    assert np.all(np.diff(got_v.astype(np.int64)) >= 0)
    same_genome = got_v[1:] == got_v[:-1]
    assert np.all(got_k[1:][same_genome] >= got_k[:-1][same_genome])


def test_sort_whose_histogram_scan_takes_a_second_round(engine):
    """2048 * 2048 + 1 elements are 2049 sort tiles: the [256][2049] histogram is 257 scan tiles, so the scan of the tile
    sums (one workgroup, 256 per round) goes into a second round, in place."""
    n = TILE * TILE + 1
    sort_tiles = -(-n // TILE)
    assert -(-(RADIX * sort_tiles) // TILE) == ROUND + 1
    rng = np.random.default_rng(20268)
    keys = _random_keys(rng, n)
    assert len(np.unique(_field(keys, 0, 16))) == 1 << 16  # every digit of both passes in use, ties everywhere
    _check_sort(engine, keys, _iota(n), 0, 16, what="second scan round")


@pytest.mark.parametrize(
    "lo,hi,by_val",
    [(-8, 8, False), (-8, 0, False), (-1, 7, True), (0, 12, False), (0, 63, False), (4, 13, False), (0, 4, True), (0, 72, False),
     (60, 68, False), (64, 72, False), (0, 40, True), (24, 40, True), (32, 40, True)],
)
def test_sort_refuses_ranges_it_cannot_sort(engine, lo, hi, by_val):
    """A negative bit_lo, a width that is not whole 8-bit digits, a bit_hi beyond the 64 bits of a key or the 32 bits of
    a value: PA_E_INVALID with a message, on the host, before any launch.  ``which`` and the buffers stay as they were."""
    assert hi > lo and (lo < 0 or (hi - lo) % 8 != 0 or hi > (32 if by_val else 64))
    n = 2049
    rng = np.random.default_rng(20269)
    keys, vals = _random_keys(rng, n), rng.integers(0, 2**32, size=n, dtype=np.uint32)
    for which in (0, 1):
        pairs = Pairs(engine, keys, vals, which)
        status = pairs.sort(lo, hi, by_val)
        message = _capi.last_error(engine.lib)
        assert status == _capi.PA_E_INVALID, (status, message)
        assert message.startswith("radix sort: ") and (str(lo) in message or str(hi) in message), message
        pairs.assert_untouched(keys, vals, which)


# ------------------------------------------------------------------ scan
def _scan(engine, v: np.ndarray, *, in_place: bool = False, with_total: bool = True):
    """One call of the scan: (outputs, total or None).  The total's slot holds a pattern before the call."""
    assert v.dtype == np.uint32
    n = len(v)
    d_in = _to_device(engine, v, FILL32)
    d_out = d_in if in_place else _to_device(engine, np.full(n, FILL32, dtype=np.uint32), FILL32)
    d_total = _to_device(engine, np.full(1, TOTAL_FILL, dtype=np.uint64), TOTAL_FILL) if with_total else None
    status = engine.lib.pa_tool_exclusive_scan_u32(engine.ctx, d_in.data_ptr(), d_out.data_ptr(), n, d_total.data_ptr() if with_total else None)
    assert status == _capi.PA_OK, f"status {status}: {_capi.last_error(engine.lib)}"
    out = _to_host(d_out, np.uint32)
    assert np.array_equal(out[n:], np.full(PAD, FILL32)), "written past n"
    if not in_place:
        assert np.array_equal(_to_host(d_in, np.uint32), np.concatenate([v, np.full(PAD, FILL32)])), "the input changed"
    total = None
    if with_total:
        slot = _to_host(d_total, np.uint64)
        assert np.array_equal(slot[1:], np.full(PAD, TOTAL_FILL)), "written past the total"
        total = int(slot[0])
    return out[:n], total


def _scan_expected(v: np.ndarray) -> tuple[np.ndarray, int, np.ndarray]:
    """(prefixes modulo 2^32, exact total, exact prefixes)."""
    wide = v.astype(np.uint64)
    exact = np.cumsum(wide, dtype=np.uint64) - wide
    return (exact & np.uint64(0xFFFFFFFF)).astype(np.uint32), int(wide.sum(dtype=np.uint64)), exact


def _check_scan(engine, v, **how):
    want, want_total, _ = _scan_expected(v)
    got, total = _scan(engine, v, **how)
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), f"n = {len(v)}, {how}: {len(bad)} prefixes differ, first at {bad[:4]}"
    if how.get("with_total", True):
        assert total == want_total, f"n = {len(v)}, {how}: total {total} (= 2^32 * {total >> 32} + {total & 0xFFFFFFFF}), exact {want_total}"


SCAN_SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, ROUND * TILE - 1, ROUND * TILE, ROUND * TILE + 1]


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes(engine, n):
    """Around a thread's 8 values, a tile of 2048 and a round of 256 tiles (the last size is the second round of
    ``scan_sums_kernel``), with values small enough that nothing wraps."""
    rng = np.random.default_rng([20270, n])
    v = rng.integers(0, 1000, size=n, dtype=np.uint32)
    assert int(v.sum(dtype=np.uint64)) < 2**32 and (n < 7 or len(np.unique(v)) > 1)
    _check_scan(engine, v)
    _check_scan(engine, v, with_total=False)  # a null total pointer, for n = 0 as well
    if n == 0:
        assert _scan(engine, v)[1] == 0  # the pattern in the total's slot became 0


@pytest.mark.parametrize("n", [2049, ROUND * TILE + 1])
def test_scan_in_place(engine, n):
    """``d_out == d_in``, as the sort scans its histogram."""
    rng = np.random.default_rng([20271, n])
    v = rng.integers(0, 1000, size=n, dtype=np.uint32)
    _check_scan(engine, v, in_place=True)
    _check_scan(engine, v, in_place=True, with_total=False)


def _assert_tiles_fit_and_total_does_not(v: np.ndarray) -> None:
    assert len(v) % TILE == 0
    tile_sums = v.astype(np.uint64).reshape(-1, TILE).sum(axis=1, dtype=np.uint64)
    assert int(tile_sums.max()) < 2**32  # every tile sum is a 32-bit number, as the contract asks ...
    assert int(tile_sums.sum(dtype=np.uint64)) >= 2**32  # ... and their sum is not
    _, _, exact = _scan_expected(v)
    assert int(exact.max()) >= 2**32  # the prefixes wrap, as documented: they are compared element by element, modulo 2^32


def test_scan_total_is_exact_beyond_32_bits(engine):
    """Three tiles of 2^21 - 1: each tile sum is 2^32 - 2048, the total 3 * 2^32 - 6144.  The prefixes wrap; the total,
    added up in 64 bits from the tiles' 32-bit sums, does not."""
    v = np.full(3 * TILE, 2**21 - 1, dtype=np.uint32)
    _assert_tiles_fit_and_total_does_not(v)
    assert int(v[:TILE].sum(dtype=np.uint64)) == 2**32 - 2048
    want, want_total, _ = _scan_expected(v)
    assert want_total == 3 * 2**32 - 6144
    got, total = _scan(engine, v)
    assert np.array_equal(got, want)
    assert total == want_total, f"total {total} = 2^32 * {total >> 32} + {total & 0xFFFFFFFF}; exact: 3 * 2^32 - 6144"
    _check_scan(engine, v, in_place=True)


def test_scan_total_is_exact_across_rounds(engine):
    """300 tiles of values just below 2^21: the total, about 300 * 2^32, is carried over the boundary between the first
    256 tile sums and the rest."""
    rng = np.random.default_rng(20272)
    v = rng.integers(2**21 - 64, 2**21, size=300 * TILE, dtype=np.uint32)
    _assert_tiles_fit_and_total_does_not(v)
    assert len(v) // TILE > ROUND and int(v.astype(np.uint64)[: ROUND * TILE].sum(dtype=np.uint64)) >= 2**32
    assert _scan_expected(v)[1] >> 32 == 299
    _check_scan(engine, v)
    _check_scan(engine, v, in_place=True)
