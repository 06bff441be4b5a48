"""The MSA pair path on the MI355X at the cases of tests/msa_cases.py: every plane count of both pair kernels, the pack
kernel's column mask under rows padded with residues, the seams of the tile, the stage and the column split, ranges off
the tile grid, outputs that held a pattern and are fenced by guard words, and the refusals.  Every comparison is of
integers, exactly: with ``tests/msa_checker.py`` (unweighted), ``tests/bootstrap_cases.py`` and the host twin (weighted),
and for the planes with the numpy restatement of the pack.  The calls go through ``engine.lib``: ``HipEngine.msa_upload``
derives table and ``bits`` from a histogram and pads with '-', ``msa_pair_counts`` allocates its own outputs."""

from __future__ import annotations

import numpy as np
import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd import engine as engine_mod
from pyani_plus_amd.engine import HipEngine
from tests import msa_cases as cases

pytestmark = pytest.mark.gpu

CHUNK_ROWS = 37  # rows per upload: no boundary but the first is a multiple of 64


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def compute_units(engine) -> int:
    return int(engine.device_info()["compute_units"])


def _device(engine, values: np.ndarray):
    return engine.torch.from_numpy(np.array(values, dtype=np.uint32, order="C").view(np.int32)).to(engine.device)


def _host(engine, tensor) -> np.ndarray:
    engine.sync()
    return tensor.cpu().numpy().view(np.uint32)


class Packed:
    """A case's planes on the device, in a buffer that held PLANE_FILL and is one stage longer than the planes."""

    def __init__(self, engine, c: cases.Case, chunk_rows: int = CHUNK_ROWS):
        n, n_pad, P = c.n_rows, cases.n_pad_of(c.n_rows), c.bits + 1
        self.words = int(engine.lib.pa_msa_plane_words(n, c.n_cols, c.bits))
        assert self.words == c.n_words * P * n_pad
        self.planes = _device(engine, np.full(self.words + cases.CHUNK * P * n_pad, cases.PLANE_FILL, dtype=np.uint32))
        nongap = np.zeros(n + cases.GUARD_WORDS, dtype=np.uint32)
        nongap[n:] = cases.GUARD
        self.nongap = _device(engine, nongap)
        for r0 in range(0, n, chunk_rows):
            r1 = min(n, r0 + chunk_rows)
            d_rows = _device_bytes(engine, c.padded[r0:r1])
            status = engine.lib.pa_msa_pack(engine.ctx, d_rows.data_ptr(), c.stride, r0, r1 - r0, n, c.n_cols, c.alphabet.code.ctypes.data, c.bits,
                                            self.planes.data_ptr(), self.nongap.data_ptr())  # fmt: skip
            engine._check(status, "pa_msa_pack")
            engine.sync()  # d_rows is freed by the next iteration


def _device_bytes(engine, rows: np.ndarray):
    return engine.torch.from_numpy(np.array(rows, dtype=np.uint8, order="C")).to(engine.device)


_packed: dict = {}


def packed(engine, name: str) -> Packed:
    """A case's planes, packed once for the tests of this module that read them."""
    if name not in _packed:
        _packed.clear()  # one alignment on the device at a time
        _packed[name] = Packed(engine, cases.case(name))
    return _packed[name]


# ---------------------------------------------------------------- the pack
def _pack_cases() -> list:
    return [c.name for c in cases.cases() if c.names & ({"alphabet", "weighted", "many_tiles", "slices3"} | {f"cols{n}" for n in cases.COL_SEAMS})]


@pytest.mark.parametrize("name", _pack_cases())
def test_pack_of_rows_padded_with_residues(engine, name):
    """All 16 alphabets and the column seams: the bytes at and past n_cols are residues, and no plane shows them."""
    c = cases.case(name)
    assert not (c.padded[:, c.n_cols :] == cases.GAP).any()
    want_planes, want_nongap = cases.pack(c)
    for chunk_rows in (CHUNK_ROWS, 100) if c.n_rows > CHUNK_ROWS else (CHUNK_ROWS,):
        assert chunk_rows % cases.TILE
        p = Packed(engine, c, chunk_rows)
        got = _host(engine, p.planes).reshape(want_planes.shape)
        n, nw = c.n_rows, c.n_words
        for plane in range(c.bits + 1):
            np.testing.assert_array_equal(got[:nw, plane, :n], want_planes[:nw, plane, :n], err_msg=f"plane {plane}")
        assert (got[:nw, :, n:] == cases.PLANE_FILL).all(), "rows past the alignment were written"
        assert (got[nw:] == cases.PLANE_FILL).all(), "words past the planes were written"
        nongap = _host(engine, p.nongap)
        np.testing.assert_array_equal(nongap[:n], want_nongap)
        np.testing.assert_array_equal(nongap[:n], (c.rows != cases.GAP).sum(axis=1))
        assert (nongap[n:] == cases.GUARD).all()


# ---------------------------------------------------------------- the pair counts
def _outputs(engine, call: cases.Call):
    cells = call.shape[0] * call.shape[1]
    out = []
    for fill in (cases.PREFILL_M, cases.PREFILL_B):
        host = np.full(cells + cases.GUARD_WORDS, fill, dtype=np.uint32)
        host[cells:] = cases.GUARD
        out.append(_device(engine, host))
    return out


def _run_calls(engine, name: str):
    c = cases.case(name)
    p = packed(engine, name)
    want = cases.expected(name)
    for call, (want_m, want_b) in zip(c.calls, want):
        cells = call.shape[0] * call.shape[1]
        match, both = _outputs(engine, call)
        status = engine.lib.pa_msa_pair_counts(engine.ctx, p.planes.data_ptr(), c.n_rows, c.n_cols, c.bits, call.q0, call.q1, call.s0, call.s1, call.symmetric,
                                               match.data_ptr(), both.data_ptr())  # fmt: skip
        engine._check(status, "pa_msa_pair_counts")
        for got, wanted, what in ((_host(engine, match), want_m, "M"), (_host(engine, both), want_b, "B")):
            assert (got[cells:] == cases.GUARD).all(), f"{what} of {call}: the words past the output's end were written"
            np.testing.assert_array_equal(got[:cells].reshape(call.shape), wanted, err_msg=f"{what} of {call}")
    return c


@pytest.mark.parametrize("alpha", [a.name for a in cases.ALPHABETS])
def test_pair_counts_of_every_alphabet(engine, alpha):
    """msa_pairs_kernel<P> for P = bits + 1 = 2 .. 9, at both ends of each: the symmetric form over two tiles (the mirror)
    and the ranges off the tile grid."""
    c = _run_calls(engine, f"alpha_{alpha}")
    assert c.bits + 1 == int(alpha[4]) + 1 and len(c.calls) == 8 and sum(0 in call.shape for call in c.calls) == 2


@pytest.mark.parametrize("name", [c.name for c in cases.unweighted_cases() if c.name.startswith(("rows", "cols", "many"))])
def test_pair_counts_at_the_row_and_column_seams(engine, compute_units, name):
    c = _run_calls(engine, name)
    for call in c.calls:
        assert cases.split_columns(cases.n_tiles(call), c.n_words, compute_units).splits == 1
    if c.n_cols == 0:
        assert all(not m.any() and not b.any() for m, b in cases.expected(name))  # no column: zeros


@pytest.mark.parametrize("name", [c.name for c in cases.unweighted_cases() if c.name.startswith("slices")])
def test_pair_counts_under_the_column_split(engine, compute_units, name):
    """Outputs that held a pattern: a split call clears them itself before its atomics.  The path is the one the case
    names on this device: from the restated split and the device's own count of compute units."""
    c = cases.case(name)
    named = int(name[6])
    for call in c.calls:
        split = cases.split_columns(cases.n_tiles(call), c.n_words, compute_units)
        print(f"{name} {call}: {compute_units} CUs, {cases.n_tiles(call)} tiles, {c.n_words} words -> {split}")
        assert split.splits == named and (named == 1 or split.splits >= 2)
        if named == 3:
            assert (c.n_words - 2 * split.words_per_split) % cases.CHUNK  # the last slice ends in the middle of a stage
    _run_calls(engine, name)


# ---------------------------------------------------------------- the weighted counts
@pytest.mark.parametrize("name", [c.name for c in cases.weighted_cases()])
def test_weighted_counts_of_the_other_plane_counts(engine, name):
    """msa_boot_pairs_kernel<P> for bits 3, 5, 6, 7 (tests/test_gpu_bootstrap.py has the rest) at 65 rows x 257 columns:
    two tiles and the mirror, one whole stage and one word of the next; drawn weights and one of 255."""
    c = cases.case(name)
    p = packed(engine, name)
    reps, n = len(c.weights), c.n_rows
    cells = reps * n * n
    match, both = _outputs(engine, cases.Call(0, reps * n, 0, n, 0))
    w = np.ascontiguousarray(c.weights)
    status = engine.lib.pa_msa_boot_counts(engine.ctx, p.planes.data_ptr(), n, c.n_cols, c.bits, w.ctypes.data, reps, match.data_ptr(), both.data_ptr())
    engine._check(status, "pa_msa_boot_counts")
    twin = engine_mod.msa_boot_counts_host(c.padded, c.n_cols, w)  # the twin reads the padded rows too
    for got, wanted, host in zip((_host(engine, match), _host(engine, both)), cases.expected(name), twin):
        assert (got[cells:] == cases.GUARD).all()
        np.testing.assert_array_equal(got[:cells].reshape(reps, n, n), wanted)
        np.testing.assert_array_equal(host, wanted)


# ---------------------------------------------------------------- the refusals
def test_the_refusals_of_pack_and_pair_counts(engine):
    c = cases.case("cols33_bits4")
    n, n_cols, bits = c.n_rows, c.n_cols, c.bits
    good = packed(engine, c.name)
    lib, ctx = engine.lib, engine.ctx
    d_rows = _device_bytes(engine, np.concatenate([c.padded, c.padded]))  # room behind the rows for the calls that shift them
    planes, nongap = good.planes.data_ptr(), _device(engine, np.zeros(n, dtype=np.uint32))
    code = c.alphabet.code

    def pack(message, *, rows=d_rows.data_ptr(), stride=c.stride, row0=0, count=n, n_rows=n, cols=n_cols, table=code, b=bits):
        status = lib.pa_msa_pack(ctx, rows, stride, row0, count, n_rows, cols, table.ctypes.data, b, planes, nongap.data_ptr())
        assert (status, _capi.last_error(lib)) == (_capi.PA_E_INVALID, f"pa_msa_pack: {message}")

    pack("bits must be 1 to 8, not 0", b=0)
    pack("bits must be 1 to 8, not 9", b=9)
    pack("row stride 48 must be a multiple of 32 and at least 64", stride=48)
    pack("row stride 32 must be a multiple of 32 and at least 64", stride=32)
    pack("rows must be 16-byte aligned", rows=d_rows.data_ptr() + 8)
    pack("rows [3, 9) past 6 rows", row0=3)
    pack(f"{1 << 32} columns (at most 2^32 - 1)", cols=1 << 32)
    gap_coded = code.copy()
    gap_coded[cases.GAP] = 1
    pack("the gap '-' must have code 0", table=gap_coded)
    wide = code.copy()
    wide[65] = 16
    pack("byte 65 has code 16, not below 2^4", table=wide)
    pack("byte 248 has code 8, not below 2^3", b=3)  # residues 241 .. 255 have the codes 1 .. 15
    pack("null argument", rows=None)

    match, both = _outputs(engine, cases.Call(0, n, 0, n, 0))

    def pairs(message, *, q=(0, n), s=(0, n), symmetric=0, n_rows=n, cols=n_cols, b=bits, d_planes=planes):
        status = lib.pa_msa_pair_counts(ctx, d_planes, n_rows, cols, b, q[0], q[1], s[0], s[1], symmetric, match.data_ptr(), both.data_ptr())
        assert (status, _capi.last_error(lib)) == (_capi.PA_E_INVALID, f"pa_msa_pair_counts: {message}")

    pairs("bits must be 1 to 8, not 0", b=0)
    pairs("bits must be 1 to 8, not 9", b=9)
    pairs("ranges [0, 7) x [0, 6) outside 6 rows", q=(0, 7))
    pairs("ranges [0, 6) x [2, 7) outside 6 rows", s=(2, 7))
    pairs("ranges [4, 3) x [0, 6) outside 6 rows", q=(4, 3))
    pairs("ranges [0, 6) x [6, 5) outside 6 rows", s=(6, 5))
    pairs("the symmetric form needs equal query and subject ranges", q=(0, 5), s=(1, 6), symmetric=1)
    pairs("the symmetric form needs equal query and subject ranges", q=(0, 6), s=(0, 5), symmetric=1)
    pairs(f"{1 << 32} columns (at most 2^32 - 1)", cols=1 << 32)
    pairs("null argument", d_planes=None)
    for buffer in (match, both):  # no refused call wrote anything
        got = _host(engine, buffer)
        assert (got[: n * n] == got[0]).all() and got[0] in (cases.PREFILL_M, cases.PREFILL_B) and (got[n * n :] == cases.GUARD).all()

    # the context still works: the same rows packed again beside the planes of before, and counted
    _packed.clear()
    again = Packed(engine, c)
    np.testing.assert_array_equal(_host(engine, again.planes), _host(engine, good.planes))
    _packed[c.name] = again
    _run_calls(engine, c.name)
