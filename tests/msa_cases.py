"""The edge cases of the MSA pair path (``msa.hip``, ``msa_boot.hip``, ``msa_tile_dev.h``) and a numpy emulation of its
plane arithmetic.

What is meant by a result is ``tests/msa_checker.py`` (unweighted) and ``tests/bootstrap_cases.py`` (weighted): counts of
bytes, written from the definitions.  This module builds the alignments on which a kernel can differ from them, and
restates *how* the kernels compute, so that ``tests/test_msa_cases.py`` can show without a GPU that each case tells a
wrong kernel from a right one:

* ``split_columns`` restates ``msa_tile::split_columns`` as a function of (blocks, words, compute units).
* ``pack`` lays the planes out as ``msa_pack_kernel`` does, ``emulate`` goes through the tiles, slices and stages of the
  pair kernels with the per-word arithmetic of ``eq_word`` / ``both_word``, writes into pre-filled outputs and mirrors.
  Both take a named fault (``FAULTS``): one wrong line of a kernel each.

Every alignment is written by construction: a seeded fill, then the rows and columns that a kernel can get wrong are
placed over it (``build_rows``), then every residue byte of the alphabet is laid down once, so that ``msa_code_table``
returns exactly the ``bits`` the alphabet names.  A case too small to hold its whole alphabet (one row of one column)
keeps the alphabet's code table all the same: the tests hand table and ``bits`` to ``pa_msa_pack`` themselves.  The row
buffers are padded past ``n_cols`` with residue bytes, never with '-': what is expected comes from the first ``n_cols``
columns alone."""

from __future__ import annotations

import functools
import re
import zlib
from pathlib import Path
from typing import NamedTuple

import numpy as np

from tests import bootstrap_cases

ROOT = Path(__file__).resolve().parent.parent
TILE_HEADER = ROOT / "pyani_plus_amd" / "csrc" / "msa_tile_dev.h"
API_HEADER = ROOT / "include" / "pyani_hip.h"

GAP = ord("-")
TILE = 64  # kTile
THREADS = 256  # kThreads
CHUNK = 8  # kChunk: words of a stage through LDS
MAX_BITS = 8  # kMaxBits
BOOT_BATCH = 32  # PA_MSA_BOOT_BATCH
NOMINAL_CUS = 256  # for the emulation on a CPU; a GPU test passes its device's own count

PREFILL_M, PREFILL_B = 0xA5A5A5A5, 0x3C3C3C3C  # what the outputs hold before a call
GUARD = 0x5EED5EED  # the 64 words past an output's end
GUARD_WORDS = 64
PLANE_FILL = 0xFFFFFFFF  # the plane buffer before the pack, and the stage of words past its end: every column the highest code


def kernel_constants() -> dict:
    """kTile, kThreads, kChunk, kMaxBits and PA_MSA_BOOT_BATCH as the two headers state them."""
    tile, api = TILE_HEADER.read_text(), API_HEADER.read_text()

    def find(pattern: str, text: str, what: str) -> int:
        m = re.search(pattern, text)
        assert m, f"{what} no longer has the form tests/msa_cases.py reads ({pattern!r}): change tests/msa_cases.py too"
        return int(m.group(1))

    return {
        "TILE": find(r"constexpr int kTile = (\d+);", tile, "kTile"),
        "THREADS": find(r"constexpr int kThreads = (\d+);", tile, "kThreads"),
        "CHUNK": find(r"constexpr int kChunk = (\d+);", tile, "kChunk"),
        "MAX_BITS": find(r"constexpr uint32_t kMaxBits = (\d+);", tile, "kMaxBits"),
        "BOOT_BATCH": find(r"#define PA_MSA_BOOT_BATCH (\d+)", api, "PA_MSA_BOOT_BATCH"),
    }


class ColumnSplit(NamedTuple):
    splits: int
    words_per_split: int


def split_columns(blocks: int, n_words: int, compute_units: int) -> ColumnSplit:
    """``msa_tile::split_columns``: about 8 blocks per CU, each slice at least 64 words and a whole number of stages."""
    want = 8 * compute_units
    splits = 1 if blocks >= want else (want + blocks - 1) // blocks
    splits = max(1, min(splits, (n_words + 63) // 64, 65535))
    wps = (n_words + splits - 1) // splits
    wps = (wps + CHUNK - 1) // CHUNK * CHUNK
    if wps == 0:
        wps = CHUNK
    splits = (n_words + wps - 1) // wps
    return ColumnSplit(max(1, splits), wps)


def n_words_of(n_cols: int) -> int:
    return (n_cols + 31) // 32


def n_pad_of(n_rows: int) -> int:
    return (n_rows + TILE - 1) // TILE * TILE


def n_tiles(call: "Call") -> int:
    tq, ts = (call.q1 - call.q0 + TILE - 1) // TILE, (call.s1 - call.s0 + TILE - 1) // TILE
    return tq * (tq + 1) // 2 if call.symmetric else tq * ts


def popcount(x: np.ndarray) -> np.ndarray:
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.uint32)
    table = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)
    return table[np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (4,))].sum(axis=-1, dtype=np.uint32)


# ---------------------------------------------------------------- alphabets
class Alphabet(NamedTuple):
    name: str  # bits4_low, bits4_high
    bits: int
    residues: tuple  # residue bytes in byte order; residue i has code i + 1, the gap code 0
    code: np.ndarray  # uint8[256]

    @property
    def top(self) -> int:
        """The residue byte of the highest code."""
        return self.residues[-1]


_NON_GAP = tuple(b for b in range(256) if b != GAP)


def _alphabet(bits: int, end: str) -> Alphabet:
    count = (max(1, 1 << (bits - 1))) if end == "low" else (1 << bits) - 1
    residues = _NON_GAP[:count] if end == "low" else _NON_GAP[-count:]  # from byte 0 up, or down from byte 255
    code = np.zeros(256, dtype=np.uint8)
    for i, b in enumerate(residues):
        code[b] = i + 1
    code.setflags(write=False)
    return Alphabet(f"bits{bits}_{end}", bits, residues, code)


ALPHABETS = tuple(_alphabet(bits, end) for bits in range(1, MAX_BITS + 1) for end in ("low", "high"))


def alphabet(name: str) -> Alphabet:
    return next(a for a in ALPHABETS if a.name == name)


def plane_pairs(alpha: Alphabet) -> dict:
    """plane p -> two residue codes that differ in bit p alone, for every plane that has such a pair."""
    top, out = len(alpha.residues), {}
    for p in range(alpha.bits):
        for x in range(1, top + 1):
            y = x ^ (1 << p)
            if 1 <= y <= top:
                out[p] = (x, y)
                break
    return out


# ---------------------------------------------------------------- rows
def feature_columns(alpha: Alphabet) -> list:
    """The columns placed in rows 0 and 1, as (code of row 0, code of row 1): for every plane two residues that only this
    plane separates; the residue whose code is that plane's bit alone against a gap, on either side (the gap is code 0:
    here too only this plane separates them, and for the smallest alphabet of a ``bits`` its top plane has no other
    pair); a residue under a residue that differs in every plane; both rows gap."""
    top = len(alpha.residues)
    cols = [pair for _p, pair in sorted(plane_pairs(alpha).items())]
    for p in range(alpha.bits):
        if (1 << p) <= top:
            cols += [(1 << p, 0), (0, 1 << p)]
    cols += [(0, 0), (0, 0), (top, 0), (top, top)]
    return cols


def build_rows(alpha: Alphabet, n: int, n_cols: int, seed: int, *, gap_column: bool = False) -> np.ndarray:
    """n x n_cols bytes.  A seeded fill (12 % gaps), then, as far as the shape has room:
    rows 0 and 1 end in ``feature_columns``; rows 2 and 3 are one row without a gap; row 4 is all gap; row 5 is the
    highest code alone; with ``gap_column`` one column is gap in every row; then every residue byte is laid down once in
    the cells that none of these own."""
    rng = np.random.default_rng(seed)
    res = np.array(alpha.residues, dtype=np.uint8)
    byte_of = np.concatenate([[GAP], res]).astype(np.uint8)  # code -> byte
    rows = res[rng.integers(len(res), size=(n, n_cols))]
    rows[rng.random((n, n_cols)) < 0.12] = GAP
    owned = np.zeros((n, n_cols), dtype=bool)
    feats = feature_columns(alpha)[:n_cols]
    if n >= 2:
        at = n_cols - len(feats)
        for k, (a, b) in enumerate(feats):
            rows[0, at + k], rows[1, at + k] = byte_of[a], byte_of[b]
        owned[0:2, at:] = True
    if n >= 4:
        rows[2] = res[rng.integers(len(res), size=n_cols)]
        rows[3] = rows[2]
        owned[2:4] = True
    if n >= 5:
        rows[4] = GAP
        owned[4] = True
    if n >= 6:
        rows[5] = alpha.top
        owned[5] = True
    column = gap_column_of(alpha, n_cols) if gap_column else None
    if column is not None:
        rows[:, column] = GAP
        owned[:, column] = True
    free = np.flatnonzero(~owned.ravel())[: len(res)]
    rows.reshape(-1)[free] = res[: len(free)]
    return rows


def gap_column_of(alpha: Alphabet, n_cols: int):
    """The column that ``build_rows(gap_column=True)`` makes all gap: in the middle of what ``feature_columns`` leaves."""
    k = len(feature_columns(alpha))
    return (n_cols - k) // 2 if n_cols > k else None


def padded_rows(alpha: Alphabet, rows: np.ndarray, extra: int, seed: int) -> np.ndarray:
    """The rows in a buffer of stride ``32 * ceil(n_cols / 32) + extra`` (at least 32), filled past n_cols with residue
    bytes: the highest code first, then drawn."""
    n, n_cols = rows.shape
    stride = max(32, n_words_of(n_cols) * 32) + extra
    rng = np.random.default_rng(seed ^ 0x5A5A)
    res = np.array(alpha.residues, dtype=np.uint8)
    out = res[rng.integers(len(res), size=(n, stride))]
    out[:, n_cols : n_cols + 2] = alpha.top
    out[:, :n_cols] = rows
    assert not (out[:, n_cols:] == GAP).any()
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------- cases
class Call(NamedTuple):
    q0: int
    q1: int
    s0: int
    s1: int
    symmetric: int

    @property
    def shape(self) -> tuple:
        return (self.q1 - self.q0, self.s1 - self.s0)


class Case(NamedTuple):
    name: str
    alphabet: Alphabet
    rows: np.ndarray  # n x n_cols: the columns that count
    padded: np.ndarray  # n x stride: what is uploaded
    calls: tuple  # of Call (unweighted cases)
    names: frozenset  # the seams and features the case is there for
    weights: object = None  # R x n_cols uint8 (weighted cases)

    @property
    def bits(self) -> int:
        return self.alphabet.bits

    @property
    def n_rows(self) -> int:
        return self.rows.shape[0]

    @property
    def n_cols(self) -> int:
        return self.rows.shape[1]

    @property
    def n_words(self) -> int:
        return n_words_of(self.rows.shape[1])

    @property
    def stride(self) -> int:
        return self.padded.shape[1]


ROW_SEAMS = (1, 2, 63, 64, 65, 128, 129)
COL_SEAMS = (0, 1, 31, 32, 33, 255, 256, 257)
MANY_TILE_ROWS, MANY_TILE_COLS, MANY_TILES = 1100, 32, 171
SPLIT_COLS = {64 * 32: 1, 64 * 32 + 1: 2, 4161: 3}  # columns -> slices; 4161 columns are 131 words: 48 + 48 + 35, the last ends mid-stage
SEAM_BITS = (1, 4, 8)
ALPHA_ROWS, ALPHA_COLS = 70, 75
WEIGHTED_BITS = (3, 5, 6, 7)
WEIGHTED_ROWS, WEIGHTED_COLS = 65, 257


def _sym(n: int) -> Call:
    return Call(0, n, 0, n, 1)


def _off_grid(n: int) -> tuple:
    """Ranges off the tile grid of an alignment of n >= 70 rows."""
    return (
        Call(3, n, 5, n, 0),  # q0 and s0 no multiples of 64, both end at the last row
        Call(n - 4, n - 3, 0, n, 0),  # nq = 1
        Call(0, n, n - 1, n, 0),  # ns = 1, the last row
        Call(10, 10, 0, n, 0),  # empty
        Call(0, n, 7, 7, 0),
        Call(1, n - 4, 1, n - 4, 0),  # square, equal ranges, yet not the symmetric form
        Call(0, n - 5, 5, n, 0),  # square over different rows
    )


def _case(name, alpha, n, n_cols, calls, names, *, gap_column=False, extra=0, weights=None) -> Case:
    seed = zlib.crc32(name.encode())
    rows = build_rows(alpha, n, n_cols, seed, gap_column=gap_column)
    padded = padded_rows(alpha, rows, extra, seed)
    rows.setflags(write=False)
    padded.setflags(write=False)
    if weights is not None:
        weights.setflags(write=False)
    return Case(name, alpha, rows, padded, tuple(calls), frozenset(names), weights)


def _heavy(n_cols: int, column: int) -> np.ndarray:
    """One weight of 255, the rest of the n_cols draws one each on the columns after it."""
    w = np.zeros((1, n_cols), dtype=np.uint8)
    w[0, column] = 255
    w[0, [(column + 1 + k) % n_cols for k in range(n_cols - 255)]] = 1
    return w


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    extras = (0, 32, 96)  # strides: as small as allowed, and larger than needed
    for alpha in ALPHABETS:
        out.append(_case(f"alpha_{alpha.name}", alpha, ALPHA_ROWS, ALPHA_COLS, (_sym(ALPHA_ROWS),) + _off_grid(ALPHA_ROWS),
                         {"alphabet", "features", "ranges"}, extra=extras[len(out) % 3]))  # fmt: skip
    for bits in SEAM_BITS:
        alpha = alphabet(f"bits{bits}_high")
        for n in ROW_SEAMS:
            calls = [_sym(n), Call(0, n, 0, n, 0)] + ([Call(1, n, 0, n - 1, 0)] if n > 2 else [])
            out.append(_case(f"rows{n}_bits{bits}", alpha, n, 40, calls, {f"rows{n}"}, gap_column=True, extra=extras[len(out) % 3]))
        for n_cols in COL_SEAMS:
            out.append(_case(f"cols{n_cols}_bits{bits}", alpha, 6, n_cols, (_sym(6), Call(1, 6, 0, 5, 0)), {f"cols{n_cols}"}, gap_column=True,
                             extra=extras[len(out) % 3]))  # fmt: skip
        for n_cols, slices in SPLIT_COLS.items():
            out.append(_case(f"slices{slices}_rows6_bits{bits}", alpha, 6, n_cols, (_sym(6), Call(1, 6, 0, 5, 0)), {f"slices{slices}"}, gap_column=True,
                             extra=extras[len(out) % 3]))  # fmt: skip
            out.append(_case(f"slices{slices}_rows65_bits{bits}", alpha, 65, n_cols, (_sym(65),), {f"slices{slices}", "mirror"}, gap_column=True))
    out.append(_case("many_tiles", alphabet("bits4_high"), MANY_TILE_ROWS, MANY_TILE_COLS,
                     (_sym(MANY_TILE_ROWS), Call(1000, MANY_TILE_ROWS, 3, 200, 0)), {"many_tiles"}, gap_column=True))  # fmt: skip
    for bits in WEIGHTED_BITS:
        for end in ("low", "high"):
            alpha = alphabet(f"bits{bits}_{end}")
            drawn = bootstrap_cases.weights(bits, WEIGHTED_COLS, 0, 2).astype(np.uint8)
            w = np.ascontiguousarray(np.vstack([drawn, _heavy(WEIGHTED_COLS, WEIGHTED_COLS - 1)]))  # 255 on the last column: the one valid bit of the last, partial stage
            out.append(_case(f"weighted_{alpha.name}", alpha, WEIGHTED_ROWS, WEIGHTED_COLS, (), {"weighted"}, extra=extras[len(out) % 3], weights=w))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def unweighted_cases() -> tuple:
    return tuple(c for c in cases() if c.weights is None)


def weighted_cases() -> tuple:
    return tuple(c for c in cases() if c.weights is not None)


# ---------------------------------------------------------------- the kernels, restated, with their wrong variants
FAULTS = tuple(f"drop_plane{p}" for p in range(MAX_BITS)) + (
    "eq_unmasked",  # eq = ~d, without the query's non-gap word
    "both_query_only",  # both = ng_q
    "pack_no_valid",  # the pack reads the bytes past n_cols as columns
    "stage_past_w_hi",  # words at or past a slice's w_hi staged as memory has them
    "drop_partial_stage",  # the stage loop stops at the last whole stage
    "no_zero",  # the outputs not cleared before a split call (or one without words)
    "mirror_boundary",  # the mirror takes c < r - r % kTile - kTile
    "weight_shift",  # weighted: popcount(eq & W_beta) << (beta + 1)
)


def pack(c: Case, fault: str | None = None) -> tuple:
    """``(planes, nongap)`` as ``msa_pack_kernel`` leaves them in a buffer that held PLANE_FILL: planes[w, p, row] for
    n_words + CHUNK words (the last CHUNK are past the buffer's end: whatever memory holds, here PLANE_FILL) and n_pad
    rows; nongap[row]."""
    assert fault in (None, "pack_no_valid")
    n, n_cols, bits, nw = c.n_rows, c.n_cols, c.bits, c.n_words
    planes = np.full((nw + CHUNK, bits + 1, n_pad_of(n)), PLANE_FILL, dtype=np.uint32)
    nongap = np.zeros(n, dtype=np.uint32)
    if nw:
        codes = c.alphabet.code[c.padded[:, : nw * 32]].astype(np.uint64)
        if fault != "pack_no_valid":
            codes[:, n_cols:] = 0
        shifts = np.arange(32, dtype=np.uint64)
        for p in range(bits + 1):
            bit = ((codes >> np.uint64(p)) & np.uint64(1)) if p < bits else (codes != 0).astype(np.uint64)
            planes[:nw, p, :n] = (bit.reshape(n, nw, 32) << shifts).sum(axis=2).astype(np.uint32).T
        nongap = popcount(planes[:nw, bits, :n]).sum(axis=0, dtype=np.uint32)
    return planes, nongap


def weight_planes(weights: np.ndarray, n_words: int) -> np.ndarray:
    """wplanes[rep, w, beta] as ``boot_weight_planes_kernel`` makes them: bit j is bit beta of w[32 w + j]."""
    reps, n_cols = weights.shape
    w = np.zeros((reps, n_words * 32), dtype=np.uint64)
    w[:, :n_cols] = weights
    shifts = np.arange(32, dtype=np.uint64)
    out = np.zeros((reps, n_words, MAX_BITS), dtype=np.uint32)
    for beta in range(MAX_BITS):
        out[:, :, beta] = (((w >> np.uint64(beta)) & np.uint64(1)).reshape(reps, n_words, 32) << shifts).sum(axis=2).astype(np.uint32)
    return out


def _tile_counts(planes, bits, q_rows, s_rows, w_lo, w_hi, fault, wplanes=None, nb=0):
    """One block: the 64 x 64 counts of a tile over the words [w_lo, w_hi).  q_rows, s_rows: 64 plane rows each, -1 for a
    row outside the range (staged as zero)."""
    words = []
    for wc in range(w_lo, w_hi, CHUNK):
        if fault == "drop_partial_stage" and wc + CHUNK > w_hi:
            break
        words += [w for w in range(wc, wc + CHUNK) if w < w_hi or fault == "stage_past_w_hi"]
    m, b = np.zeros((TILE, TILE), dtype=np.uint32), np.zeros((TILE, TILE), dtype=np.uint32)
    if not words:
        return m, b
    words = np.array(words)
    q = np.where(q_rows >= 0, planes[words][:, :, np.maximum(q_rows, 0)], np.uint32(0))  # [words, P, 64]
    s = np.where(s_rows >= 0, planes[words][:, :, np.maximum(s_rows, 0)], np.uint32(0))
    d = np.zeros((len(words), TILE, TILE), dtype=np.uint32)
    for p in range(bits):
        if fault != f"drop_plane{p}":
            d |= q[:, p, :, None] ^ s[:, p, None, :]
    ng_q, ng_s = q[:, bits, :, None], s[:, bits, None, :]
    eq = ~d if fault == "eq_unmasked" else ~d & ng_q
    both = np.broadcast_to(ng_q, d.shape) if fault == "both_query_only" else ng_q & ng_s
    if wplanes is None:
        return popcount(eq).sum(axis=0, dtype=np.uint32), popcount(both).sum(axis=0, dtype=np.uint32)
    inside = words < w_hi  # the weight words have a staging of their own: zero at and past w_hi
    for beta in range(nb):
        W = np.where(inside, wplanes[np.minimum(words, len(wplanes) - 1), beta], np.uint32(0))[:, None, None]
        shift = np.uint32(beta + 1 if fault == "weight_shift" else beta)
        m += popcount(eq & W).sum(axis=0, dtype=np.uint32) << shift
        b += popcount(both & W).sum(axis=0, dtype=np.uint32) << shift
    return m, b


def _mirror(out: np.ndarray, fault) -> None:
    n = out.shape[0]
    for r in range(n):
        bound = (r // TILE) * TILE
        if fault == "mirror_boundary":
            bound = (r - r % TILE - TILE) & 0xFFFFFFFF  # uint32 arithmetic
        bound = min(bound, n)
        out[r, :bound] = out[:bound, r]


def _pairs(planes, bits, n_words, call: Call, splits: ColumnSplit, fault, match, both, wplanes=None, nb=0) -> None:
    """The grid of one launch on one matrix: every tile and slice, stored or added; then the mirror."""
    nq, ns = call.shape
    tq, ts = (nq + TILE - 1) // TILE, (ns + TILE - 1) // TILE
    tiles = [(i, j) for i in range(tq) for j in range(i if call.symmetric else 0, tq if call.symmetric else ts)]
    lane = np.arange(TILE)
    for ti, tj in tiles:
        qi, sj = ti * TILE + lane, tj * TILE + lane
        q_ok, s_ok = qi < nq, sj < ns
        q_rows, s_rows = np.where(q_ok, call.q0 + qi, -1), np.where(s_ok, call.s0 + sj, -1)
        at = np.ix_(qi[q_ok], sj[s_ok])
        for k in range(splits.splits):
            w_lo = k * splits.words_per_split
            m, b = _tile_counts(planes, bits, q_rows, s_rows, w_lo, min(n_words, w_lo + splits.words_per_split), fault, wplanes, nb)
            m, b = m[np.ix_(q_ok, s_ok)], b[np.ix_(q_ok, s_ok)]
            if splits.splits > 1:
                match[at] += m
                both[at] += b
            else:
                match[at], both[at] = m, b
    if call.symmetric and tq > 1:
        _mirror(match, fault)
        _mirror(both, fault)


def emulate(c: Case, fault: str | None = None, compute_units: int = NOMINAL_CUS):
    """What the kernels leave in outputs that held PREFILL_M / PREFILL_B, on a device of ``compute_units``.  Unweighted: a
    list of ``(M, B)``, one per call of the case.  Weighted: ``(M, B)`` of shape ``[R, n, n]``."""
    assert fault is None or fault in FAULTS
    planes, _nongap = pack(c, "pack_no_valid" if fault == "pack_no_valid" else None)
    bits, nw, n = c.bits, c.n_words, c.n_rows
    with np.errstate(over="ignore"):
        if c.weights is None:
            out = []
            for call in c.calls:
                match, both = np.full(call.shape, PREFILL_M, dtype=np.uint32), np.full(call.shape, PREFILL_B, dtype=np.uint32)
                if match.size:
                    splits = split_columns(n_tiles(call), nw, compute_units)
                    if (splits.splits > 1 or nw == 0) and fault != "no_zero":
                        match[:], both[:] = 0, 0
                    if nw:
                        _pairs(planes, bits, nw, call, splits, fault, match, both)
                out.append((match, both))
            return out
        reps = len(c.weights)
        match, both = np.full((reps, n, n), PREFILL_M, dtype=np.uint32), np.full((reps, n, n), PREFILL_B, dtype=np.uint32)
        call = _sym(n)
        if nw == 0:
            if fault != "no_zero":
                match[:], both[:] = 0, 0
            return match, both
        wplanes, nb = weight_planes(c.weights, nw), int(c.weights.max()).bit_length()
        for r0 in range(0, reps, BOOT_BATCH):
            count = min(BOOT_BATCH, reps - r0)
            splits = split_columns(n_tiles(call) * count, nw, compute_units)
            for r in range(r0, r0 + count):
                if splits.splits > 1 and fault != "no_zero":
                    match[r], both[r] = 0, 0
                _pairs(planes, bits, nw, call, splits, fault, match[r], both[r], wplanes[r], nb)
        return match, both


# ---------------------------------------------------------------- what is meant: the checkers' counts, computed once
@functools.lru_cache(maxsize=None)
def expected(name: str):
    """Unweighted: a list of ``(M, B)`` per call from ``msa_checker.counts_matrix``.  Weighted: ``(M, B)`` ``[R, n, n]`` from
    ``bootstrap_cases.counts``."""
    from tests.msa_checker import counts_matrix

    c = case(name)
    if c.weights is None:
        whole = counts_matrix(c.rows)
        return [tuple(x[call.q0 : call.q1, call.s0 : call.s1] for x in whole) for call in c.calls]
    per = [bootstrap_cases.counts(c.rows, c.weights[r]) for r in range(len(c.weights))]
    return np.stack([m for m, _b in per]).astype(np.uint32), np.stack([b for _m, b in per]).astype(np.uint32)
