"""The cases of tests/msa_cases.py against the kernels they are aimed at, without a GPU.

The tile constants are read from csrc/msa_tile_dev.h and the batch from include/pyani_hip.h; the lines of the kernels that
tests/msa_cases.py restates are looked up in the sources.  If one of them changes, a test here fails and says that
tests/msa_cases.py has to follow, so that the GPU tests (tests/test_gpu_msa_edges.py) do not quietly stop reaching the
seams they are named for.  Then: every case has the ``bits``, the rows and the seam it names; the emulation of the plane
arithmetic equals the checkers' byte counts on every case; and every named fault of the emulation changes the result of
a case that is named here."""

from __future__ import annotations

import re

import numpy as np
import pytest

from pyani_plus_amd.engine import msa_code_table
from tests import msa_cases as cases

CSRC = cases.ROOT / "pyani_plus_amd" / "csrc"
FOLLOW = "tests/msa_cases.py restates this and its cases are sized by it: change tests/msa_cases.py too"


def _code(c, rows):
    return c.alphabet.code[rows].astype(int)


def _histogram(rows) -> np.ndarray:
    return np.bincount(np.asarray(rows).ravel(), minlength=256).astype(np.uint64)


# ---------------------------------------------------------------- the sources
def test_case_module_restates_the_kernel_constants():
    got = cases.kernel_constants()
    want = {"TILE": cases.TILE, "THREADS": cases.THREADS, "CHUNK": cases.CHUNK, "MAX_BITS": cases.MAX_BITS, "BOOT_BATCH": cases.BOOT_BATCH}
    assert got == want, f"the headers have {got}, the cases {want}; {FOLLOW}"


def test_the_restated_lines_are_the_kernels():
    sources = {name: (CSRC / name).read_text() for name in ("msa_tile_dev.h", "msa.hip", "msa_boot.hip")}
    for name, pattern, what in (
        ("msa_tile_dev.h", r"const uint64_t want = 8ull \* \(uint64_t\)c->prop\.multiProcessorCount;", "blocks wanted"),
        ("msa_tile_dev.h", r"uint64_t splits = blocks >= want \? 1 : \(want \+ blocks - 1\) / blocks;", "the first split"),
        ("msa_tile_dev.h", r"std::min<uint64_t>\(\{splits, \(\(uint64_t\)n_words \+ 63\) / 64, 65535\}\)", "a slice's least words"),
        ("msa_tile_dev.h", r"wps = \(wps \+ kChunk - 1\) / kChunk \* kChunk;", "whole stages"),
        ("msa_tile_dev.h", r"const bool ok = w < g\.w_hi && local < \(half \? r\.ns : r\.nq\);", "what is staged as zero"),
        ("msa_tile_dev.h", r"for \(int p = 1; p < P - 1; \+\+p\) d = bitop3_t<kXorOr>\(qv\[p\]\[a\], sv\[p\]\[b\], d\);", "d"),
        ("msa_tile_dev.h", r"return bitop3_t<kAndNot>\(d, qv\[P - 1\]\[a\], 0u\);", "eq"),
        ("msa_tile_dev.h", r"return qv\[P - 1\]\[a\] & sv\[P - 1\]\[b\];", "both"),
        ("msa_tile_dev.h", r"if \(c >= \(r / kTile\) \* kTile\) continue;", "the mirror's boundary"),
        ("msa.hip", r"const uint32_t valid = n_cols - col0 >= 32u \? 0xffffffffu : \(\(1u << \(uint32_t\)\(n_cols - col0\)\) - 1u\);", "the pack's column mask"),
        ("msa.hip", r"uint32_t \*dst = planes \+ \(uint64_t\)w \* P \* n_pad \+ row;", "the plane layout"),
        ("msa.hip", r"for \(uint32_t wc = g\.w_lo; wc < g\.w_hi; wc \+= kChunk\) \{", "the stage loop"),
        ("msa.hip", r"if \(accumulate \|\| n_words == 0\) \{", "when the outputs are cleared"),
        ("msa.hip", r"if \(symmetric && tq > 1\) PA_TRY\(launch_mirror", "when the mirror runs"),
        ("msa_boot.hip", r"m\[a\]\[b\] \+= \(uint32_t\)__builtin_popcount\(eq\[a\]\[b\] & W\) << beta;", "the weighted match"),
        ("msa_boot.hip", r"const ColumnSplit split = split_columns\(c, tiles \* count, n_words\);", "the weighted split"),
    ):
        assert re.search(pattern, sources[name]), f"csrc/{name}: {what} no longer has the form this test reads ({pattern!r}); {FOLLOW}"


def test_split_columns_restated():
    # 8 blocks per CU wanted, a slice at least 64 words and whole stages
    assert cases.split_columns(1, 64, 256) == (1, 64)
    assert cases.split_columns(1, 65, 256) == (2, 40)
    assert cases.split_columns(3, 131, 256) == (3, 48)
    assert cases.split_columns(2048, 10_000, 256) == (1, 10_000)
    assert cases.split_columns(1024, 10_000, 256) == (2, 5000)
    assert cases.split_columns(1, 31251, 256) == (489, 64)  # 10^6 columns of one tile
    assert cases.split_columns(1, 0, 256) == (1, 8)
    assert cases.split_columns(1, 1, 1) == (1, 8)


# ---------------------------------------------------------------- what the cases hold
def test_two_alphabets_per_bits_with_the_code_table_of_the_engine():
    assert [a.name for a in cases.ALPHABETS] == [f"bits{b}_{e}" for b in range(1, 9) for e in ("low", "high")]
    for a in cases.ALPHABETS:
        assert len(a.residues) == ((1 << a.bits) - 1 if a.name.endswith("high") else max(1, 1 << (a.bits - 1)))
        assert cases.GAP not in a.residues and list(a.residues) == sorted(set(a.residues))
        code, bits = msa_code_table(_histogram(np.array(a.residues, dtype=np.uint8)))
        assert bits == a.bits and np.array_equal(code, a.code), a.name
    assert 0 in cases.alphabet("bits8_low").residues and 255 in cases.alphabet("bits1_high").residues  # bytes a char table can get wrong


@pytest.mark.parametrize("name", [c.name for c in cases.cases()])
def test_every_case_has_the_bits_it_names(name):
    """No case is left out: a case with room for its alphabet holds every residue byte in its counted columns, so the
    engine's own table is the case's; one without room (a row of one column) is handed the alphabet's table."""
    c = cases.case(name)
    assert c.bits == int(re.search(r"bits(\d)", name).group(1)) if "bits" in name else c.bits == 4
    n, n_cols = c.rows.shape
    room = n * n_cols >= 8 * n_cols + len(c.alphabet.residues)  # beside six placed rows, a column and the features
    if room or c.names & {"alphabet", "many_tiles", "weighted", "slices1", "slices2", "slices3"}:
        code, bits = msa_code_table(_histogram(c.rows))
        assert bits == c.bits and np.array_equal(code, c.alphabet.code)
    else:
        assert set(np.unique(c.rows)) <= set(c.alphabet.residues) | {cases.GAP}
        assert int(_code(c, c.rows).max(initial=0)).bit_length() <= c.bits


def test_which_cases_are_too_small_for_their_alphabet():
    small = [c.name for c in cases.cases() if msa_code_table(_histogram(c.rows))[1] != c.bits]
    assert all(re.fullmatch(r"(rows(1|2)|cols(0|1|31|32|33))_bits(4|8)", name) for name in small), small


def test_every_case_is_padded_with_residues():
    strides = set()
    for c in cases.cases():
        n_cols = c.n_cols
        assert c.stride % 32 == 0 and c.stride >= max(32, c.n_words * 32)
        assert np.array_equal(c.padded[:, :n_cols], c.rows)
        assert not (c.padded[:, n_cols:] == cases.GAP).any() and set(np.unique(c.padded[:, n_cols:])) <= set(c.alphabet.residues)
        if c.stride > n_cols:
            assert (c.padded[:, n_cols] == c.alphabet.top).all()  # all planes set right behind the last column
        strides.add(c.stride - max(32, c.n_words * 32))
    assert strides == {0, 32, 96}  # as small as allowed, and larger than needed


def _has_column(c, a: int, b: int) -> bool:
    codes = _code(c, c.rows[:2])
    return bool(((codes[0] == a) & (codes[1] == b)).any())


@pytest.mark.parametrize("name", [c.name for c in cases.cases() if c.n_rows >= 6 and c.n_cols >= 40])
def test_the_rows_hold_what_a_kernel_can_get_wrong(name):
    c = cases.case(name)
    a, top = c.alphabet, len(c.alphabet.residues)
    pairs = cases.plane_pairs(a)
    assert set(pairs) == {p for p in range(a.bits) if any(1 <= (x ^ (1 << p)) <= top for x in range(1, top + 1))}
    assert a.name.endswith("low") or a.bits == 1 or set(pairs) == set(range(a.bits))  # the largest alphabet has a pair for every plane
    for p, (x, y) in pairs.items():
        assert x ^ y == 1 << p and _has_column(c, x, y), (p, x, y)  # two residues that plane p alone separates
    for p in range(a.bits):
        assert _has_column(c, 1 << p, 0) and _has_column(c, 0, 1 << p), p  # exactly one row is gap, on either side
    assert _has_column(c, 0, 0)  # both gap
    gap_column = cases.gap_column_of(a, c.n_cols) if name.startswith(("rows", "cols", "slices", "many")) else None
    assert np.array_equal(c.rows[2], c.rows[3])
    assert (c.rows[4] == cases.GAP).all()
    others = np.ones(c.n_cols, dtype=bool)
    if gap_column is None:
        assert not (c.rows[2] == cases.GAP).any()  # two identical rows without a gap
        assert not (c.rows == cases.GAP).all(axis=0).any()
    else:
        assert (c.rows[:, gap_column] == cases.GAP).all()  # an all-gap column
        others[gap_column] = False
        assert not (c.rows[2, others] == cases.GAP).any()
    assert (c.rows[5, others] == a.top).all() and _code(c, c.rows[5, others]).min() == top  # the highest code: every plane it has is set
    if c.weights is None:
        m, b = cases.expected(name)[0]
        assert m[2, 3] == b[2, 3] == int(others.sum()) and m[4].max() == 0 and b[:, 4].max() == 0


def test_the_alphabet_cases_have_identical_rows_and_the_seam_cases_a_gap_column():
    for c in cases.cases():
        has = bool((c.rows == cases.GAP).all(axis=0).any())
        if "alphabet" in c.names or c.weights is not None:
            m, b = (cases.expected(c.name)[0] if c.weights is None else [x[0] for x in cases.expected(c.name)])
            assert not has and (m[2, 3] == b[2, 3] == c.n_cols or c.weights is not None)
        elif c.n_cols > len(cases.feature_columns(c.alphabet)):
            assert has, c.name


def test_the_shapes_reach_every_seam():
    names = [c.name for c in cases.cases()]
    for bits in cases.SEAM_BITS:
        for n in (1, 2, cases.TILE - 1, cases.TILE, cases.TILE + 1, 2 * cases.TILE, 2 * cases.TILE + 1):
            c = cases.case(f"rows{n}_bits{bits}")
            assert c.n_rows == n and c.calls[0] == (0, n, 0, n, 1) and c.calls[1] == (0, n, 0, n, 0)
        stage = 32 * cases.CHUNK
        for n_cols in (0, 1, 31, 32, 33, stage - 1, stage, stage + 1):
            assert cases.case(f"cols{n_cols}_bits{bits}").n_cols == n_cols
        for rows in (6, 65):
            assert cases.case(f"slices1_rows{rows}_bits{bits}").n_words == 64  # the most that one slice takes
            assert cases.case(f"slices2_rows{rows}_bits{bits}").n_cols == 64 * 32 + 1
            assert cases.case(f"slices3_rows{rows}_bits{bits}").n_words == 131
            assert all(call.symmetric for call in cases.case(f"slices3_rows{rows}_bits{bits}").calls) == (rows == 65)
    many = cases.case("many_tiles")
    assert cases.n_tiles(many.calls[0]) == cases.MANY_TILES == 171 and many.rows.shape == (1100, 32)
    assert len(names) == len(set(names))
    assert max(c.n_rows for c in cases.cases()) <= 1100 and max(c.n_cols for c in cases.cases()) <= 4161


@pytest.mark.parametrize("compute_units", [cases.NOMINAL_CUS, 304, 64, 8])
def test_the_split_cases_land_on_the_path_they_name(compute_units):
    """On any device of at least 8 CUs (3 tiles then still want slices)."""
    for c in cases.cases():
        for call in c.calls:
            if 0 in call.shape:
                continue  # an empty range launches nothing
            split = cases.split_columns(cases.n_tiles(call), c.n_words, compute_units)
            named = [int(x[6:]) for x in c.names if x.startswith("slices")]
            assert split.splits == (named[0] if named else 1), (c.name, call, split)
            if named == [3]:
                last = c.n_words - 2 * split.words_per_split
                assert 0 < last < split.words_per_split and last % cases.CHUNK  # the last slice ends in the middle of a stage
                assert split.words_per_split % cases.CHUNK == 0


def test_the_ranges_are_off_the_tile_grid():
    for a in cases.ALPHABETS:
        c = cases.case(f"alpha_{a.name}")
        n, calls = c.n_rows, c.calls
        assert n > cases.TILE and calls[0] == (0, n, 0, n, 1)  # two tiles: the mirror runs for every alphabet
        rect = calls[1:]
        assert any(x.q0 % cases.TILE and x.s0 % cases.TILE and x.q1 == n and x.s1 == n for x in rect)
        assert any(x.q1 - x.q0 == 1 and x.s1 - x.s0 > cases.TILE for x in rect) and any(x.s1 - x.s0 == 1 and x.s1 == n for x in rect)
        assert any(x.q1 == x.q0 for x in rect) and any(x.s1 == x.s0 for x in rect)
        assert any((x.q0, x.q1) == (x.s0, x.s1) and not x.symmetric and x.q1 > x.q0 for x in rect)
        assert any(x.q1 - x.q0 == x.s1 - x.s0 > 0 and x.q0 != x.s0 for x in rect)


def test_the_weighted_cases():
    got = sorted(c.name for c in cases.weighted_cases())
    assert got == sorted(f"weighted_bits{b}_{e}" for b in (3, 5, 6, 7) for e in ("low", "high"))
    for c in cases.weighted_cases():
        assert c.rows.shape == (cases.TILE + 1, 32 * cases.CHUNK + 1)
        w = c.weights
        assert w.dtype == np.uint8 and (w.sum(axis=1, dtype=np.int64) == c.n_cols).all()
        assert 2 <= int(w[:2].max()) <= 7 and w[2].max() == 255 and w[2, c.n_cols - 1] == 255  # drawn weights, and one of 255


# ---------------------------------------------------------------- the emulation against the checkers
def _same(got, want) -> bool:
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _equal(c, got) -> bool:
    want = cases.expected(c.name)
    if c.weights is not None:
        return _same(got, want)
    assert len(got) == len(want) == len(c.calls)
    return all(g[0].shape == call.shape and _same(g, w) for g, w, call in zip(got, want, c.calls))


@pytest.mark.parametrize("name", [c.name for c in cases.cases()])
def test_emulation_without_a_fault_equals_the_checker(name):
    c = cases.case(name)
    assert _equal(c, cases.emulate(c))
    planes, nongap = cases.pack(c)
    assert np.array_equal(nongap, (c.rows != cases.GAP).sum(axis=1))
    assert (planes[c.n_words :] == cases.PLANE_FILL).all() and (planes[:, :, c.n_rows :] == cases.PLANE_FILL).all()


def test_emulation_does_not_depend_on_the_compute_units():
    for name in ("slices3_rows65_bits4", "slices2_rows6_bits8", "rows129_bits1", "weighted_bits5_high"):
        c = cases.case(name)
        for cus in (1, 8, 304):
            assert _equal(c, cases.emulate(c, compute_units=cus)), (name, cus)


# the cases that have to tell each fault (a fault may be told by more)
TELLERS = {
    "eq_unmasked": ["alpha_bits1_low", "alpha_bits8_high", "cols1_bits1"],  # both rows gap; the columns past the last
    "both_query_only": ["alpha_bits1_low", "alpha_bits8_high", "rows2_bits4"],  # exactly one row gap
    "pack_no_valid": ["cols1_bits1", "cols31_bits4", "cols33_bits8", "cols257_bits1", "slices2_rows6_bits4", "alpha_bits6_low"],
    "stage_past_w_hi": ["cols1_bits1", "cols257_bits8", "slices2_rows65_bits1", "slices3_rows6_bits4"],
    "drop_partial_stage": ["cols1_bits8", "cols33_bits4","cols257_bits1", "slices2_rows6_bits1", "slices3_rows65_bits8"],
    "no_zero": ["cols0_bits1", "cols0_bits8", "slices2_rows6_bits4", "slices3_rows65_bits1"],
    "mirror_boundary": ["rows65_bits1", "rows128_bits4", "rows129_bits8", "many_tiles", "slices2_rows65_bits4", "alpha_bits3_low"],
    "weight_shift": ["weighted_bits3_low", "weighted_bits7_high"],
}


@pytest.mark.parametrize("fault", [f for f in cases.FAULTS if not f.startswith("drop_plane")])
def test_every_fault_is_told_by_the_cases_named_for_it(fault):
    for name in TELLERS[fault]:
        c = cases.case(name)
        assert not _equal(c, cases.emulate(c, fault)), f"{name} does not tell a kernel with the fault {fault} from a right one"
    print(f"{fault}: told by {', '.join(TELLERS[fault])}")


@pytest.mark.parametrize("alpha", [a.name for a in cases.ALPHABETS])
def test_every_plane_of_every_alphabet_is_told(alpha):
    """A pair kernel that leaves plane p out of d gives other counts on the alphabet's own case, for every p below its bits
    (and the same counts for a p it does not have)."""
    a = cases.alphabet(alpha)
    for c in [cases.case(f"alpha_{alpha}")] + [w for w in cases.weighted_cases() if w.alphabet is a]:
        for p in range(cases.MAX_BITS):
            assert _equal(c, cases.emulate(c, f"drop_plane{p}")) == (p >= a.bits), (c.name, p)
    print(f"{alpha}: planes 0..{a.bits - 1} each told by alpha_{alpha}")


def test_the_stores_of_a_call_without_a_split_hide_a_missing_memset():
    """Why the split cases exist: on one slice every cell is stored, and `no_zero` shows in no result."""
    for name in ("slices1_rows6_bits4", "slices1_rows65_bits1", "rows129_bits8", "alpha_bits5_high"):
        c = cases.case(name)
        assert _equal(c, cases.emulate(c, "no_zero")), name
