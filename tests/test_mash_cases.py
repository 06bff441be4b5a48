"""The cases of tests/mash_cases.py against the kernels they are aimed at, without a GPU.

The launch constants and the lines of the two merge loops are read from csrc/bottom_mash.hip; if one of them changes, a
test here fails and says that tests/mash_cases.py has to follow, so that the GPU tests (tests/test_gpu_mash_edges.py) do
not quietly stop reaching the launch shapes and lanes they are named for.  The two kernels' merge loops are restated in
Python, and every case names one wrong variant of them that it exists to catch: the variant's result differs from the
brute-force estimator on that case, the restatement's does not."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from tests import mash_cases as cases

SOURCE = Path(__file__).resolve().parent.parent / "pyani_plus_amd" / "csrc" / "bottom_mash.hip"
FOLLOW = "tests/mash_cases.py restates this and its cases are sized by it: change tests/mash_cases.py too"
BIG = 0xFFFFFFFF


def _find(pattern: str, text: str, what: str) -> re.Match:
    m = re.search(pattern, text, re.S)
    assert m, f"csrc/bottom_mash.hip: {what} no longer has the form this test reads ({pattern!r}); {FOLLOW}"
    return m


@pytest.fixture(scope="module")
def kernel() -> dict:
    """What the source says: the launch constants, and that the host arithmetic and the merge loops read as restated."""
    text = SOURCE.read_text()
    budget = _find(r"constexpr uint32_t kLdsBudget = (\d+)u \* (\d+)u;", text, "kLdsBudget")
    out = {
        "lds_budget": int(budget.group(1)) * int(budget.group(2)),
        "max_tile_threads": int(_find(r"constexpr uint32_t kMaxTileThreads = (\d+);", text, "kMaxTileThreads").group(1)),
        "max_tq": int(_find(r"uint32_t tq = std::min\(\{lists / 2u, nq, (\d+)u\}\);", text, "tq").group(1)),
        "threads": int(_find(r"constexpr int kThreads = (\d+);", text, "kThreads").group(1)),
        "sentinel": int(_find(r"constexpr uint32_t kSentinel = (0x[0-9a-fA-F]+)u;", text, "kSentinel").group(1), 16),
    }
    per = _find(r"const uint32_t per = \(total \+ (\d+)u\) / (\d+)u;", text, "the steps of a lane")
    assert int(per.group(1)) + 1 == int(per.group(2)), FOLLOW
    out["wave"] = int(per.group(2))
    for pattern, what in (
        (r"const uint32_t stride = \(uint32_t\)longest \+ 1u;", "stride"),
        (r"const uint32_t lists = kLdsBudget / \(4u \* stride\);", "lists"),
        (r"if \(lists >= 2 && P < \(1ULL << 32\) && P > 0\) \{", "the choice between the kernels"),
        (r"uint32_t ts = std::min\(\{lists - tq, ns, kMaxTileThreads / tq\}\);", "ts"),
        (r"const uint32_t threads = \(\(tq \* ts \+ 63u\) / 64u\) \* 64u;", "the tile block"),
        (r"const uint32_t lds_bytes = \(tq \+ ts\) \* stride \* 4u;", "the dynamic LDS"),
        (r"longest = std::max\(longest, std::min<uint64_t>\(m, h_off\[g \+ 1\] - h_off\[g\]\)\);", "longest"),
        (r"constexpr int kWavesPerBlock = kThreads / 64;", "pairs per block of the wave kernel"),
        (r"const uint32_t d0 = min\(lane \* per, total\), d1 = min\(d0 \+ per, total\);", "a lane's slice"),
        (r"const uint32_t len = \(uint32_t\)min\(\(uint64_t\)m, off\[g \+ 1\] - beg\);", "the truncation of a staged list"),
        (r"while \(uni < m && \(x & y\) != kSentinel\) \{", "the tile loop's condition"),
        (r"const uint32_t adv_a = x <= y \? 1u : 0u, adv_b = y <= x \? 1u : 0u;", "the tile loop's step"),
        (r"const bool take_a = \(j >= nb\) \|\| \(i < na && a\[i\] <= b\[j\]\);", "the walk's tie"),
        (r"uni \+= \(i > 0 && a\[i - 1\] == b\[j\]\) \? 0u : 1u;", "the walk's B step"),
        (r"if \(a\[i\] <= b\[d - i - 1\]\) lo = i \+ 1; else hi = i;", "the merge path"),
        (r"if \(before >= m\) my_com = 0;", "lanes beyond the m-th union element"),
        (r"else if \(incl > m\) \{", "the straddling lane"),
        (r"walk\(a, na, b, nb, i, j, d1 - d0, m - before, &u2, &c2\);", "the bounded second walk"),
        (r"denom\[pair\] = total_union < m \? total_union : m;", "the wave kernel's denominator"),
    ):
        _find(pattern, text, what)
    return out


def test_case_module_restates_the_kernel_constants(kernel):
    got = (kernel["lds_budget"], kernel["max_tile_threads"], kernel["max_tq"], kernel["threads"], kernel["wave"], kernel["sentinel"])
    want = (cases.LDS_BUDGET, cases.MAX_TILE_THREADS, cases.MAX_TQ, cases.THREADS, cases.WAVE, cases.SENTINEL)
    assert got == want, f"kLdsBudget, kMaxTileThreads, the bound of tq, kThreads, the lanes of `per`, kSentinel are {got} in the kernel file, {want} in the cases; {FOLLOW}"


# ---------------------------------------------------------------- the two merge loops, restated, with their wrong variants
def tile_pair(a: list[int], b: list[int], m: int, variant: str | None = None) -> tuple[int, int]:
    """One thread of ``mash_tile_kernel`` over two lists of dense ids.  Variants: ``tie_strict`` (B advances on y < x
    only: a tie is no common element and its B copy a new one), ``no_truncate`` (the lists staged and merged whole, m
    ignored), ``sentinel_as_value`` (the loop runs on ``uni < m`` alone: two spent lists show two equal sentinels, a common
    element each turn)."""
    assert variant in (None, "tie_strict", "no_truncate", "sentinel_as_value")
    whole = variant == "no_truncate"
    A = (a if whole else a[:m]) + [cases.SENTINEL]
    B = (b if whole else b[:m]) + [cases.SENTINEL]
    i = j = uni = com = 0
    x, y = A[0], B[0]
    while (whole or uni < m) and (variant == "sentinel_as_value" or (x & y) != cases.SENTINEL):
        adv_a = x <= y
        adv_b = y < x if variant == "tie_strict" else y <= x
        com += adv_a and adv_b
        uni += 1
        i += adv_a
        j += adv_b
        x = A[i] if i < len(A) else cases.SENTINEL  # past a spent list: whatever LDS holds; the variant's denom is m either way
        y = B[j] if j < len(B) else cases.SENTINEL
    return com, uni


def merge_path(a: list[int], b: list[int], d: int) -> int:
    na, nb = len(a), len(b)
    lo, hi = (d - nb if d > nb else 0), (d if d < na else na)
    while lo < hi:
        i = (lo + hi) >> 1
        if a[i] <= b[d - i - 1]:
            lo = i + 1
        else:
            hi = i
    return lo


def walk(a, b, i: int, j: int, steps: int, union_limit: int, variant: str | None) -> tuple[int, int]:
    na, nb = len(a), len(b)
    uni = com = t = 0
    while t < steps and uni < union_limit:
        if variant == "tie_strict":
            take_a = j >= nb or (i < na and a[i] < b[j])
        else:
            take_a = j >= nb or (i < na and a[i] <= b[j])
        if take_a:
            com += j < nb and a[i] == b[j]
            uni += 1
            i += 1
        else:
            uni += 1 if variant == "b_repeat" else not (i > 0 and a[i - 1] == b[j])
            j += 1
        t += 1
    return uni, com


def wave_pair(a: list[int], b: list[int], m: int, variant: str | None = None, lanes_out: list | None = None) -> tuple[int, int]:
    """One wavefront of ``mash_pair_kernel``.  Variants: ``tie_strict`` (the walk takes B first on a tie), ``b_repeat`` (a
    B step always counts as a new union element), ``no_rewalk`` (the lane in which the m-th union element falls keeps its
    whole count), ``no_truncate`` (m ignored: every lane keeps its count, the denominator is the whole union)."""
    assert variant in (None, "tie_strict", "b_repeat", "no_rewalk", "no_truncate")
    total = len(a) + len(b)
    per = (total + cases.WAVE - 1) // cases.WAVE
    lanes = []
    for lane in range(cases.WAVE):
        d0 = min(lane * per, total)
        d1 = min(d0 + per, total)
        i = j = uni = com = 0
        if d0 < d1:
            i = merge_path(a, b, d0)
            j = d0 - i
            uni, com = walk(a, b, i, j, d1 - d0, BIG, variant)
        lanes.append((i, j, d1 - d0, uni, com))
    before = common = 0
    for lane, (i, j, steps, uni, com) in enumerate(lanes):
        incl = before + uni
        if variant == "no_truncate":
            mine = com
        elif before >= m:
            mine = 0
        elif incl > m and variant != "no_rewalk":
            mine = walk(a, b, i, j, steps, m - before, variant)[1]
        else:
            mine = com
        if lanes_out is not None:
            lanes_out.append({"lane": lane, "before": before, "incl": incl, "first": (i, j), "steps": steps})
        common += mine
        before = incl
    return common, (before if variant == "no_truncate" else min(before, m))


def dense_ids(sketches: list[np.ndarray]) -> list[list[int]]:
    """``pa_dense_ids_sorted``: every hash's rank among the distinct hashes of the whole set."""
    distinct = np.unique(np.concatenate(sketches))
    return [np.searchsorted(distinct, s).tolist() for s in sketches]


def restated(sketches, m: int, pairs, path: str, variant: str | None = None) -> list[tuple[int, int]]:
    if path == "tile":
        ids = dense_ids(sketches)
        return [tile_pair(ids[q], ids[s], m, variant) for q, s in pairs]
    lists = [s.tolist() for s in sketches]
    return [wave_pair(lists[q], lists[s], m, variant) for q, s in pairs]


def check_case(sketches, m: int, pairs, path: str, variant: str, what: str) -> None:
    want = [cases.brute_pair(sketches[q], sketches[s], m) for q, s in pairs]
    assert restated(sketches, m, pairs, path) == want, f"{what}: the restated {path} kernel differs from the brute-force estimator"
    wrong = restated(sketches, m, pairs, path, variant)
    assert wrong != want, f"{what}: the variant {variant!r} of the {path} kernel gives the right answer on every pair; {FOLLOW}"


# ---------------------------------------------------------------- 1. geometry ladder
LADDER_PAIRS = ((0, 1), (1, 0), (1, 1), (2, 1), (0, 2), (3, 4), (4, 4))
LADDER_CATCHES = {
    "longest 9983": "tie_strict", "longest 9984": "tie_strict", "longest 13311": "tie_strict", "longest 13312": "tie_strict",
    "longest 19967": "tie_strict", "longest 19968": "b_repeat", "25000 cut to 19967": "no_truncate", "25000 cut to 19968": "no_rewalk",
}  # fmt: skip


@pytest.mark.parametrize("run", cases.ladder_runs(), ids=lambda r: r[0])
def test_ladder_case_lands_on_its_shape_and_tells_its_variant(run):
    name, length, edge, m = run
    sketches = cases.ladder_case(length, edge)
    for s in sketches:
        assert s.dtype == np.uint64 and np.all(s[1:] > s[:-1])
    sizes = [len(s) for s in sketches]
    assert sizes[cases.LADDER_LONG] == length and max(x for g, x in enumerate(sizes) if g != cases.LADDER_LONG) <= 8 and 0 in sizes
    plan = cases.launch_plan(sketches, m)
    lists, tq, ts = cases.LADDER[min(m, length)]
    assert plan["longest"] == min(m, length) and plan["lists"] == lists, f"{name}: {plan}; {FOLLOW}"
    if lists >= 2:
        assert (plan["path"], plan["tq"], plan["ts"], plan["threads"]) == ("tile", tq, ts, 64), f"{name}: {plan}; {FOLLOW}"
        assert plan["lds_bytes"] <= cases.LDS_BUDGET and plan["tiles_q"] * tq >= 5 > (plan["tiles_q"] - 1) * tq
        if ts == 2:
            assert plan["tiles_s"] == 3  # a ragged last tile of one column
        if min(m, length) in (9983, 13311, 19967):
            assert plan["lds_bytes"] == cases.LDS_BUDGET  # the last length of its shape fills the budget to the byte
    else:
        assert plan["path"] == "wave" and plan["blocks"] == 7  # 25 pairs, four to a block: three idle wavefronts in the last
    if length > m:
        assert length == cases.TRUNCATED_LEN and m in cases.TRUNCATED_MS
    common, denom = cases.brute_pair(sketches[0], sketches[cases.LADDER_LONG], m)
    assert denom == m and common == {None: 2, 19967: 2 + (m - 19967)}[edge]  # the elements past the m-th are not counted
    check_case(sketches, m, LADDER_PAIRS, plan["path"], LADDER_CATCHES[name], name)


def test_ladder_thresholds_are_the_formula_s():
    """Each length of the ladder is the last or the first of its number of lists."""
    lists = lambda longest: cases.LDS_BUDGET // (4 * (longest + 1))  # noqa: E731
    assert [lists(x) for x in (8, 9983, 9984, 13311, 13312, 19967, 19968)] == [4437, 4, 3, 3, 2, 2, 1], FOLLOW
    assert sorted(cases.LADDER) == [9983, 9984, 13311, 13312, 19967, 19968] and cases.TRUNCATED_MS == (19967, 19968)
    assert 2 * (19967 + 1) * 4 == cases.LDS_BUDGET == 159744


# ---------------------------------------------------------------- 2. many short lists
SHORT_CATCHES = {8: "sentinel_as_value", 3: "no_truncate", 1: "tie_strict"}


def test_short_case_holds_what_it_names():
    sketches, pool = cases.short_case()
    assert len(sketches) == cases.SHORT_N == 70 and pool.size == 40 and pool[0] == 0 and pool[-1] == cases.TOP
    for s in sketches:
        assert s.dtype == np.uint64 and len(s) <= 8 and np.all(s[1:] > s[:-1]) and np.all(np.isin(s, pool))
    sizes = {len(s) for s in sketches}
    assert sizes == set(range(9))
    assert len(sketches[0]) == len(sketches[33]) == 0
    assert np.array_equal(sketches[1], sketches[2]) and np.array_equal(sketches[1], sketches[36]) and len(sketches[1]) == 8  # identical, across a tile edge too
    assert len(sketches[3]) == 4 and np.array_equal(sketches[3], sketches[1][:4])  # a strict prefix
    both = np.sort(np.concatenate([sketches[4], sketches[5]]))
    assert np.intersect1d(sketches[4], sketches[5]).size == 0 and np.array_equal(both[0::2], sketches[4]) and np.array_equal(both[1::2], sketches[5])  # interleaved
    assert sketches[6].tolist() == [0, cases.TOP] == sketches[69].tolist() and sketches[7].tolist() == [cases.TOP]


@pytest.mark.parametrize("window", cases.SHORT_WINDOWS, ids=str)
def test_short_windows_land_on_their_shapes(window):
    sketches, _pool = cases.short_case()
    q_range, s_range = window
    want = {
        ((0, 70), (0, 70)): (32, 32, 3, 3, 1024),  # the 1024-thread block, 3 x 3 tiles, a ragged edge of 6
        ((3, 40), (35, 70)): (32, 32, 2, 2, 1024),  # ragged edges of 5 and 3 at offsets
        ((0, 5), (0, 7)): (5, 7, 1, 1, 64),  # 35 live threads in a block of 64
        ((69, 70), (0, 70)): (1, 70, 1, 1, 128),  # one row, 70 live threads in a block of 128
    }[window]
    for m in cases.SHORT_MS:
        plan = cases.launch_plan(sketches, m, q_range, s_range)
        assert plan["path"] == "tile" and (plan["tq"], plan["ts"], plan["tiles_q"], plan["tiles_s"], plan["threads"]) == want, f"{window}, m = {m}: {plan}; {FOLLOW}"
    assert 70 - 2 * 32 == 6 and cases.launch_plan(sketches, 8)["lists"] == 4437


@pytest.mark.parametrize("m", cases.SHORT_MS)
def test_short_case_tells_its_variant(m):
    sketches, _pool = cases.short_case()
    pairs = [(q, s) for q in range(cases.SHORT_N) for s in range(cases.SHORT_N)]
    check_case(sketches, m, pairs, "tile", SHORT_CATCHES[m], f"70 short lists, m = {m}")
    common, denom = cases.brute_matrices(sketches, m)
    o_common, o_denom = oracle.mash_pairs(sketches, m)
    assert np.array_equal(common, o_common) and np.array_equal(denom, o_denom)
    assert denom.min() == 0 and denom.max() == m and common[1, 2] == min(m, 8) and common[4, 5] == 0
    if m == 8:
        assert (denom < m).sum() > 100  # unions shorter than m: both lists are spent before the loop's bound


# ---------------------------------------------------------------- 3. wave kernel
WAVE_PAIRS = ((cases.WAVE_A, cases.WAVE_B), (cases.WAVE_B, cases.WAVE_A), (cases.WAVE_A, 4), (3, cases.WAVE_A), (1, 2), (1, 1), (2, 3), (4, 4))
WAVE_CATCHES = {"last step": "tie_strict", "first step": "no_rewalk", "tie across lanes": "b_repeat"}


def test_wave_case_holds_what_it_names():
    sketches, facts = cases.wave_case()
    assert [len(s) for s in sketches] == [cases.WAVE_LONG, 0, 1, 3, 70, cases.WAVE_LONG]
    for s in sketches:
        assert s.dtype == np.uint64 and np.all(s[1:] > s[:-1])
    a, b = sketches[cases.WAVE_A], sketches[cases.WAVE_B]
    assert np.array_equal(np.intersect1d(a, b), a[::3])  # every third hash of the first
    assert sketches[3][0] == 0 and sketches[3][-1] == cases.TOP
    totals = sorted({len(x) + len(y) for x in sketches for y in sketches})
    assert totals[0] == 0 and totals[1] == 1 and sum(t < cases.WAVE for t in totals) >= 5 and totals[-1] == 2 * cases.WAVE_LONG
    assert facts["per"] == -(-facts["total"] // cases.WAVE) and len(set(facts["lane"].values())) == 3
    for m in facts["m"].values():
        plan = cases.launch_plan(sketches, m)
        assert plan["path"] == "wave" and plan["lists"] == 1 and m < len(np.union1d(a, b)), f"m = {m}: {plan}; {FOLLOW}"


@pytest.mark.parametrize("where", cases.WAVE_WHERE)
def test_wave_case_puts_the_mth_element_where_it_says_and_tells_its_variant(where):
    sketches, facts = cases.wave_case()
    m, lane, per = facts["m"][where], facts["lane"][where], facts["per"]
    a, b = sketches[cases.WAVE_A].tolist(), sketches[cases.WAVE_B].tolist()
    lanes: list[dict] = []
    assert wave_pair(a, b, m, None, lanes) == cases.brute_pair(sketches[cases.WAVE_A], sketches[cases.WAVE_B], m)
    mine, after = lanes[lane], lanes[lane + 1]
    assert mine["steps"] == per == after["steps"] and mine["before"] < m <= mine["incl"]  # the m-th union element is in this lane
    i, j = mine["first"]
    if where == "first step":
        assert mine["before"] == m - 1 and mine["incl"] > m + 1  # its first step; the second walk stops after one step
        assert walk(a, b, i, j, per, BIG, None)[1] > walk(a, b, i, j, per, 1, None)[1]  # common elements of the lane past the m-th
    else:
        assert mine["incl"] == m and after["before"] == m  # its last step: no second walk, and the next lane counts nothing
        assert walk(a, b, i, j, per - 1, BIG, None)[0] == m - mine["before"] - 1
        i2, j2 = after["first"]
        tie = where == "tie across lanes"
        # in the tie case the lane's last step is an A step and the next lane starts on the B element equal to it
        assert (i2 - i) + (j2 - j) == per
        assert (j2 < len(b) and a[i2 - 1] == b[j2]) == tie
        assert walk(a, b, i2, j2, 1, BIG, None)[0] == (0 if tie else 1)
    check_case(sketches, m, WAVE_PAIRS, "wave", WAVE_CATCHES[where], f"wave kernel, the m-th union element on a lane's {where}")


def test_every_variant_is_told_by_some_case():
    named = set(LADDER_CATCHES.values()) | set(SHORT_CATCHES.values()) | set(WAVE_CATCHES.values())
    assert named == set(cases.VARIANTS)


# ---------------------------------------------------------------- 4. pa_ani_mash
def test_ani_grid_and_the_oracle_s_error():
    assert len(cases.ANI_GRID) == 36 and cases.ANI_SIZES == (1, 255, 256, 257) and cases.ANI_KS == (1, 21, 31, 64)
    assert cases.THREADS == 256  # the sizes are one block less one, one block, and one more
    c1, d1 = cases.ani_vectors(1)
    assert (int(c1[0]), int(d1[0])) == (999, 1000)
    for size in cases.ANI_SIZES[1:]:
        c, d = cases.ani_vectors(size)
        assert c.dtype == d.dtype == np.uint32 and len(c) == len(d) == size and {(int(x), int(y)) for x, y in zip(c, d)} == set(cases.ANI_GRID)
    worst = 0.0
    for k in cases.ANI_KS:
        ref = cases.ani_reference(k)
        grid = np.array(cases.ANI_GRID, dtype=np.uint64).astype(np.uint32)
        host = oracle.mash_ani(grid[:, 0], grid[:, 1], k)
        for (c, d), v in zip(cases.ANI_GRID, host):
            if ref[(c, d)] is None:
                assert (c == 0 or d == 0) and np.isnan(v)
            elif c == d:
                assert v == 1.0 and ref[(c, d)][0] == 1
            else:
                worst = max(worst, cases.ani_error_in_units(float(v), c, d, k))
    assert 0.0 < worst < 4.0  # a float64 restatement: a few roundings, each at most half a unit


# ---------------------------------------------------------------- 5. pa_sketch_bottom: the loop stops below the maximum
def test_escalation_genomes_raise_the_threshold_once():
    from pyani_plus_amd.engine import pack_genomes

    k, m = cases.ESCALATION_K, cases.ESCALATION_M
    genomes = cases.escalation_genomes()
    assert max(len(g) for g in genomes) <= 200_000 and len(genomes[0]) < len(genomes[1])
    arena = pack_genomes(genomes, fasta=False)
    positions = [int(arena.genome_start[g + 1] - arena.genome_start[g]) for g in range(len(genomes))]  # what the host sizes the threshold by
    assert positions[0] == min(positions) and len(genomes[0]) <= positions[0] < len(genomes[0]) + 64
    thresholds = cases.escalation_thresholds(positions, m)
    assert len(thresholds) >= 3 and thresholds[-1] == cases.TOP and thresholds[1] < cases.TOP // 4
    every = [oracle.sketch_seq(g, k, 1) for g in genomes]
    assert len(every[1]) >= 10 * m  # distinct k-mers of the repeated unit
    under = [[int((h <= np.uint64(t)).sum()) for h in every] for t in thresholds]
    assert under[0][0] >= 2 * m and under[0][1] < m // 2, f"first threshold: {under[0]}; {FOLLOW}"  # the repeat genome comes up short
    assert min(under[1]) >= 2 * m, f"second threshold: {under[1]}; {FOLLOW}"  # and the loop stops here, below the maximum
    for g, seq in enumerate(genomes):
        assert np.array_equal(oracle.sketch_bottom_seq(seq, k, m), every[g][:m])
