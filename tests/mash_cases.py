"""Inputs aimed at the edges of csrc/bottom_mash.hip: every launch shape of ``mash_tile_kernel`` between the 1024-thread
block and the exact-budget LDS launch, the fall-back to ``mash_pair_kernel`` and the lane in which its m-th union element
falls, ``mash_ani_kernel`` on a made grid, and a ``pa_sketch_bottom`` call whose threshold loop stops below the maximum.

The sketches are hand-built sorted uint64 lists (``engine.sketches_from_host``): no genome is hashed for the pair cases.
Used by tests/test_mash_cases.py (no GPU: the cases against the constants parsed from the kernel file, and against wrong
variants of the two merge loops) and by tests/test_gpu_mash_edges.py (the kernels against ``brute_matrices`` and the
oracle).  The constants below restate the kernel file's; when those change, change them here, and the cases follow."""

from __future__ import annotations

from decimal import Decimal, getcontext
from functools import lru_cache

import numpy as np

# csrc/bottom_mash.hip: kLdsBudget, kMaxTileThreads, the 32u of tq, kThreads, the wavefront
LDS_BUDGET, MAX_TILE_THREADS, MAX_TQ, THREADS, WAVE = 156 * 1024, 1024, 32, 256, 64
SENTINEL = 0xFFFFFFFF
TOP = 2**64 - 1
VARIANTS = ("tie_strict", "b_repeat", "no_rewalk", "no_truncate", "sentinel_as_value")


# ---------------------------------------------------------------- the estimator, by brute force
def brute_pair(a: np.ndarray, b: np.ndarray, m: int) -> tuple[int, int]:
    """(common, denom): ``denom`` = min(m, |A u B|), ``common`` = the shared hashes among the first ``denom`` of the
    sorted union."""
    union = np.union1d(a, b)
    denom = min(int(m), union.size)
    return int(np.intersect1d(union[:denom], np.intersect1d(a, b)).size), denom


def brute_matrices(sketches: list[np.ndarray], m: int, q_range=None, s_range=None) -> tuple[np.ndarray, np.ndarray]:
    n = len(sketches)
    q0, q1 = q_range or (0, n)
    s0, s1 = s_range or (0, n)
    common = np.zeros((q1 - q0, s1 - s0), dtype=np.uint32)
    denom = np.zeros_like(common)
    for q in range(q0, q1):
        for s in range(s0, s1):
            common[q - q0, s - s0], denom[q - q0, s - s0] = brute_pair(sketches[q], sketches[s], m)
    return common, denom


# ---------------------------------------------------------------- the host's choice of a launch
def launch_plan(sketches: list[np.ndarray], m: int, q_range=None, s_range=None) -> dict:
    """``pa_pair_mash``'s arithmetic: {"path": "tile", longest, lists, tq, ts, tiles_q, tiles_s, threads, lds_bytes} or
    {"path": "wave", longest, lists, blocks}."""
    n = len(sketches)
    q0, q1 = q_range or (0, n)
    s0, s1 = s_range or (0, n)
    nq, ns = q1 - q0, s1 - s0
    longest = max([min(m, len(sketches[g])) for g in list(range(q0, q1)) + list(range(s0, s1))], default=0)
    postings = sum(len(s) for s in sketches)
    stride = longest + 1
    lists = LDS_BUDGET // (4 * stride)
    if lists >= 2 and 0 < postings < 2**32:
        tq = min(lists // 2, nq, MAX_TQ)
        ts = min(lists - tq, ns, MAX_TILE_THREADS // tq)
        return {
            "path": "tile", "longest": longest, "lists": lists, "tq": tq, "ts": ts, "tiles_q": -(-nq // tq), "tiles_s": -(-ns // ts),
            "threads": -(-tq * ts // WAVE) * WAVE, "lds_bytes": (tq + ts) * stride * 4,
        }  # fmt: skip
    return {"path": "wave", "longest": longest, "lists": lists, "blocks": -(-nq * ns // (THREADS // WAVE))}


# ---------------------------------------------------------------- 1. geometry ladder
# governing length -> (lists, tq, ts) for an all-pairs call over the five sketches of `ladder_case`.  The first row of the
# ladder, longest = 8 -> 4437 lists -> tq = ts = 32 and 1024 threads, needs 32 rows and columns: it is `short_case`.
LADDER = {
    9983: (4, 2, 2),
    9984: (3, 1, 2),
    13311: (3, 1, 2),
    13312: (2, 1, 1),
    19967: (2, 1, 1),  # dynamic LDS of exactly the budget
    19968: (1, None, None),  # one wavefront per pair
}
LADDER_LONG = 1  # where the governing list sits
TRUNCATED_LEN, TRUNCATED_MS = 25_000, (19967, 19968)  # a longer list cut by m at either side of the last threshold


def _long_list(length: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """(``length`` sorted distinct hashes in [1, 2^64 - 2], sorted hashes that are not among them)."""
    rng = np.random.default_rng([19, seed])
    pool = np.unique(rng.integers(1, TOP - 1, size=length + 96, dtype=np.uint64, endpoint=True))
    assert pool.size >= length + 48
    pick = np.zeros(pool.size, dtype=bool)
    pick[rng.choice(pool.size, size=length, replace=False)] = True
    return pool[pick], pool[~pick]


@lru_cache(maxsize=None)
def ladder_case(length: int, edge: int | None = None) -> list[np.ndarray]:
    """Five sketches: one of exactly ``length`` hashes and four of at most 8.  ``edge`` (default ``length``) is the m the
    short lists are built around: sketch 0 holds one hash below the long list and the long list's elements edge - 3 ..
    edge (those that exist), so the m-th union element of that pair is element edge - 2 and the next two must not count."""
    edge = length if edge is None else edge
    long, other = _long_list(length, length)
    u64 = lambda *v: np.array(sorted(v), dtype=np.uint64)  # noqa: E731
    below = int(long[0]) - 1 if int(long[0]) > 1 else 0
    s0 = u64(below, *[int(long[i]) for i in range(max(edge - 3, 0), min(edge + 1, length))])
    s2 = u64(0, int(other[0]), int(other[1]), int(long[length // 2]), int(other[2]), int(long[-1]), TOP)
    s3 = u64(*[int(long[i]) for i in range(max(length - 2, 0), length)], int(other[3]))
    sketches = [s0, long, s2, s3, np.empty(0, dtype=np.uint64)]
    assert all(len(s) <= 8 for g, s in enumerate(sketches) if g != LADDER_LONG) and len(long) == length
    return sketches


def ladder_runs() -> list[tuple[str, int, int | None, int]]:
    """(name, length of the governing list, edge, m): every row of ``LADDER`` with m = its length, then the 25 000-hash
    list with m at either side of the threshold between the two kernels."""
    runs = [(f"longest {length}", length, None, length) for length in LADDER]
    runs += [(f"{TRUNCATED_LEN} cut to {m}", TRUNCATED_LEN, TRUNCATED_MS[0], m) for m in TRUNCATED_MS]
    return runs


# ---------------------------------------------------------------- 2. many short lists
SHORT_N, SHORT_POOL, SHORT_MS = 70, 40, (8, 3, 1)
SHORT_WINDOWS = (((0, 70), (0, 70)), ((3, 40), (35, 70)), ((0, 5), (0, 7)), ((69, 70), (0, 70)))
# index -> what it is; the rest are random draws of 0..8 values of the pool
SHORT_FIXED = {
    0: "empty", 1: "first eight", 2: "first eight again", 3: "prefix of four", 4: "even", 5: "odd", 6: "0 and 2^64-1", 7: "2^64-1",
    33: "empty", 36: "first eight again", 69: "0 and 2^64-1",
}  # fmt: skip


@lru_cache(maxsize=None)
def short_case() -> tuple[list[np.ndarray], np.ndarray]:
    """(70 sketches of 0..8 hashes, the pool of 40 values they are drawn from: 0, 2^64 - 1 and 38 random ones)."""
    rng = np.random.default_rng(7070)
    pool = np.unique(np.concatenate([rng.integers(1, TOP - 1, size=SHORT_POOL - 2, dtype=np.uint64), np.array([0, TOP], dtype=np.uint64)]))
    assert pool.size == SHORT_POOL and pool[0] == 0 and pool[-1] == TOP
    made = {
        "empty": pool[:0], "first eight": pool[:8], "first eight again": pool[:8], "prefix of four": pool[:4], "even": pool[2:10:2],
        "odd": pool[3:11:2], "0 and 2^64-1": pool[[0, -1]], "2^64-1": pool[-1:],
    }  # fmt: skip
    sketches = []
    for g in range(SHORT_N):
        if g in SHORT_FIXED:
            sketches.append(made[SHORT_FIXED[g]].copy())
        else:
            size = int(rng.integers(0, 9))
            sketches.append(np.sort(pool[rng.choice(SHORT_POOL, size=size, replace=False)]))
    return sketches, pool


# ---------------------------------------------------------------- 3. wave kernel
WAVE_LONG = 20_000
WAVE_A, WAVE_B = 0, 5  # the two long lists; 1..4 hold 0, 1, 3 and 70 hashes
WAVE_WHERE = ("last step", "first step", "tie across lanes")  # of a lane's slice: where the m-th union element falls


def merge_steps(a: np.ndarray, b: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The na + nb steps of the merge with ties taking A first: (step is an A step, step is a new union element, A step
    whose element B holds too)."""
    tagged = np.concatenate([np.stack([a, np.zeros_like(a)]), np.stack([b, np.ones_like(b)])], axis=1)
    order = np.lexsort((tagged[1], tagged[0]))
    value, from_b = tagged[0][order], tagged[1][order].astype(bool)
    repeat = np.zeros(value.size, dtype=bool)
    repeat[1:] = from_b[1:] & ~from_b[:-1] & (value[1:] == value[:-1])
    tie_a = np.zeros(value.size, dtype=bool)
    tie_a[:-1] = repeat[1:]
    return ~from_b, ~repeat, tie_a


@lru_cache(maxsize=None)
def wave_case() -> tuple[list[np.ndarray], dict]:
    """(six sketches, facts).  ``facts`` = {"per": merge steps per lane of the pair of the two long lists, "m": {"last
    step", "first step", "tie across lanes": m}, "lane": {the same keys: the lane the m-th union element falls in}}: the
    m-th union element of that pair falls on the last step of a lane's slice, on the first, and on an A step at the end
    of a slice whose equal B element is the first step of the next lane."""
    a, other = _long_list(WAVE_LONG, 3)
    rng = np.random.default_rng(20_000)
    fresh = np.unique(rng.integers(1, TOP - 1, size=WAVE_LONG, dtype=np.uint64))
    fresh = fresh[~np.isin(fresh, a)]
    shared = a[::3]
    b = np.unique(np.concatenate([shared, fresh[: WAVE_LONG - shared.size]]))
    assert b.size == WAVE_LONG and np.intersect1d(a, b).size == shared.size
    e70 = np.unique(np.concatenate([a[100:18_000:512], other[:35]]))
    assert e70.size == 70
    sketches = [a, np.empty(0, dtype=np.uint64), a[5:6].copy(), np.array([0, int(a[100]), TOP], dtype=np.uint64), e70, b]
    total = a.size + b.size
    per = -(-total // WAVE)
    is_a, new, tie_a = merge_steps(a, b)
    seen = np.cumsum(new)  # union elements after each step
    floor = LDS_BUDGET // 8  # m below this would put the call on the tile path
    m, lane = {}, {}
    for name in WAVE_WHERE:
        for ln in range(WAVE - 2, 0, -1):  # from the top: m stays above the threshold between the kernels
            first, last = ln * per, (ln + 1) * per - 1
            if last + 1 >= total or ln in lane.values():
                continue
            at = {"last step": last, "first step": first, "tie across lanes": last}[name]
            fits = new[at] and (name != "tie across lanes" or (is_a[at] and tie_a[at]))
            if name == "last step":
                fits = fits and not tie_a[at]
            if fits and seen[at] >= floor:
                m[name], lane[name] = int(seen[at]), ln
                break
        assert name in m, f"no lane puts the m-th union element on its {name}: another seed"
    return sketches, {"per": per, "total": total, "m": m, "lane": lane}


# ---------------------------------------------------------------- 4. pa_ani_mash
ANI_VALUES = (0, 1, 2, 999, 1000, 2**32 - 1)
ANI_SIZES = (1, 255, 256, 257)
ANI_KS = (1, 21, 31, 64)
ANI_GRID = tuple((c, d) for c in ANI_VALUES for d in ANI_VALUES)


def ani_vectors(size: int) -> tuple[np.ndarray, np.ndarray]:
    """(common, denom) uint32 vectors of ``size``: the grid cycled, started where the single entry of size 1 is
    (999, 1000)."""
    at = (np.arange(size) + ANI_GRID.index((999, 1000)) * size) % len(ANI_GRID)
    grid = np.array(ANI_GRID, dtype=np.uint64)
    return grid[at, 0].astype(np.uint32), grid[at, 1].astype(np.uint32)


@lru_cache(maxsize=None)
def ani_reference(k: int) -> dict:
    """(common, denom) -> None where the result is NaN, else (1 + ln(2j / (1 + j)) / k, ln(2j / (1 + j))) as ``Decimal``
    at 60 digits."""
    getcontext().prec = 60
    out = {}
    for c, d in ANI_GRID:
        if c == 0 or d == 0:
            out[(c, d)] = None
            continue
        j = Decimal(c) / Decimal(d)
        ln = (2 * j / (1 + j)).ln()
        out[(c, d)] = (1 + ln / k, ln)
    return out


def ani_error_in_units(value: float, c: int, d: int, k: int) -> float:
    """|value - reference| in units of u = 2^-52 max(1, |ln(2j / (1 + j))| / k)."""
    getcontext().prec = 60
    ref, ln = ani_reference(k)[(c, d)]
    unit = Decimal(2) ** -52 * max(Decimal(1), abs(ln) / k)
    return float(abs(Decimal(float(value)) - ref) / unit)


# ---------------------------------------------------------------- 5. pa_sketch_bottom: a threshold raised once
ESCALATION_K, ESCALATION_M = 21, 100
ESCALATION_RANDOM, ESCALATION_UNIT, ESCALATION_COPIES = 20_000, 2_000, 25


@lru_cache(maxsize=None)
def escalation_genomes() -> list[bytes]:
    """A random genome of 20 kb, the shortest, which sets the first threshold at 4m / 20 000 = 2 % of the hash space, and
    a genome of 25 copies of a random 2 kb unit: about 2 000 distinct k-mers, some 40 of them under the first threshold
    and some 320 under the second (16 %)."""
    rng = np.random.default_rng(515)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    random = letters[rng.integers(0, 4, ESCALATION_RANDOM)].tobytes()
    unit = letters[rng.integers(0, 4, ESCALATION_UNIT)].tobytes()
    return [random, unit * ESCALATION_COPIES]


def escalation_thresholds(lengths: list[int], m: int) -> list[int]:
    """``max_hash`` of each turn of ``pa_sketch_bottom``'s loop, up to and including the maximum."""
    frac, out = 4.0 * m / min(x for x in lengths if x), []
    while True:
        out.append(TOP if frac >= 1.0 else int(frac * 18446744073709551616.0))
        if frac >= 1.0:
            return out
        frac *= 8.0
