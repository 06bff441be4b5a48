"""Inputs aimed at the edges of the pair phase: the in-loop flush of ``row_sum_kernel``'s bit-sliced counters, long probe
chains in the hash dictionary, and the shapes, offsets and extremes of ``ani_kernel``.

Used by tests/test_pair_phase_cases.py (no GPU: the cases against the constants parsed from csrc/pairs_bitrow.hip) and
by tests/test_gpu_pair_edges.py (the kernels against the oracle).  The constants below restate the kernel's; when the
kernel's change, change them here, and the sizes of the cases follow."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

# csrc/pairs_bitrow.hip: kPlanes, kBatch, kThreads, kMaxTileSubjects, and the columns one thread of a bit row covers
PLANES, BATCH, THREADS, MAX_TILE_SUBJECTS, COLS_PER_THREAD = 10, 8, 256, 2048, 128
SLOT_MULTIPLIER = 0x9E3779B1
TOP = 2**64 - 1  # a legal hash, and the dictionary's empty marker
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- row sums across counter flushes
def flush_rows(tpr: int, planes: int = PLANES, batch: int = BATCH, threads: int = THREADS) -> int:
    """Query hashes beyond which lane 0 has flushed its counters inside the loop and gone on adding: a lane flushes once
    ``pending + batch > 2^planes - 1``, and a turn of the workgroup takes ``batch`` rows for each of its
    ``threads // tpr`` whole rows of threads."""
    return -(-(2**planes - batch) // batch) * batch * (threads // tpr)


def tile_tpr(n_subjects: int) -> int:
    """Threads per bit row of a tile of ``n_subjects`` columns."""
    return (n_subjects + COLS_PER_THREAD - 1) // COLS_PER_THREAD


# subjects in the tile that put it at the wanted threads per row: 128 -> 1, 300 -> 3 (256 % 3: one idle thread), 2000 -> 16
FLUSH_TILE = {1: 128, 3: 300, 16: 2000}
FLUSH_TAIL, FLUSH_HEAD = 5000, 3000
# the sketches that matter, in this order, at the columns `flush_columns` gives
FLUSH_KINDS = ("query", "every second", "tail", "head", "disjoint", "empty")


def flush_query_len(tpr: int) -> int:
    """Two in-loop flushes of every lane, then a tail longer than ``FLUSH_TAIL`` (and no multiple of anything)."""
    return 2 * flush_rows(tpr) + FLUSH_TAIL + 1037


def flush_columns(n: int) -> list[int]:
    """Where the six sketches of ``FLUSH_KINDS`` sit: the last column of the tile and the columns next to word and thread
    edges (0, 31 | 32, 127 | 128); a tile of one thread per row has no column 128 and takes 64 | 63 instead."""
    cols: list[int] = []
    for c in (n - 1, 0, 31, 32, 127, 128, 64, 63):
        if c < n and c not in cols:
            cols.append(c)
    return cols[: len(FLUSH_KINDS)]


@lru_cache(maxsize=None)
def flush_case(tpr: int) -> tuple[list[np.ndarray], dict]:
    """(sketches, facts): one long query among ``FLUSH_TILE[tpr]`` sketches.  ``facts`` = {"query": its index, "columns":
    {kind: index}, "row": the query's row of intersection sizes as the construction implies it}."""
    n = FLUSH_TILE[tpr]
    rng = np.random.default_rng([2025, tpr])
    n_query = flush_query_len(tpr)
    pool = np.unique(rng.integers(0, 2**63, size=n_query + 60_000, dtype=np.uint64))
    pool = pool[rng.permutation(pool.size)]
    query, outside = np.sort(pool[:n_query]), pool[n_query:]
    assert query.size == n_query and outside.size > 40_000
    special = {
        "query": query,  # every lane's counter reaches the flush value with all upper planes set, twice
        "every second": query[::2],
        "tail": query[-FLUSH_TAIL:],  # added after the flushes: planes that were not reset, a dropped tail
        "head": query[:FLUSH_HEAD],  # added before the first flush
        "disjoint": np.sort(outside[:4000]),
        "empty": np.empty(0, dtype=np.uint64),
    }
    columns = dict(zip(FLUSH_KINDS, flush_columns(n)))
    sketches: list[np.ndarray] = [None] * n  # type: ignore[list-item]
    row = np.zeros(n, dtype=np.uint32)
    for kind, col in columns.items():
        sketches[col] = special[kind]
    row[columns["query"]], row[columns["every second"]] = n_query, (n_query + 1) // 2
    row[columns["tail"]], row[columns["head"]] = FLUSH_TAIL, FLUSH_HEAD
    spare = outside[4000:]
    for col in range(n):
        if sketches[col] is not None:
            continue
        size = int(rng.integers(4, 13))
        shared = int(rng.integers(0, size + 1))  # so many of the query's hashes, the rest from outside it
        mine = query[rng.choice(n_query, size=shared, replace=False)]
        other = spare[rng.choice(spare.size, size=size - shared, replace=False)]
        sketches[col] = np.sort(np.concatenate([mine, other]))
        row[col] = shared
    return sketches, {"query": columns["query"], "columns": columns, "row": row}


# ---------------------------------------------------------------- hash dictionary with long probe chains
def slot_of(h, cap):
    """``slot_of`` of csrc/pairs_bitrow.hip: an int, or an array of uint64 -> the first slot probed in a table of ``cap``."""
    h = np.asarray(h, dtype=np.uint64)
    x = (((h & np.uint64(_M32)) * np.uint64(SLOT_MULTIPLIER)) & np.uint64(_M32)) ^ (h >> np.uint64(32))
    return (x * np.uint64(cap)) >> np.uint64(32)


def dict_cap(n_post: int) -> int:
    """Slots of the dictionary of a tile with ``n_post`` subject postings (``cap64`` of ``dict_insert``)."""
    return n_post + n_post // 2 + 1024


def keys_on_slot(rng, slot: int, cap: int, count: int) -> np.ndarray:
    """``count`` distinct keys whose first probe is ``slot``: the low 32 bits are drawn, the high 32 solved for."""
    x_lo, x_hi = -(-(slot << 32) // cap), -(-((slot + 1) << 32) // cap)  # x with (x * cap) >> 32 == slot
    assert x_hi - x_lo >= 4 * count
    x = x_lo + rng.choice(x_hi - x_lo, size=count, replace=False).astype(np.uint64)
    lo = rng.choice(2**32 - 1, size=count, replace=False).astype(np.uint64)
    hi = x ^ ((lo * np.uint64(SLOT_MULTIPLIER)) & np.uint64(_M32))
    return (hi << np.uint64(32)) | lo


CLUSTER_SUBJECT_SIZES = (1000, 800, 700, 500, 300, 100)
CLUSTER_KEYS = {"end": 1500, "middle": 1000, "random": 300}  # distinct subject keys per group
CLUSTER_ABSENT = 150  # keys per target slot that only queries hold


@lru_cache(maxsize=None)
def clustered_case() -> tuple[list[np.ndarray], dict]:
    """(sketches, facts): six subjects first, then four queries.  In the dictionary of the subject tile, 1 500 keys start
    at the last slot (the chain runs over the end of the table) and 1 000 at the middle one.  ``facts`` = {"n_subjects",
    "cap", "slots": {group: slot}, "keys": {group: keys of the subjects}, "absent": {group: keys of queries only}}."""
    rng = np.random.default_rng(4242)
    n_post = sum(CLUSTER_SUBJECT_SIZES)
    cap = dict_cap(n_post)
    slots = {"end": cap - 1, "middle": cap // 2}
    drawn = {g: keys_on_slot(rng, s, cap, CLUSTER_KEYS[g] + CLUSTER_ABSENT) for g, s in slots.items()}
    keys = {g: drawn[g][: CLUSTER_KEYS[g]] for g in slots}
    absent = {g: drawn[g][CLUSTER_KEYS[g] :] for g in slots}
    keys["random"] = rng.integers(1, 2**63, size=CLUSTER_KEYS["random"], dtype=np.uint64)
    every = np.concatenate([keys["end"], keys["middle"], keys["random"]])
    assert np.unique(every).size == every.size
    every = every[rng.permutation(every.size)]
    # overlapping windows of the shuffled keys that together hold every key
    subjects, begin, last = [], 0.0, CLUSTER_SUBJECT_SIZES[-1]
    step = (every.size - last) / (n_post - last)
    for size in CLUSTER_SUBJECT_SIZES:
        at = int(round(begin))
        subjects.append(np.sort(every[at : at + size]))
        begin += size * step
    assert np.unique(np.concatenate(subjects)).size == every.size
    both_absent = np.concatenate([absent["end"], absent["middle"]])
    edge = np.array([0, TOP], dtype=np.uint64)
    queries = [
        np.concatenate([every[:500], absent["end"][:100], absent["middle"][:100], edge]),
        np.concatenate([both_absent, edge[:1]]),  # nothing but lookups that end at an empty slot
        np.concatenate([keys["end"], edge[1:]]),  # the whole chain over the end of the table
        np.concatenate([every[rng.choice(every.size, size=700, replace=False)], both_absent[::3]]),
    ]
    sketches = subjects + [np.sort(q) for q in queries]
    return sketches, {"n_subjects": len(subjects), "cap": cap, "slots": slots, "keys": keys, "absent": absent}


def set_counts(sketches: list[np.ndarray]) -> np.ndarray:
    """All intersection sizes from Python sets (small cases only)."""
    sets = [set(s.tolist()) for s in sketches]
    return np.array([[len(a & b) for b in sets] for a in sets], dtype=np.uint32)


# ---------------------------------------------------------------- ANI transform: shapes, offsets, extremes
ANI_KS = (1, 7, 21, 31, 51, 64)
ANI_SIZE_POOL = (1, 2, 3, 1000, 10**6, 2**32 + 5, 1000, 3)  # repeats: pairs of different genomes of one size
_U32_MAX = 2**32 - 1


def _ani_block(seed: int, n: int, q_range, s_range):
    """Sizes of ``n`` genomes from the pool and a block of counts: 0, 1, min(|Q|, |S|) or a value between them."""
    rng = np.random.default_rng([77, seed])
    pool = np.array(ANI_SIZE_POOL, dtype=np.uint64)
    sizes = pool[(np.arange(n) + seed) % pool.size] if n >= pool.size else pool[rng.integers(0, pool.size, size=n)]
    q, s = sizes[q_range[0] : q_range[1]], sizes[s_range[0] : s_range[1]]
    most = np.minimum(np.minimum.outer(q, s), np.uint64(_U32_MAX))
    kind = rng.choice(4, size=most.shape, p=[0.35, 0.15, 0.25, 0.25])
    between = np.minimum(most, np.uint64(1) + (rng.integers(0, 2**62, size=most.shape).astype(np.uint64) % most))
    counts = np.select([kind == 0, kind == 1, kind == 2], [np.uint64(0), np.uint64(1), most], between)
    return [int(x) for x in sizes], np.ascontiguousarray(counts, dtype=np.uint32)


@lru_cache(maxsize=None)
def ani_shapes() -> list[tuple]:
    """(sizes of all genomes, counts [nq, ns], q_range, s_range, misalign): ``misalign`` = elements by which the counts
    start inside their buffer (1: rows on 4-byte boundaries, the whole matrix takes the scalar path)."""
    big = 2**32 + 5
    shapes = [
        ([1000], np.array([[1000]], dtype=np.uint32), (0, 1), (0, 1), 0),  # 1 x 1
        ([3, big], np.array([[3, 0]], dtype=np.uint32), (0, 1), (0, 2), 0),  # 1 x 2: (c, 0)
        ([3, big], np.array([[0, _U32_MAX]], dtype=np.uint32), (1, 2), (0, 2), 0),  # 1 x 2: (0, c) at q0 = 1
        ([1, 2, 10**6], np.array([[1, 0, 1], [0, 2, 1], [1, 2, 10**6]], dtype=np.uint32), (0, 3), (0, 3), 0),  # 3 x 3
    ]
    for seed, (n, q_range, s_range, misalign) in enumerate([
        (7, (0, 5), (0, 7), 0),  # 5 x 7: odd rows start unaligned
        (9, (3, 7), (1, 7), 0),  # a 4 x 6 window at odd q0 and s0 inside 9 genomes
        (513, (0, 2), (0, 513), 0),  # two column blocks and an odd tail
        (70_000, (0, 70_000), (0, 3), 0),  # more rows than the grid has rows of blocks
        (8, (0, 6), (0, 8), 1),  # even ns, rows 4-byte aligned
    ]):  # fmt: skip
        sizes, counts = _ani_block(seed, n, q_range, s_range)
        shapes.append((sizes, counts, q_range, s_range, misalign))
    return shapes


def ani_cases() -> list[tuple]:
    """(sizes, counts, q_range, s_range, k, misalign) for every shape and every k of ``ANI_KS``."""
    return [(sizes, counts, q, s, k, mis) for sizes, counts, q, s, mis in ani_shapes() for k in ANI_KS]
