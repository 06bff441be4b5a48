"""The cases of tests/pair_phase_cases.py against the kernels they are aimed at, without a GPU.

The constants of ``row_sum_kernel``, the slot function and the dictionary's size are read from csrc/pairs_bitrow.hip; if
one of them changes, a test here fails and says that tests/pair_phase_cases.py has to follow, so that the GPU tests
(tests/test_gpu_pair_edges.py) do not quietly stop reaching the flush or the long probe chains."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from tests import pair_phase_cases as cases

SOURCE = Path(__file__).resolve().parent.parent / "pyani_plus_amd" / "csrc" / "pairs_bitrow.hip"
FOLLOW = "tests/pair_phase_cases.py restates this and its cases are sized by it: change it there too"
TPRS = sorted(cases.FLUSH_TILE)


def _find(pattern: str, text: str, what: str) -> re.Match:
    m = re.search(pattern, text, re.S)
    assert m, f"csrc/pairs_bitrow.hip: {what} no longer has the form this test reads ({pattern!r}); {FOLLOW}"
    return m


@pytest.fixture(scope="module")
def kernel() -> dict:
    """What the source says: the counters' constants, the slot function's multiplier, the dictionary's size."""
    text = SOURCE.read_text()
    out = {name: int(_find(rf"constexpr \w+ {name} = (\d+);", text, name).group(1)) for name in ("kThreads", "kPlanes", "kBatch", "kMaxTileSubjects")}
    _find(r"if \(pending \+ kBatch > \(1u << kPlanes\) - 1u\) flush\(\);", text, "the in-loop flush")
    _find(r"j0 \+= \(uint64_t\)kRowsPerIter \* kBatch\)", text, "the loop's step")
    _find(r"constexpr int kRowsPerIter = kThreads / TPR;", text, "the rows of a turn")
    tpr = re.findall(r"const int tpr = \(int\)\(\(cols \+ (\d+)u\) / (\d+)u\);", text)
    assert len(tpr) == 2 and all(int(b) == int(a) + 1 for a, b in tpr), f"csrc/pairs_bitrow.hip: threads per row of a tile; {FOLLOW}"
    out["cols_per_thread"] = int(tpr[0][1])
    body = _find(r"uint32_t slot_of\(uint64_t h, uint32_t cap\) \{(.*?)\n\}", text, "slot_of").group(1)
    out["multiplier"] = int(_find(r"x = \(\(uint32_t\)h \* (0x[0-9A-Fa-f]+)u\) \^ \(uint32_t\)\(h >> 32\);", body, "slot_of's mix").group(1), 16)
    _find(r"return \(uint32_t\)\(\(\(uint64_t\)x \* cap\) >> 32\);", body, "slot_of's multiply-shift")
    out["cap64"] = _find(r"const uint64_t cap64 = ([^;]+);", text, "cap64 of dict_insert").group(1).strip()
    assert re.fullmatch(r"[n_post0-9 +*/()]+", out["cap64"]), f"cap64 = {out['cap64']}; {FOLLOW}"
    assert len(re.findall(r"if \(\+\+slot == cap\) slot = 0;", text)) == 2, f"csrc/pairs_bitrow.hip: the probe's wrap; {FOLLOW}"
    return out


def _lane(n_hashes: int, tpr: int, planes: int, batch: int, threads: int, slot: int = 0) -> tuple[int, int]:
    """The turns of one lane of ``row_sum_kernel`` over a query of ``n_hashes``: (flushes inside the loop, turns taken
    after the last of them)."""
    rows, pending, flushes, after = threads // tpr, 0, 0, 0
    for _j0 in range(slot, n_hashes, rows * batch):
        after += 1
        pending += batch
        if pending + batch > 2**planes - 1:
            pending, flushes, after = 0, flushes + 1, 0
    return flushes, after


def test_case_module_restates_the_kernel_constants(kernel):
    got = (kernel["kPlanes"], kernel["kBatch"], kernel["kThreads"], kernel["kMaxTileSubjects"], kernel["cols_per_thread"])
    want = (cases.PLANES, cases.BATCH, cases.THREADS, cases.MAX_TILE_SUBJECTS, cases.COLS_PER_THREAD)
    assert got == want, f"kPlanes, kBatch, kThreads, kMaxTileSubjects, columns per thread are {got} in the kernel, {want} in the cases; {FOLLOW}"
    assert kernel["multiplier"] == cases.SLOT_MULTIPLIER, f"slot_of multiplies by {kernel['multiplier']:#x}; {FOLLOW}"


@pytest.mark.parametrize("tpr", TPRS)
def test_flush_cases_reach_two_in_loop_flushes(kernel, tpr):
    planes, batch, threads = kernel["kPlanes"], kernel["kBatch"], kernel["kThreads"]
    sketches, facts = cases.flush_case(tpr)
    n, query = len(sketches), sketches[facts["query"]]
    assert n <= kernel["kMaxTileSubjects"] and -(-n // kernel["cols_per_thread"]) == tpr == cases.tile_tpr(n), f"{n} subjects are not one tile of {tpr} threads per row; {FOLLOW}"
    if tpr == 3:
        assert threads % tpr == 1  # one thread past the last whole row sits the loop out
    need = 2 * cases.flush_rows(tpr, planes, batch, threads)
    assert len(query) >= need + 1000, f"TPR {tpr}: the query has {len(query)} hashes, two in-loop flushes and a tail need {need + 1000}; {FOLLOW}"
    for slot in (0, threads // tpr - 1):
        flushes, after = _lane(len(query), tpr, planes, batch, threads, slot)
        assert flushes >= 2 and after >= 1, f"TPR {tpr}, row {slot} of a turn: {flushes} in-loop flushes, {after} turns after; {FOLLOW}"
    # the hashes of the tail follow every lane's second flush, those of the head precede every lane's first
    assert len(query) - cases.FLUSH_TAIL >= need and cases.FLUSH_HEAD <= need // 2, FOLLOW
    # the emulation's flush points are those of the formula
    assert _lane(need // 2, tpr, planes, batch, threads) == (1, 0) and _lane(need // 2 + 1, tpr, planes, batch, threads) == (1, 1)


def test_the_old_70_000_hash_shape_never_flushed_in_the_loop(kernel):
    """[70 000, 500, 66 000] of test_gpu_parity_random.py: three subjects, one thread per row, 274 rows per lane."""
    planes, batch, threads = kernel["kPlanes"], kernel["kBatch"], kernel["kThreads"]
    for slot in (0, 255):
        assert _lane(70_000, 1, planes, batch, threads, slot)[0] == 0
    assert _lane(70_000, 1, 8, 1, threads)[0] >= 1  # it did with eight planes and a row per turn


@pytest.mark.parametrize("tpr", TPRS)
def test_flush_case_sketches_and_oracle_counts(tpr):
    sketches, facts = cases.flush_case(tpr)
    n, i = len(sketches), facts["query"]
    for s in sketches:
        assert s.dtype == np.uint64 and np.all(s[1:] > s[:-1])
    cols = facts["columns"]
    assert sorted(cols) == sorted(cases.FLUSH_KINDS) and len(set(cols.values())) == 6
    assert {0, 31, 32, n - 1} <= set(cols.values()) and (tpr == 1 or {127, 128} <= set(cols.values()))
    sizes = [len(s) for s in sketches]
    assert all(4 <= sizes[c] <= 12 for c in range(n) if c not in cols.values())
    want = facts["row"]
    q = len(sketches[i])
    assert [int(want[cols[kind]]) for kind in cases.FLUSH_KINDS] == [q, (q + 1) // 2, 5000, 3000, 0, 0]
    row = oracle.pair_counts(sketches, (i, i + 1), (0, n), threads=8)[0]
    assert np.array_equal(row, want)
    column = oracle.pair_counts(sketches, (0, n), (i, i + 1), threads=8)[:, 0]
    assert np.array_equal(column, want)
    shared = want[[c for c in range(n) if c not in cols.values()]]
    assert shared.min() == 0 and shared.max() >= 8  # small sketches inside, outside and across the query


def test_clustered_case_lands_on_its_slots(kernel):
    sketches, facts = cases.clustered_case()
    ns, cap = facts["n_subjects"], facts["cap"]
    n_post = sum(len(s) for s in sketches[:ns])
    # the kernel's expressions, evaluated: the slot function with the parsed multiplier, cap64 as written
    assert eval(kernel["cap64"].replace("/", "//"), {"n_post": n_post}) == cases.dict_cap(n_post) == cap, f"cap64 = {kernel['cap64']}; {FOLLOW}"  # noqa: S307
    for n in (0, 1, 3, 4095, 10**6 + 1):
        assert eval(kernel["cap64"].replace("/", "//"), {"n_post": n}) == cases.dict_cap(n), FOLLOW  # noqa: S307

    def slot(h: int) -> int:
        x = (((h & 0xFFFFFFFF) * kernel["multiplier"]) & 0xFFFFFFFF) ^ (h >> 32)
        return (x * cap) >> 32

    probe = np.concatenate([np.concatenate(sketches), np.array([0, 1, 2**32, 2**64 - 2], dtype=np.uint64)])
    assert [slot(int(h)) for h in probe] == cases.slot_of(probe, cap).tolist(), f"slot_of differs from the kernel's; {FOLLOW}"
    assert int(cases.slot_of(12345678901234567890, cap)) == slot(12345678901234567890)
    assert facts["slots"] == {"end": cap - 1, "middle": cap // 2}
    subject_keys = set(np.concatenate(sketches[:ns]).tolist())
    for group, target in facts["slots"].items():
        keys, absent = facts["keys"][group], facts["absent"][group]
        assert len(set(keys.tolist())) == cases.CLUSTER_KEYS[group] >= 1000 and set(keys.tolist()) <= subject_keys
        assert {slot(int(h)) for h in keys} == {slot(int(h)) for h in absent} == {target}, f"{group}: keys off their slot; {FOLLOW}"
        assert len(absent) == cases.CLUSTER_ABSENT and not set(absent.tolist()) & subject_keys
        assert any(set(absent.tolist()) & set(q.tolist()) for q in sketches[ns:])
    assert len(subject_keys) == sum(cases.CLUSTER_KEYS.values()) and 0 not in subject_keys and cases.TOP not in subject_keys
    # the chain from the last slot runs over the end of the table and stays clear of the middle one
    assert cases.CLUSTER_KEYS["end"] < cap // 2 - 300 and cap // 2 + cases.CLUSTER_KEYS["middle"] + 300 < cap - 1
    assert [len(s) for s in sketches[:ns]] == list(cases.CLUSTER_SUBJECT_SIZES) and len(sketches) == ns + 4
    for s in sketches:
        assert s.dtype == np.uint64 and np.all(s[1:] > s[:-1])
    held = [set(q.tolist()) for q in sketches[ns:]]
    assert sum(0 in q for q in held) >= 1 and sum(cases.TOP in q for q in held) >= 1
    want = cases.set_counts(sketches)
    assert np.array_equal(oracle.pair_counts(sketches), want)
    assert want[ns + 1, :ns].sum() == 0 and want[ns + 2, :ns].sum() >= cases.CLUSTER_KEYS["end"]  # only absent keys; the whole chain
    assert all(want[a, b] > 0 for a in range(ns - 1) for b in (a + 1,))  # neighbouring subjects overlap


def test_ani_cases_cover_the_edge_paths():
    shapes = cases.ani_shapes()
    assert {(c.shape, q, s, mis) for _z, c, q, s, mis in shapes} >= {
        ((1, 1), (0, 1), (0, 1), 0), ((1, 2), (0, 1), (0, 2), 0), ((3, 3), (0, 3), (0, 3), 0), ((5, 7), (0, 5), (0, 7), 0),
        ((4, 6), (3, 7), (1, 7), 0), ((2, 513), (0, 2), (0, 513), 0), ((70_000, 3), (0, 70_000), (0, 3), 0), ((6, 8), (0, 6), (0, 8), 1),
    }  # fmt: skip
    seen_sizes, pairs, full = set(), set(), 0
    for sizes, counts, q_range, s_range, _mis in shapes:
        assert counts.dtype == np.uint32 and counts.shape == (q_range[1] - q_range[0], s_range[1] - s_range[0]) and q_range[1] <= len(sizes) >= s_range[1]
        seen_sizes |= set(sizes)
        q = np.array(sizes[q_range[0] : q_range[1]], dtype=np.uint64)[:, None]
        s = np.array(sizes[s_range[0] : s_range[1]], dtype=np.uint64)[None, :]
        assert np.all(counts <= np.minimum(q, s))
        full += int(np.sum((counts == q) & (counts == s)))
        even = counts[:, : counts.shape[1] // 2 * 2].reshape(counts.shape[0], -1, 2)
        pairs |= {(bool(a), bool(b)) for a, b in even.reshape(-1, 2)[:5000]}
    assert seen_sizes >= {1, 2, 3, 1000, 10**6, 2**32 + 5}
    assert pairs == {(False, False), (False, True), (True, False), (True, True)} and full >= 10
    every = cases.ani_cases()
    assert len(every) == len(shapes) * 6 and {c[4] for c in every} == {1, 7, 21, 31, 51, 64}
