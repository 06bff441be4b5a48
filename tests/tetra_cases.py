"""The independent restatement of the TETRA-hip definition (include/pyani_hip.h) and the inputs
aimed at the edges of ``pa_tetra_counts`` and ``pa_tetra_corr``.

Two layers, neither of which goes through the library:

* counts from the FASTA text with numpy: a code array per record, window validity, ``bincount``;
* Z-scores, unit rows and r in plain Python floats (IEEE doubles, one operation per step, in the contract's order), so
  that they can be compared with the host twins bit for bit.

The definition is this project's own (after Teeling et al. 2004); nothing here is taken from pyani or JSpecies.

The case builders read the chunk constants from ``csrc/tetra.hip`` and the tile from ``csrc/pairs_f64_tile.h``, so that
the seam cases sit on the kernel's seams whatever those constants are.  Used by tests/test_tetra_host.py (no GPU) and tests/test_gpu_tetra.py."""

from __future__ import annotations

import math
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
BINS, WORDS, OFF3, OFF2 = 336, 256, 256, 320
_CODES = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _CODES[ord(_c)] = _CODES[ord(_c.lower())] = _i


@lru_cache(maxsize=None)
def kernel_constants() -> dict[str, int]:
    """kThreads, kBlocksPerLane and kCopies as csrc/tetra.hip states them, kTile as csrc/pairs_f64_tile.h does."""
    csrc = ROOT / "pyani_plus_amd" / "csrc"
    out = {}
    for file, names in (("tetra.hip", ("kThreads", "kBlocksPerLane", "kCopies")), ("pairs_f64_tile.h", ("kTile",))):
        text = (csrc / file).read_text()
        for name in names:
            found = re.search(rf"constexpr int {name} = (\d+);", text)
            assert found, f"{name} not found in {file}"
            out[name] = int(found.group(1))
    return out


def chunk_bases() -> int:
    """Positions one workgroup of the count kernel takes."""
    k = kernel_constants()
    return 64 * k["kThreads"] * k["kBlocksPerLane"]


# ---------------------------------------------------------------- layer 1: counts from the text
def fasta_records(text: bytes) -> list[bytes]:
    """The residue strings of a FASTA text: what precedes the first '>' is ignored, " \\t\\r\\n" leave the sequence lines."""
    records: list[list[bytes]] = []
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            records.append([])
        elif records:
            records[-1].append(line.translate(None, b" \t\r"))
    return [b"".join(parts) for parts in records]


def forward_counts(text: bytes) -> np.ndarray:
    """F of one genome: 336 forward-strand counts, windows of 2, 3 and 4 valid bases inside one record."""
    out = np.zeros(BINS, dtype=np.uint64)
    for record in fasta_records(text):
        codes = _CODES[np.frombuffer(record, dtype=np.uint8)]
        for k, off, size in ((4, 0, 256), (3, OFF3, 64), (2, OFF2, 16)):
            if len(codes) < k:
                continue
            windows = len(codes) - k + 1
            valid = np.ones(windows, dtype=bool)
            index = np.zeros(windows, dtype=np.int64)
            for i in range(k):
                part = codes[i : i + windows]
                valid &= part >= 0
                index = index * 4 + np.maximum(part, 0)
            out[off : off + size] += np.bincount(index[valid], minlength=size).astype(np.uint64)
    return out


# ---------------------------------------------------------------- layer 2: Z, U and r in Python floats
def rc_word(w: int, k: int) -> int:
    digits = [(w >> (2 * (k - 1 - i))) & 3 for i in range(k)]  # first base first
    out = 0
    for d in reversed(digits):
        out = out * 4 + (3 - d)
    return out


def both_strands(f) -> tuple[list[int], list[int], list[int]]:
    f = [int(x) for x in f]
    c4 = [f[w] + f[rc_word(w, 4)] for w in range(256)]
    c3 = [f[OFF3 + w] + f[OFF3 + rc_word(w, 3)] for w in range(64)]
    c2 = [f[OFF2 + w] + f[OFF2 + rc_word(w, 2)] for w in range(16)]
    return c4, c3, c2


def zscores(f) -> list[float]:
    c4, c3, c2 = both_strands(f)
    z = []
    for w in range(256):
        n, left, right, mid = float(c4[w]), float(c3[w >> 2]), float(c3[w & 63]), float(c2[(w >> 2) & 15])
        value = 0.0
        if mid != 0.0:
            e = (left * right) / mid
            v = (e * ((mid - left) * (mid - right))) / (mid * mid)
            if v > 0.0:
                value = (n - e) / math.sqrt(v)
        z.append(value)
    return z


def unit_row(z: list[float]) -> list[float]:
    total = 0.0
    for x in z:
        total = total + x
    mean = total / 256.0
    ss = 0.0
    for x in z:
        d = x - mean
        ss = ss + d * d  # Python rounds the product before the addition
    if ss == 0.0:
        return [math.nan] * 256
    norm = math.sqrt(ss)
    return [(x - mean) / norm for x in z]


def correlation(ua: list[float], ub: list[float], same: bool) -> float:
    acc = 0.0
    for a, b in zip(ua, ub):
        acc = acc + a * b
    if acc != acc:
        return acc
    if same:
        return 1.0
    return min(1.0, max(-1.0, acc))


def correlation_matrix(unit: list[list[float]], q_range=None, s_range=None) -> np.ndarray:
    n = len(unit)
    (q0, q1), (s0, s1) = q_range or (0, n), s_range or (0, n)
    return np.array([[correlation(unit[i], unit[j], i == j) for j in range(s0, s1)] for i in range(q0, q1)], dtype=np.float64).reshape(q1 - q0, s1 - s0)


def same_bits(got, want) -> None:
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = got.view(np.uint64) != want.view(np.uint64)
    both_nan = np.isnan(got) & np.isnan(want)
    bad = diff & ~both_nan
    assert not bad.any(), f"{int(bad.sum())} of {got.size} values differ, first at {np.argwhere(bad)[0]}: {got[bad][0]!r} != {want[bad][0]!r}"


# ---------------------------------------------------------------- inputs
def random_bases(rng, n: int, p=(0.25, 0.25, 0.25, 0.25)) -> bytes:
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=p)].tobytes()


def markov_bases(rng, n: int, skew: float) -> bytes:
    """A first-order chain whose transition rows lean on the previous base: a spectrum unlike a uniform one."""
    rows = np.full((4, 4), (1.0 - skew) / 4)
    for b in range(4):
        rows[b, (b + 1 + int(skew * 10)) % 4] += skew
    out = np.empty(n, dtype=np.int64)
    state = 0
    draws = rng.random(n)
    cum = np.cumsum(rows, axis=1)
    for i in range(n):
        state = int(np.searchsorted(cum[state], draws[i]))
        state = min(state, 3)
        out[i] = state
    return np.frombuffer(b"ACGT", dtype=np.uint8)[out].tobytes()


def fasta(*records: bytes, width: int = 70) -> bytes:
    lines = []
    for r, record in enumerate(records):
        lines.append(b">r%d" % r)
        lines.extend(record[i : i + width] for i in range(0, len(record), width))
    return b"\n".join(lines) + b"\n"


def reverse_complement(seq: bytes) -> bytes:
    return seq.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


@lru_cache(maxsize=None)
def count_cases() -> dict[str, list[bytes]]:
    """name -> the FASTA texts of the genomes of one arena.  Every list goes through the kernel in one call."""
    rng = np.random.default_rng(20040101)
    cases: dict[str, list[bytes]] = {}
    # valid lengths 0 .. 5, and the lengths around a packed word, a mask word, a block and two blocks
    cases["lengths"] = [fasta(random_bases(rng, n)) for n in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
    # two records, the one-position separator at every offset of a block
    cases["separator"] = [fasta(random_bases(rng, 64 + off), random_bases(rng, 70)) for off in range(64)]
    # one N at every offset of the second block of a 200-base genome
    texts = []
    for off in range(64):
        seq = bytearray(random_bases(rng, 200))
        seq[64 + off] = ord("N")
        texts.append(fasta(bytes(seq)))
    cases["one_n"] = texts
    # runs of 1 .. 5 N across a block edge and inside a block
    texts = []
    for run in range(1, 6):
        for at in (62, 100):
            seq = bytearray(random_bases(rng, 200))
            seq[at : at + run] = b"N" * run
            texts.append(fasta(bytes(seq)))
    cases["n_runs"] = texts
    cases["homopolymer"] = [fasta(b"A" * 100_000)]
    # three chunks and five bases, 0.1 % N: lane seams and workgroup seams carry windows, clean and masked blocks mix
    n = 3 * chunk_bases() + 5
    seq = bytearray(random_bases(rng, n))
    for at in rng.choice(n, size=n // 1000, replace=False):
        seq[at] = ord("N")
    cases["three_chunks"] = [fasta(bytes(seq), width=n)]
    # 300 genomes of one block each beside a large one; empty genomes are added by `arena_with_empty`
    cases["many_small"] = [fasta(random_bases(rng, int(m))) for m in rng.integers(40, 64, size=150)] + [fasta(random_bases(rng, 300_000), width=100_000)] + [
        fasta(random_bases(rng, int(m))) for m in rng.integers(1, 64, size=150)
    ]
    return cases


EMPTY_AT = {"many_small": (0, 7, 151, 301)}  # positions (in the final genome list) of genomes without a single block


def case_arena(name: str):
    """(HostArena, expected counts [n, 336]) of a case; ``EMPTY_AT`` inserts genomes whose start equals the next one's."""
    from pyani_plus_amd.engine import pack_genomes

    texts = count_cases()[name]
    arena = pack_genomes(list(texts), fasta=True)
    want = [forward_counts(t) for t in texts]
    starts = [int(s) for s in arena.genome_start]
    for at in EMPTY_AT.get(name, ()):
        starts.insert(at, starts[at])
        want.insert(at, np.zeros(BINS, dtype=np.uint64))
    arena.genome_start = np.array(starts, dtype=np.uint64)
    return arena, np.stack(want)


@lru_cache(maxsize=None)
def unit_rows(n: int, seed: int = 7) -> np.ndarray:
    """n unit rows from genomes of different composition (through the contract's own arithmetic, layer 2); row 1 of
    three or more is a degenerate genome's: all NaN."""
    rng = np.random.default_rng(seed)
    rows = []
    for g in range(n):
        if g == 1 and n >= 3:
            rows.append([math.nan] * 256)
            continue
        p = rng.dirichlet((8, 8, 8, 8))
        rows.append(unit_row(zscores(forward_counts(fasta(random_bases(rng, 3000, p))))))
    return np.array(rows, dtype=np.float64).reshape(n, WORDS)
