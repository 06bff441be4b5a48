"""CPU test of the k-mer hash kernel's second-product tables (pyani_plus_amd/csrc/murmur_words.h).

The kernel forms k_j = rotl(word * cA, r) * cB of every murmur word from three table values {A.hi, T, B} and one 32 x 64 bit
product.  The formulas are plain C++ shared by device and host; a small host program runs them over every word slot, every
byte count of a word and every pair of 4-base groups, and the values are compared with the MurmurHash3 definition.
"""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "pyani_plus_amd" / "csrc"
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
M64 = (1 << 64) - 1


def _compiler() -> str:
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")):
        if cand and Path(cand).exists():
            return cand
    pytest.fail("no C++ compiler for the host program")


@pytest.fixture(scope="module")
def second_products(tmp_path_factory) -> np.ndarray:
    tmp = tmp_path_factory.mktemp("murmur_words")
    exe, out = tmp / "murmur_word_tables", tmp / "kj.bin"
    subprocess.run([_compiler(), "-O2", "-std=c++17", f"-I{CSRC}", str(ROOT / "tests" / "murmur_word_tables_main.cpp"), "-o", str(exe)], check=True)
    subprocess.run([str(exe), str(out)], check=True)
    return np.fromfile(out, dtype="<u8").reshape(4, 8, 65536)


def _ascii_group(g: int, nv: int) -> int:
    """The 4-base group g (base i at bits 2i) as little-endian ASCII, its first nv bytes."""
    return int.from_bytes(bytes(b"ACGT"[(g >> (2 * i)) & 3] for i in range(max(0, min(4, nv)))), "little")


def _definition(j: int, word: int) -> int:
    """MurmurHash3_x64_128: k1 = rotl(k1 * c1, 31) * c2 for the even words, k2 = rotl(k2 * c2, 33) * c1 for the odd ones."""
    ca, cb, r = (C2, C1, 33) if j & 1 else (C1, C2, 31)
    p = (word * ca) & M64
    return ((((p << r) | (p >> (64 - r))) & M64) * cb) & M64


@pytest.mark.parametrize("j", range(4))
def test_second_product_of_every_group_pair(second_products, j):
    """Every byte count 1..8 of word j (k = 8j + 1 .. 8j + 8: the lo group partial, the hi group empty, partial, full)
    and every one of the 65 536 group pairs: the value from {A.hi, T, B} equals rotl(word * cA, r) * cB.  The expected
    values are numpy uint64 arithmetic (wrapping), itself held to Python integers on every 61st pair."""
    ca, cb, r = (C2, C1, 33) if j & 1 else (C1, C2, 31)
    for n in range(1, 9):
        lo = np.array([_ascii_group(g, n) for g in range(256)], dtype=np.uint64)
        hi = np.array([_ascii_group(g, n - 4) for g in range(256)], dtype=np.uint64)
        word = (lo[None, :] | (hi[:, None] << np.uint64(32))).reshape(-1)  # index lo + 256 * hi
        with np.errstate(over="ignore"):
            p = word * np.uint64(ca)
            want = ((p << np.uint64(r)) | (p >> np.uint64(64 - r))) * np.uint64(cb)
        for i in range(0, 65536, 61):
            assert int(want[i]) == _definition(j, int(word[i])), (j, n, i)
        got = second_products[j, n - 1]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"word {j}, {n} bytes: {bad.size} of 65536 differ, first at lo={bad[0] & 255} hi={bad[0] >> 8}"
