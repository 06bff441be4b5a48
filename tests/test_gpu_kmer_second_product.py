"""GPU test of the k-mer hash kernel's second-product tables (kmer_hash_kernel<K, kSecondTables>, k = 1 .. 32).

(a) the device sketch equals the oracle's for k-mer sizes that cover an empty hi group, partial groups in either half,
    exact word ends and both ends of the kernel's range; the input is checked to read every table entry at k = 31;
(b) in the tools build the three forms of the kernel (PA_KMER_VARIANT unset, 0, 1) give identical sketches.
"""

from __future__ import annotations

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

KS = [1, 3, 4, 5, 8, 9, 12, 15, 16, 17, 21, 24, 25, 28, 31, 32]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _fasta(name: bytes, seq: bytes) -> bytes:
    return b">" + name + b"\n" + b"\n".join(seq[i : i + 70] for i in range(0, len(seq), 70)) + b"\n"


def _genomes() -> list[bytes]:
    """Three random genomes of 20 kb, 11 kb and 3 kb; the second has runs of N and lower-case stretches.  The seed is
    one of the few for which test_input_reads_every_table_entry_at_k31 holds: a canonical k-mer rarely starts with
    TTTT (its reverse complement then has to start with TTTT too), so that entry of word 0 is read about once in
    130 000 windows."""
    rng = np.random.default_rng(17)
    seqs = [rng.choice(ACGT, size=n) for n in (20_000, 11_000, 3_000)]
    dirty = seqs[1]
    for p in (0, 977, 4_096, 7_777, 10_990):  # also at the genome's two ends
        dirty[p : p + int(rng.integers(1, 40))] = ord("N")
    lower = rng.random(dirty.size) < 0.3
    dirty[lower & (dirty != ord("N"))] += 32
    return [_fasta(b"g%d" % i, s.tobytes()) for i, s in enumerate(seqs)]


TEXTS = _genomes()
_WANT: dict = {}


def _want(k: int, scaled: int) -> list[np.ndarray]:
    if (k, scaled) not in _WANT:
        _WANT[k, scaled] = [oracle.sketch_fasta_text(t, k, scaled)[0] for t in TEXTS]
    return _WANT[k, scaled]


@pytest.fixture(scope="module")
def engine():
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def tools_engine():
    """The -DPA_TOOLS build of the library: PA_KMER_VARIANT exists there only."""
    from pyani_plus_amd.engine import HipEngine

    eng = HipEngine(0, tools=True)
    yield eng
    eng.close()


def _groups_read(k: int) -> set:
    """The (word slot, half, group value) triples that the canonical k-mers of TEXTS look up."""
    seen = set()
    code = np.full(256, 4, dtype=np.uint8)
    for i, b in enumerate(b"ACGT"):
        code[b] = code[b + 32] = i
    for text in TEXTS:
        seq = np.frombuffer(b"".join(text.split(b"\n")[1:]), dtype=np.uint8)
        c = code[seq]
        w = np.lib.stride_tricks.sliding_window_view(c, k)
        w = w[(w < 4).all(axis=1)]
        rc = 3 - w[:, ::-1]
        differ = w != rc
        first = differ.argmax(axis=1)
        rows = np.arange(w.shape[0])
        fwd = ~differ.any(axis=1) | (w[rows, first] < rc[rows, first])  # lexicographic order is code order: A < C < G < T
        canon = np.where(fwd[:, None], w, rc).astype(np.uint32)
        for j in range((k + 7) // 8):
            for half in (0, 1):
                bases = canon[:, 8 * j + 4 * half : min(k, 8 * j + 4 * half + 4)]
                if bases.shape[1] == 0:
                    continue
                value = (bases << (2 * np.arange(bases.shape[1], dtype=np.uint32))).sum(axis=1)
                seen |= {(j, half, int(v)) for v in np.unique(value)}
    return seen


def test_input_reads_every_table_entry_at_k31():
    """The condition on the input of the tests below: at k = 31 every entry of the four lo-group tables and of the four
    hi-group tables is read -- the 7-byte last word's hi group has three bases, 64 values."""
    seen = _groups_read(31)
    want = {(j, half, v) for j in range(4) for half in (0, 1) for v in range(64 if (j, half) == (3, 1) else 256)}
    assert seen == want, f"{len(want - seen)} table entries unread"


@pytest.mark.parametrize("scaled", [1, 1000])
@pytest.mark.parametrize("k", KS)
def test_sketch_equals_oracle(engine, k, scaled):
    from pyani_plus_amd.engine import pack_genomes

    got = engine.sketch(engine.upload(pack_genomes(TEXTS)), k, scaled).to_host()
    for g, want in enumerate(_want(k, scaled)):
        assert np.array_equal(got[g], want), f"genome {g}: {len(got[g])} hashes against the oracle's {len(want)} (k={k}, scaled={scaled})"


@pytest.mark.parametrize("scaled", [1, 50])
def test_variants_agree(tools_engine, monkeypatch, scaled):
    """PA_KMER_VARIANT unset (second-product tables), 0 (arithmetic) and 1 (first-product tables, the form before) at
    k = 31: identical sketches, equal to the oracle's."""
    from pyani_plus_amd.engine import pack_genomes

    dev = tools_engine.upload(pack_genomes(TEXTS))
    for variant in (None, "0", "1"):
        if variant is None:
            monkeypatch.delenv("PA_KMER_VARIANT", raising=False)
        else:
            monkeypatch.setenv("PA_KMER_VARIANT", variant)
        got = tools_engine.sketch(dev, 31, scaled).to_host()
        for g, want in enumerate(_want(31, scaled)):
            assert np.array_equal(got[g], want), f"PA_KMER_VARIANT={variant}: genome {g} differs (scaled={scaled})"
