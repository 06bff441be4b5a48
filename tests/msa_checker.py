"""CPU checker of external-alignment-hip, written from the definitions:
M = columns where q == s and q != '-', B = columns where neither is '-', n_x = non-gap bytes of row x.
Also a restatement of the reference's FASTA parser and a numpy-backed stand-in for HipEngine's MSA calls."""

from __future__ import annotations

import numpy as np

GAP = ord("-")
WHITESPACE = b" \t\r\n"


def fasta_records(data: bytes) -> list[tuple[bytes, bytes]]:
    """(title, sequence) per record with the semantics of pyani_plus.utils.fasta_bytes_iterator."""
    # the reference iterates a binary file: lines end at '\n' only (bytes.splitlines would also split at \r, \v, \f, ...)
    lines = [chunk + b"\n" for chunk in data.split(b"\n")]
    if lines and lines[-1] == b"\n":
        lines.pop()
    else:
        lines[-1] = lines[-1][:-1]
    out, title, seq = [], None, []
    for line in lines:
        if line[:1] == b">":
            if title is not None:
                out.append((title, b"".join(seq).translate(None, WHITESPACE)))
            title, seq = line[1:].rstrip(), []
        elif title is not None:
            seq.append(line.rstrip())
    if title is not None:
        out.append((title, b"".join(seq).translate(None, WHITESPACE)))
    return out


def counts_against(rows: np.ndarray, s: int) -> tuple[np.ndarray, np.ndarray]:
    """(M, B) of every row against row s, vectorised over the rows."""
    m = np.zeros(rows.shape[0], dtype=np.uint32)
    b = np.zeros(rows.shape[0], dtype=np.uint32)
    subject = rows[s].copy()
    ng_s = subject != GAP
    step = max(1, (1 << 26) // max(rows.shape[1], 1))  # rows at a time: bounded temporaries on long alignments
    for r0 in range(0, rows.shape[0], step):
        block = rows[r0 : r0 + step]
        ng = block != GAP
        b[r0 : r0 + step] = (ng & ng_s).sum(axis=1)
        m[r0 : r0 + step] = ((block == subject) & ng).sum(axis=1)
    return m, b


def counts_matrix(rows: np.ndarray, q_range=None, s_range=None) -> tuple[np.ndarray, np.ndarray]:
    q0, q1 = q_range or (0, rows.shape[0])
    s0, s1 = s_range or (0, rows.shape[0])
    m = np.zeros((q1 - q0, s1 - s0), dtype=np.uint32)
    b = np.zeros_like(m)
    for j, s in enumerate(range(s0, s1)):
        mm, bb = counts_against(rows, s)
        m[:, j], b[:, j] = mm[q0:q1], bb[q0:q1]
    return m, b


def reference_rows(rows: np.ndarray, hashes: list[str], subject: str, queries: set[str]) -> list[tuple]:
    """One subject column as the reference's worker yields it, from the checker's counts (Python int arithmetic)."""
    s = hashes.index(subject)
    n = (rows != GAP).sum(axis=1)
    m, b = counts_against(rows, s)
    out = []
    for q, h in enumerate(hashes):
        if h < subject or h not in queries:
            continue
        if h == subject:
            out.append((h, subject, 1.0, int(n[q]), 0, 1.0, 1.0))
            continue
        mq, bq, nq, ns = int(m[q]), int(b[q]), int(n[q]), int(n[s])
        aln = nq + ns - bq
        out.append((h, subject, mq / aln, aln, aln - mq, bq / nq, bq / ns))
        out.append((subject, h, mq / aln, aln, aln - mq, bq / ns, bq / nq))
    return out


class _Host:
    def __init__(self, a):
        self.a = np.asarray(a)

    def cpu(self):
        return self

    def numpy(self):
        return self.a.view(np.int32)


class NumpyMsaEngine:
    """The MSA calls of HipEngine on the CPU (the checker's counts): lets the method module run without a GPU."""

    def msa_upload(self, msa):
        return msa

    def msa_pair_counts(self, msa, q_range=None, s_range=None, *, symmetric=False):
        rows = msa.rows[:, : msa.n_cols] if msa.n_cols else msa.rows[:, :0]
        m, b = counts_matrix(rows, q_range, s_range)
        return _Host(m), _Host(b)


def golden_msa_bytes(spec: dict) -> bytes:
    """The FASTA text of a seeded golden alignment (tests/golden/external_alignment/columns.json keeps its settings)."""
    from pyani_plus_amd.synth import msa_fasta_bytes, synth_msa_rows

    rows = synth_msa_rows(spec["rows"], spec["columns"], seed=spec["seed"], **spec["opts"])
    return msa_fasta_bytes([f"{spec['prefix']}{i:02d}" for i in range(spec["rows"])], rows, seed=spec["seed"])


def golden_columns(path) -> dict:
    """name -> (FASTA text, hashes, {subject: [row tuples with hashes]}) of the seeded goldens; the text's md5 is
    checked against the recorded one (the generator must still make the alignment the reference saw)."""
    import hashlib
    import json
    from pathlib import Path

    out = {}
    for name, g in json.loads(Path(path).read_text())["msas"].items():
        text = golden_msa_bytes(g["spec"])
        assert hashlib.md5(text).hexdigest() == g["md5"], f"{name}: the generator no longer makes the recorded alignment"
        hashes = g["hashes"]
        cols = {s: [(hashes[r[0]], hashes[r[1]], *r[2:]) for r in col] for s, col in zip(hashes, g["columns"])}
        out[name] = (text, hashes, cols)
    return out
