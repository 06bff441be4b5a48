"""external-alignment-hip on the MI355X: the pack and pair-count kernels against the CPU checker, the column worker
against the reference's recorded columns, the run driver (labels, resume, export-run), and full-size shapes."""

from __future__ import annotations

import json
import logging
import shutil
import sqlite3
from pathlib import Path

import numpy as np
import pytest

from pyani_plus_amd import rundb
from pyani_plus_amd.engine import DeviceMSA, HipEngine, LoadedMSA, msa_code_table
from pyani_plus_amd.methods import external_alignment_hip as ea
from pyani_plus_amd.synth import msa_fasta_bytes, synth_msa_rows
from tests.msa_checker import counts_against, counts_matrix, golden_columns

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "external_alignment"
VIRAL = ROOT / "tests" / "golden" / "viral_example"
LOGGER = logging.getLogger("test")
KEYS = ["query_hash", "subject_hash", "identity", "aln_length", "sim_errors", "cov_query", "cov_subject"]


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def _loaded(rows: np.ndarray) -> LoadedMSA:
    n, length = rows.shape
    stride = max(32, (length + 31) // 32 * 32)
    padded = np.full((n, stride), ord("-"), dtype=np.uint8)
    padded[:, :length] = rows
    hist = np.bincount(rows.ravel(), minlength=256).astype(np.uint64)
    return LoadedMSA("", [f"r{i}".encode() for i in range(n)], np.full(n, length, np.uint64), hist, padded, length)


def _alphabet_rows(rng, n, length, n_residues):
    letters = np.array([c for c in range(256) if c != ord("-")], dtype=np.uint8)[:n_residues]
    rows = letters[rng.integers(0, n_residues, (n, length))]
    rows[rng.random((n, length)) < 0.15] = ord("-")
    return rows


def _numpy_planes(rows, code, bits):
    n, length = rows.shape
    words = (length + 31) // 32
    codes = np.zeros((n, words * 32), dtype=np.uint32)
    codes[:, :length] = code[rows]
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    planes = []
    for p in range(bits):
        bitsets = ((codes >> p) & 1).reshape(n, words, 32).astype(np.uint64)
        planes.append((bitsets * weights).sum(axis=2).astype(np.uint32))
    ng = (codes != 0).reshape(n, words, 32).astype(np.uint64)
    planes.append((ng * weights).sum(axis=2).astype(np.uint32))
    return planes, (codes != 0).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("n_residues,bits", [(1, 1), (3, 2), (5, 3), (20, 5), (200, 8)])
def test_pack_planes_against_numpy(engine, n_residues, bits):
    rng = np.random.default_rng(bits)
    for length in (1, 31, 32, 33, 1000, 65537):
        for n in (1, 2, 3, 65, 130):
            rows = _alphabet_rows(rng, n, length, n_residues)
            room = n * length >= n_residues
            if room:  # every letter once, whatever was drawn
                rows.reshape(-1)[:n_residues] = [c for c in range(256) if c != ord("-")][:n_residues]
            msa = _loaded(rows)
            code, b = msa_code_table(msa.histogram)
            assert b == bits if room else b <= bits, (length, n)  # without room for the alphabet: packed with the bits it has
            dm = engine.msa_upload(msa, chunk_bytes=max(msa.rows.shape[1], 40 * msa.rows.shape[1]))
            planes = dm.planes.cpu().numpy().view(np.uint32)
            n_pad = (n + 63) // 64 * 64
            words = (length + 31) // 32
            planes = planes[: words * (b + 1) * n_pad].reshape(words, b + 1, n_pad)[:, :, :n]
            want, nongap = _numpy_planes(rows, code, b)
            for p in range(b + 1):
                assert np.array_equal(planes[:, p, :].T, want[p]), (length, n, p)
            assert np.array_equal(dm.nongap.cpu().numpy().view(np.uint32)[:n], nongap), (length, n)


def _check_counts(engine, rows, *, rect=None):
    msa = _loaded(rows)
    dm = engine.msa_upload(msa)
    n = rows.shape[0]
    m, b = engine.msa_pair_counts(dm, symmetric=True)
    wm, wb = counts_matrix(rows)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), wm)
    assert np.array_equal(b.cpu().numpy().view(np.uint32), wb)
    for q_range, s_range in rect or [((0, n), (n // 3, n // 3 + 1)), ((1, n), (0, n - 1)), ((n // 2, n), (0, (n + 1) // 2))]:
        m, b = engine.msa_pair_counts(dm, q_range, s_range)
        wm, wb = counts_matrix(rows, q_range, s_range)
        assert np.array_equal(m.cpu().numpy().view(np.uint32), wm), (q_range, s_range)
        assert np.array_equal(b.cpu().numpy().view(np.uint32), wb), (q_range, s_range)


def test_pair_counts_symmetric_and_rectangular(engine):
    rng = np.random.default_rng(7)
    for n, length, n_res in ((1, 10, 4), (2, 33, 4), (70, 1000, 5), (130, 4097, 20), (200, 300, 200)):
        rows = _alphabet_rows(rng, n, length, n_res)
        _check_counts(engine, rows)


def test_pair_counts_split_columns(engine):
    # 40 rows: one tile, so the columns are split across blocks and the partial counts added
    rows = synth_msa_rows(40, 1_000_000, seed=4, divergence=0.02, gap_runs=1e-4, n_runs=1e-4)
    _check_counts(engine, rows, rect=[((0, 40), (5, 6)), ((3, 40), (0, 17))])


# ------------------------------------------------------------------ the column worker against the reference's columns
def _run(tmp_path, name, text):
    aln = tmp_path / f"{name}.fasta"
    aln.write_bytes(text)
    import hashlib
    from types import SimpleNamespace

    tool = ea.get_external_alignment_hip()
    conf = SimpleNamespace(method=ea.METHOD, program=tool.exe_path.stem, version=tool.version, fragsize=None, mode=None, kmersize=None,
                           minmatch=None, extra=ea.make_extra(hashlib.md5(text).hexdigest(), "md5", aln))
    run = SimpleNamespace(run_id=1, configuration=conf, status="Running", fasta_hashes=[])
    session = SimpleNamespace(bind=SimpleNamespace(url=f"sqlite:///{tmp_path / 'x.db'}"), commit=lambda: None)
    return run, session


@pytest.fixture(scope="module")
def seeded():
    return golden_columns(GOLDEN / "columns.json")


@pytest.mark.parametrize("name", ["seeded_dna", "seeded_iupac", "seeded_divergent"])
def test_golden_columns_on_the_device(engine, tmp_path, seeded, name):
    text, hashes, columns = seeded[name]
    run, session = _run(tmp_path, name, text)
    out = tmp_path / "col.json"
    for subject in hashes:
        assert ea.compute_external_alignment_hip(LOGGER, tmp_path, session, run, out, tmp_path, {}, {}, {h: 0 for h in hashes}, subject,
                                                 engine=engine) == 0
        assert json.loads(out.read_text())["comparisons"] == [dict(zip(KEYS, r)) for r in columns[subject]], subject
    assert ea.compute_external_alignment_hip(LOGGER, tmp_path, session, run, out, tmp_path, {}, {}, {h: 0 for h in hashes}, "", engine=engine) == 0
    assert json.loads(out.read_text())["comparisons"] == [dict(zip(KEYS, r)) for s in hashes for r in columns[s]]


# ------------------------------------------------------------------ the run driver
MOCK_ROWS = [b"GACC-GGTTTT", b"AACC-GG-TTT", b"AACC-GGATTT"]
MOCK_HASHES = ["5584c7029328dc48d33f95f0a78f7e57", "689d3fd6881db36b5e08329cf23cecdd", "78975d5144a1cd12e98898d573cf6536"]
MOCK_FILES = ["OP073605.fasta", "MGV-GENOME-0264574.fas", "MGV-GENOME-0266457.fna"]


def _mock_for(label: str) -> bytes:
    names = {"stem": [f.rsplit(".", 1)[0] for f in MOCK_FILES], "filename": MOCK_FILES, "md5": MOCK_HASHES}[label]
    return b"".join(b">" + n.encode() + b" mock\n" + r + b"\n" for n, r in zip(names, MOCK_ROWS))


def _genomes(tmp_path) -> Path:
    fasta = tmp_path / "genomes"
    fasta.mkdir()
    for f in MOCK_FILES:
        shutil.copy(VIRAL / f, fasta / f)
    return fasta


@pytest.mark.parametrize("label", ["stem", "filename", "md5"])
def test_mock_run_with_each_label(engine, tmp_path, label):
    golden = json.loads((GOLDEN / "columns.json").read_text())["mock"]
    fasta = _genomes(tmp_path)
    aln = tmp_path / "mock.fasta"
    aln.write_bytes(_mock_for(label) if label != "stem" else (GOLDEN / golden["file"]).read_bytes())
    db = tmp_path / "mock.db"
    run = rundb.run_external_alignment_hip(fasta, db, alignment=aln, label=label, temp=tmp_path / "tmp", logger=LOGGER, engine=engine)
    assert run.status == "Done"
    conn = sqlite3.connect(db)
    df_identity, df_cov_query = conn.execute("SELECT df_identity, df_cov_query FROM runs WHERE run_id=?", (run.run_id,)).fetchone()
    assert df_identity == golden["df_identity"]
    assert df_cov_query == golden["df_cov_query"]
    assert conn.execute("SELECT extra FROM configurations").fetchone()[0].endswith(f";label={label};alignment=mock.fasta")
    written = rundb.export_run(db, tmp_path / "export", logger=LOGGER)
    names = sorted(Path(p).name for p in written)
    assert any("aln_length" in p for p in names) and any("sim_errors" in p for p in names) and any("hadamard" in p for p in names)


def test_resume_partial_run(engine, tmp_path):
    fasta = _genomes(tmp_path)
    aln = tmp_path / "mock.fasta"
    aln.write_bytes(_mock_for("stem"))
    db = tmp_path / "mock.db"
    run = rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp_path / "tmp", logger=LOGGER, engine=engine)
    conn = sqlite3.connect(db)
    full = conn.execute("SELECT query_hash, subject_hash, identity, aln_length, sim_errors, cov_query FROM comparisons ORDER BY 1, 2").fetchall()
    want = conn.execute("SELECT df_identity, df_cov_query, df_aln_length, df_sim_errors FROM runs").fetchone()
    # the rows of the second and third columns' workers, as an interrupted run leaves them out
    b = MOCK_HASHES[1]
    conn.execute("DELETE FROM comparisons WHERE subject_hash>=? AND query_hash>=?", (b, b))
    conn.execute("UPDATE runs SET status='Worker interrupted', df_identity=NULL")
    conn.commit()
    conn.close()
    resumed = rundb.resume(db, temp=tmp_path / "tmp2", logger=LOGGER, engine=engine)
    assert resumed.status == "Done"
    conn = sqlite3.connect(db)
    again = conn.execute("SELECT query_hash, subject_hash, identity, aln_length, sim_errors, cov_query FROM comparisons ORDER BY 1, 2").fetchall()
    assert again == full and len(full) == 9
    assert conn.execute("SELECT df_identity, df_cov_query, df_aln_length, df_sim_errors FROM runs").fetchone() == want
    with pytest.raises(SystemExit):
        rundb.run_external_alignment_hip(fasta, db, alignment=aln, temp=tmp_path / "tmp3", logger=LOGGER, engine=engine, gpus=2)


# ------------------------------------------------------------------ full size
def test_scale_10000_rows_sars_cov_2_length(engine):
    rows = synth_msa_rows(10_000, 29_903, seed=21, divergence=0.01, gap_runs=2e-5, n_runs=5e-5)
    msa = _loaded(rows)
    assert msa_code_table(msa.histogram)[1] == 3
    dm = engine.msa_upload(msa)
    m, b = engine.msa_pair_counts(dm, symmetric=True)
    m, b = m.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    n = (rows != ord("-")).sum(axis=1)
    assert np.array_equal(np.diagonal(m), n) and np.array_equal(np.diagonal(b), n)
    assert np.array_equal(m, m.T) and np.array_equal(b, b.T)
    rng = np.random.default_rng(0)
    for s in rng.choice(10_000, 200, replace=False):
        wm, wb = counts_against(rows, int(s))
        assert np.array_equal(m[:, s], wm) and np.array_equal(b[:, s], wb), s
    rect_m, rect_b = engine.msa_pair_counts(dm, (0, 10_000), (4321, 4322))
    assert np.array_equal(rect_m.cpu().numpy().view(np.uint32)[:, 0], m[:, 4321])
    assert np.array_equal(rect_b.cpu().numpy().view(np.uint32)[:, 0], b[:, 4321])


def test_scale_1000_rows_core_genome_length(engine):
    rows = synth_msa_rows(1_000, 2_000_000, seed=22, divergence=0.01, gap_runs=1e-5, n_runs=1e-5)
    dm = engine.msa_upload(_loaded(rows))
    m, b = engine.msa_pair_counts(dm, symmetric=True)
    m, b = m.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)
    for s in (0, 517, 999):
        wm, wb = counts_against(rows, s)
        assert np.array_equal(m[:, s], wm) and np.array_equal(b[:, s], wb), s
