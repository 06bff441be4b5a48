"""Host driver of the MI355X sketch -> pair-count -> ANI pipeline.

Everything numeric happens inside ``libpyani_hip.so`` (``include/pyani_hip.h``);
this module only owns buffers.  PyTorch is used for device memory, the HIP
stream and (in ``distributed.py``) RCCL -- never for arithmetic on the path.

Reference steps replaced:
  A2  ``sourmash scripts singlesketch``  (pyani_plus/methods/sourmash.py:67-83)
  A5  ``sourmash scripts manysearch``    (pyani_plus/methods/sourmash.py:184-200)
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import _capi
from ._capi import HipBackendError, check


def max_hash_for_scaled(scaled: int) -> int:
    """sourmash's ``max_hash`` for a ``scaled`` value (double-rounded 2**64/scaled)."""
    return int(_capi.load_library().pa_max_hash(int(scaled)))


# --------------------------------------------------------------------------- host arena
@dataclass
class HostArena:
    """2-bit packed genomes + invalid-position mask (layout: DESIGN.md, "Data layout")."""

    packed: np.ndarray  # uint32, 16 bases / word
    mask: np.ndarray  # uint32, 32 positions / word, bit=1 -> not a usable base
    genome_start: np.ndarray  # uint64 [n+1], multiples of 64
    residues: list[int] = field(default_factory=list)  # Genome.length per genome
    records: list[int] = field(default_factory=list)
    invalid: list[int] = field(default_factory=list)
    # FASTA records (contigs) in arena order: first arena position, residues, owning genome
    contig_start: np.ndarray | None = None
    contig_len: np.ndarray | None = None
    contig_genome: np.ndarray | None = None
    pinned_packed: "object" = None  # torch tensor owning ``packed`` when the loader wrote it into page-locked memory
    # residues that are neither ACGT nor N (IUPAC codes, ...): ascending arena positions and upper-cased bytes.  The mask
    # bit stands for N; the fragment-ANI path hashes these as the characters they are, as fastANI does
    ambig_pos: np.ndarray | None = None  # uint64
    ambig_byte: np.ndarray | None = None  # uint8

    @property
    def n_genomes(self) -> int:
        return len(self.genome_start) - 1

    @property
    def arena_bases(self) -> int:
        return int(self.genome_start[-1])


def _text_ambiguous(lib, text: bytes, fasta: bool, at_most: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(positions relative to the genome's first, upper-cased bytes) of the residues that are neither ACGT nor N.

    ``at_most``: a bound on their number the caller already has (the packer's count of invalid residues, N included):
    the list then comes out of ONE pass over the text instead of a counting pass and a filling pass."""
    if not len(text) or at_most == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    if at_most is None:
        at_most = int(lib.pa_text_ambiguous(text, len(text), int(fasta), None, None, 0))
        if at_most < 0:
            raise HipBackendError(f"pa_text_ambiguous failed: {_capi.last_error()}")
        if at_most == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    pos, byte = np.zeros(at_most, dtype=np.uint64), np.zeros(at_most, dtype=np.uint8)
    n = int(lib.pa_text_ambiguous(text, len(text), int(fasta), pos.ctypes.data, byte.ctypes.data, at_most))
    if n < 0 or n > at_most:
        raise HipBackendError(f"pa_text_ambiguous failed: {_capi.last_error() if n < 0 else f'{n} residues against a bound of {at_most}'}")
    return pos[:n].copy(), byte[:n].copy()


def pack_genomes(texts: list[bytes], *, fasta: bool = True) -> HostArena:
    """Pack decompressed FASTA texts (or bare residue strings) into one arena (host only)."""
    lib = _capi.load_library()
    bounds = [int(lib.pa_pack_bound(len(t))) for t in texts]
    total = sum(bounds)
    packed = np.zeros(total // 16, dtype=np.uint32)
    mask = np.zeros(total // 32, dtype=np.uint32)
    starts = np.zeros(len(texts) + 1, dtype=np.uint64)
    residues, records, invalid = [], [], []
    c_start, c_len, c_genome = [], [], []
    a_pos, a_byte = [], []
    pos = 0
    for g, text in enumerate(texts):
        nb, nr, nrec, ninv = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        buf = bytes(text) if len(text) else None
        p_ptr = packed.ctypes.data + (pos // 16) * 4
        m_ptr = mask.ctypes.data + (pos // 32) * 4
        if fasta:
            st = lib.pa_pack_fasta(buf, len(text), p_ptr, m_ptr, bounds[g], C.byref(nb), C.byref(nr), C.byref(nrec), C.byref(ninv))
        else:
            st = lib.pa_pack_seq(buf, len(text), p_ptr, m_ptr, bounds[g], C.byref(nb), C.byref(ninv))
            nr.value, nrec.value = len(text), 1
        check(st, "pa_pack_fasta" if fasta else "pa_pack_seq")
        if fasta and nrec.value:
            rs = np.zeros(int(nrec.value), dtype=np.uint64)
            rl = np.zeros(int(nrec.value), dtype=np.uint64)
            lib.pa_fasta_records(buf, len(text), rs.ctypes.data, rl.ctypes.data, int(nrec.value))
            c_start.extend((rs + np.uint64(pos)).tolist())
            c_len.extend(rl.tolist())
            c_genome.extend([g] * int(nrec.value))
        elif not fasta:
            c_start.append(pos)
            c_len.append(len(text))
            c_genome.append(g)
        if ninv.value:
            ap, ab = _text_ambiguous(lib, buf, fasta, at_most=int(ninv.value))  # (ninv counts the N too: a bound, one pass)
            a_pos.append(ap + np.uint64(pos))
            a_byte.append(ab)
        starts[g] = pos
        pos += int(nb.value)
        residues.append(int(nr.value))
        records.append(int(nrec.value))
        invalid.append(int(ninv.value))
    starts[len(texts)] = pos
    return HostArena(
        packed[: pos // 16].copy(), mask[: pos // 32].copy(), starts, residues, records, invalid,
        np.array(c_start, dtype=np.uint64), np.array(c_len, dtype=np.uint32), np.array(c_genome, dtype=np.uint32),
        ambig_pos=np.concatenate(a_pos) if a_pos else np.zeros(0, np.uint64), ambig_byte=np.concatenate(a_byte) if a_byte else np.zeros(0, np.uint8),
    )


@dataclass
class LoadedFasta:
    """Per-file result of the threaded host front-end (``pa_fasta_batch_load``)."""

    path: str
    status: int
    message: str
    md5: str
    length: int  # sum of residues = Genome.length
    records: int
    invalid: int
    description: str
    gzip: bool


def load_fasta_files(paths, threads: int = 0, *, pinned: bool = False) -> tuple[list[LoadedFasta], HostArena]:
    """Read, gunzip, md5, parse and pack FASTA files on host threads.

    Returns per-file metadata (failed files carry ``status != 0`` and the reference's error
    text in ``message``) and the arena of the files that loaded, in order.  ``pinned``: the packed bases are
    written into page-locked memory (a torch tensor kept in ``arena.pinned_packed``), ready for
    ``HipEngine.sketch_streamed`` without a staging copy."""
    import os

    lib = _capi.load_library()
    paths = [str(p) for p in paths]
    n = len(paths)
    if threads <= 0:
        threads = int(lib.pa_host_cpu_budget())  # CPUs of the affinity mask, capped by the cgroup quota
    arr = (C.c_char_p * max(n, 1))(*[p.encode() for p in paths])
    batch = C.c_void_p()
    check(lib.pa_fasta_batch_load(arr, n, threads, C.byref(batch)), "pa_fasta_batch_load")
    try:
        infos: list[LoadedFasta] = []
        ok_residues, ok_records, ok_invalid = [], [], []
        rec_tables = []
        for i, path in enumerate(paths):
            md5 = C.create_string_buffer(33)
            nres, nrec, ninv, nb, nt = (C.c_uint64(0) for _ in range(5))
            desc, msg = C.c_char_p(), C.c_char_p()
            gz = C.c_int(0)
            st = lib.pa_fasta_batch_info(batch, i, md5, C.byref(nres), C.byref(nrec), C.byref(ninv), C.byref(nb), C.byref(nt), C.byref(desc), C.byref(msg), C.byref(gz))
            infos.append(
                LoadedFasta(path, st, (msg.value or b"").decode(errors="replace"), md5.value.decode(), int(nres.value), int(nrec.value),
                            int(ninv.value), (desc.value or b"").decode(errors="replace"), bool(gz.value))
            )  # fmt: skip
            if st == 0:
                ok_residues.append(int(nres.value))
                ok_records.append(int(nrec.value))
                ok_invalid.append(int(ninv.value))
                rs_p, rl_p, rn = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.c_uint64(0)
                lib.pa_fasta_batch_records(batch, i, C.byref(rs_p), C.byref(rl_p), C.byref(rn))
                k_rec = int(rn.value)
                rec_tables.append((np.ctypeslib.as_array(rs_p, (k_rec,)).copy(), np.ctypeslib.as_array(rl_p, (k_rec,)).copy()) if k_rec else (np.zeros(0, np.uint64), np.zeros(0, np.uint64)))
        total = int(lib.pa_fasta_batch_arena_bases(batch))
        pinned_packed = None
        if pinned:
            import torch

            pinned_packed = torch.empty(max(total // 16, 1), dtype=torch.int32, pin_memory=torch.cuda.is_available())
            packed = pinned_packed.numpy().view(np.uint32)
        else:
            packed = np.empty(max(total // 16, 1), dtype=np.uint32)
        mask = np.empty(max(total // 32, 1), dtype=np.uint32)
        starts_all = np.zeros(n + 1, dtype=np.uint64)
        check(lib.pa_fasta_batch_copy_arena(batch, packed.ctypes.data, mask.ctypes.data, starts_all.ctypes.data), "pa_fasta_batch_copy_arena")
        keep = [i for i, info in enumerate(infos) if info.status == 0]
        starts = np.array([starts_all[i] for i in keep] + [total], dtype=np.uint64)
        c_start = np.concatenate([rs + starts[g] for g, (rs, _rl) in enumerate(rec_tables)]) if rec_tables else np.zeros(0, np.uint64)
        c_len = np.concatenate([rl for _rs, rl in rec_tables]).astype(np.uint32) if rec_tables else np.zeros(0, np.uint32)
        c_genome = np.concatenate([np.full(len(rs), g, dtype=np.uint32) for g, (rs, _rl) in enumerate(rec_tables)]) if rec_tables else np.zeros(0, np.uint32)
        n_amb = int(lib.pa_fasta_batch_ambiguous(batch, None, None, 0))
        a_pos, a_byte = np.zeros(max(n_amb, 0), dtype=np.uint64), np.zeros(max(n_amb, 0), dtype=np.uint8)
        if n_amb > 0:
            lib.pa_fasta_batch_ambiguous(batch, a_pos.ctypes.data, a_byte.ctypes.data, n_amb)
        return infos, HostArena(
            packed[: total // 16], mask[: total // 32], starts, ok_residues, ok_records, ok_invalid,
            c_start.astype(np.uint64), c_len, c_genome, pinned_packed[: max(total // 16, 1)] if pinned_packed is not None else None,
            ambig_pos=a_pos, ambig_byte=a_byte,
        )
    finally:
        lib.pa_fasta_batch_free(batch)


# --------------------------------------------------------------------------- device objects
@dataclass
class DeviceArena:
    packed: "object"  # torch.int32 tensor
    mask: "object"
    genome_start: np.ndarray  # host uint64 [n+1]
    dirty: "object" = None  # torch.int64 tensor: one bit per 64-position block that needs its mask words (built on first use)
    # the host arena's list of residues that are neither ACGT nor N (``HostArena.ambig_pos`` / ``ambig_byte``), handed to the
    # library before a fragment-ANI call on this arena
    ambig_pos: np.ndarray | None = None
    ambig_byte: np.ndarray | None = None

    @property
    def n_genomes(self) -> int:
        return len(self.genome_start) - 1

    @property
    def arena_bases(self) -> int:
        return int(self.genome_start[-1])


@dataclass
class PinnedArena:
    """A host arena ready for ``HipEngine.sketch_streamed``: packed bases in page-locked memory and the
    invalid-position mask as runs (start, length) instead of a bitmap."""

    packed: "object"  # pinned torch.int32 tensor
    run_start: np.ndarray  # uint64
    run_len: np.ndarray  # uint64
    genome_start: np.ndarray  # host uint64 [n+1]

    @property
    def n_genomes(self) -> int:
        return len(self.genome_start) - 1

    @property
    def arena_bases(self) -> int:
        return int(self.genome_start[-1])


def mask_runs(mask: np.ndarray, arena_bases: int) -> tuple[np.ndarray, np.ndarray]:
    """Runs of invalid positions of a mask bitmap (host helper ``pa_mask_runs``)."""
    lib = _capi.load_library()
    mask = np.ascontiguousarray(mask, dtype=np.uint32)
    n = int(lib.pa_mask_runs(mask.ctypes.data, arena_bases, None, None, 0))
    if n < 0:
        raise HipBackendError("pa_mask_runs: null mask")
    start = np.empty(max(n, 1), dtype=np.uint64)
    length = np.empty(max(n, 1), dtype=np.uint64)
    got = int(lib.pa_mask_runs(mask.ctypes.data, arena_bases, start.ctypes.data, length.ctypes.data, n))
    if got != n:
        raise HipBackendError("pa_mask_runs: run count changed between calls")
    return start[:n], length[:n]


@dataclass
class DeviceSketches:
    """CSR of ascending duplicate-free u64 hashes, resident in HBM."""

    hashes: "object"  # torch.int64 tensor (bit pattern of uint64), length >= total
    off: "object"  # torch.int64 tensor [n+1]
    n: int
    total: int
    host_off: np.ndarray | None = None  # uint64 [n+1] copy of `off` when the host has it (pair phase needs no round trip then)

    def offsets_host(self) -> np.ndarray:
        if self.host_off is None:
            self.host_off = np.ascontiguousarray(self.off.cpu().numpy().astype(np.uint64))
        return self.host_off

    def sizes(self) -> np.ndarray:
        off = self.offsets_host()
        return (off[1:] - off[:-1]).astype(np.uint64)

    def to_host(self) -> list[np.ndarray]:
        off = self.offsets_host().astype(np.int64)
        flat = self.hashes[: self.total].cpu().numpy().view(np.uint64)
        return [flat[int(off[g]) : int(off[g + 1])].copy() for g in range(self.n)]


def _pair_ranges(n: int, q_range, s_range, *, tetra: bool = False) -> tuple[int, int, int, int]:
    """``(q0, q1, s0, s1)`` of an all-pairs call: the query and the subject range, each all ``n`` unless given.
    ``tetra``: checked against the ``n`` genomes of a TETRA-hip call, before the output is allocated."""
    q0, q1 = q_range or (0, n)
    s0, s1 = s_range or (0, n)
    if tetra and not (0 <= q0 <= q1 <= n and 0 <= s0 <= s1 <= n):
        raise ValueError(f"ranges [{q0}, {q1}) x [{s0}, {s1}) outside the {n} genomes")
    return q0, q1, s0, s1


class HipEngine:
    """One HIP context on one GPU.  Raises ``HipBackendError`` when no MI355X is usable."""

    def __init__(self, device: int = 0, *, tools: bool = False):
        """``tools``: bind the -DPA_TOOLS build of the library (``_capi.TOOLS_LIB_PATH``), in which the environment
        switches of tools/ and of the rare-path tests exist; the product library ignores them."""
        self.lib = _capi.load_library(tools)
        self._check = lambda status, what: check(status, what, self.lib)
        try:
            import torch
        except ImportError as err:  # pragma: no cover
            raise HipBackendError("PyTorch (ROCm build) is required for device memory") from err
        if not torch.cuda.is_available():
            raise HipBackendError("no HIP device visible to PyTorch; the HIP path has no CPU fallback")
        self.torch = torch
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        self._check(self.lib.pa_ctx_create(device, C.byref(ctx)), "pa_ctx_create")
        self.ctx = ctx
        self.use_torch_stream()

    # -- plumbing
    def use_torch_stream(self) -> None:
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        self._check(self.lib.pa_ctx_set_stream(self.ctx, C.c_void_p(stream)), "pa_ctx_set_stream")

    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.pa_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus, mem = C.c_int(0), C.c_uint64(0)
        self._check(self.lib.pa_ctx_device_info(self.ctx, name, C.byref(cus), C.byref(mem)), "pa_ctx_device_info")
        return {"name": name.value.decode(), "compute_units": cus.value, "global_mem": mem.value}

    def sync(self) -> None:
        self._check(self.lib.pa_ctx_sync(self.ctx), "pa_ctx_sync")

    # -- data movement
    def upload(self, arena: HostArena) -> DeviceArena:
        t = self.torch
        packed = t.from_numpy(arena.packed.view(np.int32)).to(self.device)
        mask = t.from_numpy(arena.mask.view(np.int32)).to(self.device)
        return DeviceArena(packed, mask, arena.genome_start.copy(), ambig_pos=arena.ambig_pos, ambig_byte=arena.ambig_byte)

    def _set_ambiguous(self, arena: DeviceArena) -> None:
        """Hand the arena's residues that are neither ACGT nor N to the fragment-ANI kernels (``pa_fragani_set_ambiguous``:
        a list the context holds already changes nothing there, a reusable index included)."""
        pos = getattr(arena, "ambig_pos", None)
        n = 0 if pos is None else len(pos)
        if n:
            p = np.ascontiguousarray(pos, dtype=np.uint64)
            b = np.ascontiguousarray(arena.ambig_byte, dtype=np.uint8)
            self._check(self.lib.pa_fragani_set_ambiguous(self.ctx, arena.packed.data_ptr(), p.ctypes.data, b.ctypes.data, n), "pa_fragani_set_ambiguous")
        else:
            self._check(self.lib.pa_fragani_set_ambiguous(self.ctx, None, None, None, 0), "pa_fragani_set_ambiguous")

    def sketches_from_host(self, sketches: list[np.ndarray]) -> DeviceSketches:
        t = self.torch
        off = np.zeros(len(sketches) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in sketches], out=off[1:])
        flat = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]) if sketches else np.empty(0, np.uint64)
        if flat.size == 0:
            flat = np.zeros(1, dtype=np.uint64)
        return DeviceSketches(
            t.from_numpy(flat.view(np.int64).copy()).to(self.device), t.from_numpy(off).to(self.device), len(sketches), int(off[-1]),
            np.ascontiguousarray(off.astype(np.uint64)),
        )

    def sketches_from_gathered(self, hashes, off, off_host: np.ndarray) -> DeviceSketches:
        """The CSR an all-gather delivered (``distributed.allgather_sketches``: tensors on this device, or on the host
        when the collective ran there) as ``DeviceSketches``."""
        hashes, off = hashes.to(self.device), off.to(self.device)
        return DeviceSketches(hashes, off, len(off_host) - 1, int(off_host[-1]), np.ascontiguousarray(off_host, dtype=np.uint64))

    def arena_dirty(self, arena: DeviceArena):
        """The arena's dirty-block bitmap (``pa_arena_dirty``), built on first use and kept with the arena."""
        if arena.dirty is None:
            t = self.torch
            words = (arena.arena_bases // 64 + 63) // 64
            dirty = t.empty(max(words, 1), dtype=t.int64, device=self.device)
            self._check(self.lib.pa_arena_dirty(self.ctx, arena.mask.data_ptr(), arena.arena_bases, dirty.data_ptr()), "pa_arena_dirty")
            arena.dirty = dirty
        return arena.dirty

    # -- the three device steps
    def sketch(self, arena: DeviceArena, k: int, scaled: int, *, max_hash: int | None = None) -> DeviceSketches:
        t = self.torch
        mh = int(max_hash) if max_hash is not None else max_hash_for_scaled(scaled)
        n = arena.n_genomes
        frac = 1.0 if mh >= 2**64 - 1 else (mh + 1) / 2.0**64
        cap = int(arena.arena_bases * frac * 1.25) + 4096
        off = t.empty(n + 1, dtype=t.int64, device=self.device)
        gs = np.ascontiguousarray(arena.genome_start, dtype=np.uint64)
        total = C.c_uint64(0)
        dirty = self.arena_dirty(arena)
        for _attempt in range(2):
            hashes = t.empty(max(cap, 1), dtype=t.int64, device=self.device)
            st = self.lib.pa_sketch(
                self.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), dirty.data_ptr(), arena.arena_bases,
                gs.ctypes.data_as(C.POINTER(C.c_uint64)), n, k, mh, hashes.data_ptr(), cap, off.data_ptr(), C.byref(total),
            )  # fmt: skip
            if st == _capi.PA_E_CAPACITY:
                cap = int(total.value)
                continue
            self._check(st, "pa_sketch")
            return DeviceSketches(hashes, off, n, int(total.value))
        raise HipBackendError("pa_sketch: capacity retry failed")

    def pin_arena(self, arena: HostArena) -> PinnedArena:
        """Page-lock the packed bases and reduce the mask to runs (done once, outside any timed region)."""
        t = self.torch
        if arena.pinned_packed is not None:
            packed = arena.pinned_packed  # the loader wrote straight into page-locked memory
        else:
            packed = t.from_numpy(np.ascontiguousarray(arena.packed).view(np.int32)).pin_memory()
        start, length = mask_runs(arena.mask, int(arena.genome_start[-1]))
        return PinnedArena(packed, start, length, np.ascontiguousarray(arena.genome_start, dtype=np.uint64).copy())

    def sketch_streamed(self, host: PinnedArena, k: int, scaled: int, *, max_hash: int | None = None, arena: DeviceArena | None = None):
        """Host arena -> (device arena, sketches); the upload runs behind the hash kernel (``pa_sketch_streamed``)."""
        t = self.torch
        mh = int(max_hash) if max_hash is not None else max_hash_for_scaled(scaled)
        n, bases = host.n_genomes, host.arena_bases
        if arena is None:
            arena = DeviceArena(
                t.empty(max(bases // 16, 1), dtype=t.int32, device=self.device),
                t.empty(max(bases // 32, 1), dtype=t.int32, device=self.device),
                host.genome_start.copy(),
            )
        if arena.dirty is None:
            arena.dirty = t.empty(max((bases // 64 + 63) // 64, 1), dtype=t.int64, device=self.device)
        frac = 1.0 if mh >= 2**64 - 1 else (mh + 1) / 2.0**64
        cap = int(bases * frac * 1.25) + 4096
        off = t.empty(n + 1, dtype=t.int64, device=self.device)
        gs = np.ascontiguousarray(host.genome_start, dtype=np.uint64)
        total = C.c_uint64(0)
        for _attempt in range(2):
            hashes = t.empty(max(cap, 1), dtype=t.int64, device=self.device)
            st = self.lib.pa_sketch_streamed(
                self.ctx, host.packed.data_ptr(), host.run_start.ctypes.data, host.run_len.ctypes.data, len(host.run_start),
                bases, gs.ctypes.data_as(C.POINTER(C.c_uint64)), n, k, mh, arena.packed.data_ptr(), arena.mask.data_ptr(),
                arena.dirty.data_ptr(), hashes.data_ptr(), cap, off.data_ptr(), C.byref(total),
            )  # fmt: skip
            if st == _capi.PA_E_CAPACITY:
                cap = int(total.value)
                continue
            self._check(st, "pa_sketch_streamed")
            return arena, DeviceSketches(hashes, off, n, int(total.value))
        raise HipBackendError("pa_sketch_streamed: capacity retry failed")

    def pair_counts(self, sk: DeviceSketches, q_range=None, s_range=None, algo: int = _capi.PA_PAIRS_AUTO):
        """uint32 |S_q n S_s| for q in q_range, s in s_range -> torch.int32 [nq, ns] on the GPU."""
        t = self.torch
        q0, q1, s0, s1 = _pair_ranges(sk.n, q_range, s_range)
        counts = t.empty((q1 - q0, s1 - s0), dtype=t.int32, device=self.device)
        h_off = sk.offsets_host()  # one small copy per sketch set, cached; the pair phase itself then never waits for the host
        assert h_off.dtype == np.uint64 and len(h_off) == sk.n + 1
        self._check(
            self.lib.pa_pair_counts_ex(
                self.ctx, sk.hashes.data_ptr(), sk.off.data_ptr(), h_off.ctypes.data, sk.n, q0, q1, s0, s1, counts.data_ptr(), algo,
            ),  # fmt: skip
            "pa_pair_counts",
        )
        return counts

    def pair_dict_prepare(self, subject_hashes, n_postings: int) -> None:
        """Enqueue the dictionary build of one subject tile from its ``n_postings`` contiguous hashes (multi-GPU
        overlap with the sketch all-gather); the next default-algorithm ``pair_counts`` over that tile uses it."""
        self._check(self.lib.pa_pair_dict_prepare(self.ctx, subject_hashes.data_ptr(), int(n_postings)), "pa_pair_dict_prepare")

    def ani(self, counts, sk: DeviceSketches, k: int, q_range=None, s_range=None):
        """Device f64 (identity, cov_query); NaN marks the reference's NULL."""
        t = self.torch
        q0, q1, s0, s1 = _pair_ranges(sk.n, q_range, s_range)
        ident = t.empty((q1 - q0, s1 - s0), dtype=t.float64, device=self.device)
        cov = t.empty_like(ident)
        self._check(
            self.lib.pa_ani(self.ctx, counts.data_ptr(), sk.off.data_ptr(), q0, q1, s0, s1, k, ident.data_ptr(), cov.data_ptr()),
            "pa_ani",
        )
        return ident, cov

    # -- bottom-m MinHash + Mash Jaccard (named by BASELINE configs[1]; not a reference code path)
    def sketch_bottom(self, arena: DeviceArena, k: int, m: int) -> DeviceSketches:
        t = self.torch
        n = arena.n_genomes
        hashes = t.empty(max(n * m, 1), dtype=t.int64, device=self.device)
        off = t.empty(n + 1, dtype=t.int64, device=self.device)
        gs = np.ascontiguousarray(arena.genome_start, dtype=np.uint64)
        total = C.c_uint64(0)
        self._check(
            self.lib.pa_sketch_bottom(
                self.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), self.arena_dirty(arena).data_ptr(), arena.arena_bases,
                gs.ctypes.data_as(C.POINTER(C.c_uint64)), n, k, m, hashes.data_ptr(), n * m, off.data_ptr(), C.byref(total),
            ),  # fmt: skip
            "pa_sketch_bottom",
        )
        return DeviceSketches(hashes, off, n, int(total.value))

    def pair_mash(self, sk: DeviceSketches, m: int, q_range=None, s_range=None):
        """(common, denom) int32 tensors [nq, ns] of the Mash Jaccard estimator."""
        t = self.torch
        q0, q1, s0, s1 = _pair_ranges(sk.n, q_range, s_range)
        common = t.empty((q1 - q0, s1 - s0), dtype=t.int32, device=self.device)
        denom = t.empty_like(common)
        self._check(
            self.lib.pa_pair_mash(self.ctx, sk.hashes.data_ptr(), sk.off.data_ptr(), sk.n, q0, q1, s0, s1, m, common.data_ptr(), denom.data_ptr()),
            "pa_pair_mash",
        )
        return common, denom

    def ani_mash(self, common, denom, k: int):
        t = self.torch
        out = t.empty(common.shape, dtype=t.float64, device=self.device)
        self._check(self.lib.pa_ani_mash(self.ctx, common.data_ptr(), denom.data_ptr(), common.numel(), k, out.data_ptr()), "pa_ani_mash")
        return out

    # -- fastANI-style fragment ANI (BASELINE configs[3])
    def fragani(self, arena: DeviceArena, contig_start, contig_len, contig_genome, k: int = 16, frag_len: int = 3000, ref_range=None,
                query_range=None, reuse_index: bool = False, out=None, columns_only: bool = False):
        """All ordered genome pairs: (total_frags[n], matched[n, n], ident_sum[n, n]) as numpy arrays;
        ANI(q, r) = ident_sum / matched (percent), rows = query.  ``ref_range`` = (r0, r1) maps the queries against
        those reference genomes only (the other columns stay 0); ``query_range`` = (q0, q1) maps those query genomes
        only and leaves the other rows of ``out`` = (total, matched, ident_sum) as they are; ``reuse_index``: the
        previous call was on this very arena with the same k and fragment length, take over its reference index;
        ``columns_only``: the two matrices are [n, r1 - r0] -- the columns of the reference range and nothing else."""
        n = arena.n_genomes
        r0, r1 = ref_range if ref_range is not None else (0, n)
        q0, q1 = query_range if query_range is not None else (0, n)
        cols = int(r1) - int(r0) if columns_only else n
        cs = np.ascontiguousarray(contig_start, dtype=np.uint64)
        cl = np.ascontiguousarray(contig_len, dtype=np.uint32)
        cg = np.ascontiguousarray(contig_genome, dtype=np.uint32)
        if out is None:
            total = np.zeros(n, dtype=np.uint32)
            matched = np.zeros((n, cols), dtype=np.uint32)
            ident_sum = np.zeros((n, cols), dtype=np.float64)
        else:
            total, matched, ident_sum = out
            assert total.shape == (n,) and matched.shape == (n, cols) == ident_sum.shape
            assert total.dtype == np.uint32 and matched.dtype == np.uint32 and ident_sum.dtype == np.float64
            assert matched.flags.c_contiguous and ident_sum.flags.c_contiguous
        flags = (_capi.PA_FRAGANI_REUSE_INDEX if reuse_index else 0) | (_capi.PA_FRAGANI_COLUMNS_ONLY if columns_only else 0)
        self._set_ambiguous(arena)
        self._check(
            self.lib.pa_fragani_ex(
                self.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), arena.arena_bases, cs.ctypes.data, cl.ctypes.data,
                cg.ctypes.data, len(cs), n, k, frag_len, int(q0), int(q1), int(r0), int(r1),
                flags, total.ctypes.data, matched.ctypes.data, ident_sum.ctypes.data,
            ),  # fmt: skip
            "pa_fragani",
        )
        return total, matched, ident_sum

    def fragani_sketch(self, arena: DeviceArena, contig_start, contig_len, contig_genome, k: int, window: int):
        """Stage 1 alone: winnowed minimizers (hash, window id, contig) of every contig."""
        cs = np.ascontiguousarray(contig_start, dtype=np.uint64)
        cl = np.ascontiguousarray(contig_len, dtype=np.uint32)
        cg = np.ascontiguousarray(contig_genome, dtype=np.uint32)
        cap = max(1024, arena.arena_bases)  # at most one minimizer per position
        h = np.zeros(cap, dtype=np.uint32)
        wp = np.zeros(cap, dtype=np.uint32)
        ct = np.zeros(cap, dtype=np.uint32)
        n = C.c_uint64(0)
        self._set_ambiguous(arena)
        self._check(
            self.lib.pa_fragani_sketch(
                self.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), arena.arena_bases, cs.ctypes.data, cl.ctypes.data,
                cg.ctypes.data, len(cs), arena.n_genomes, k, window, h.ctypes.data, wp.ctypes.data, ct.ctypes.data, cap, C.byref(n),
            ),  # fmt: skip
            "pa_fragani_sketch",
        )
        m = int(n.value)
        return h[:m], wp[:m], ct[:m]

    def fragani_workspace(self) -> dict:
        """Device bytes of the context's fragment-ANI workspace: held now, the most ever held, the cap (0: none)."""
        held, peak, cap = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.pa_fragani_workspace(self.ctx, C.byref(held), C.byref(peak), C.byref(cap)), "pa_fragani_workspace")
        return {"held_bytes": int(held.value), "peak_bytes": int(peak.value), "cap_bytes": int(cap.value)}

    def fragani_set_workspace_cap(self, cap_bytes: int) -> None:
        """Later fragment-ANI calls that would take the workspace past ``cap_bytes`` (0: no cap) fail with a message naming
        the call and the sizes (``HipBackendError``), the workspace as it was."""
        self._check(self.lib.pa_fragani_set_workspace_cap(self.ctx, int(cap_bytes)), "pa_fragani_set_workspace_cap")

    # -- external alignment
    def msa_upload(self, msa: "LoadedMSA", *, chunk_bytes: int = 1 << 29, table=None) -> "DeviceMSA":
        """Rows -> bit planes on the device (``pa_msa_pack``), the rows uploaded in chunks of at most ``chunk_bytes``.
        ``table``: ``(code, bits)`` to pack with (default: ``msa_code_table`` of the alignment's bytes)."""
        t = self.torch
        code, bits = table if table is not None else msa_code_table(msa.histogram)
        n, stride = msa.n_rows, msa.rows.shape[1]
        words = int(self.lib.pa_msa_plane_words(n, msa.n_cols, bits))
        planes = t.empty(max(words, 1), dtype=t.int32, device=self.device)
        nongap = t.zeros(max(n, 1), dtype=t.int32, device=self.device)
        step = max(1, int(chunk_bytes) // stride)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            d_rows = t.from_numpy(msa.rows[r0:r1]).to(self.device)
            self._check(
                self.lib.pa_msa_pack(
                    self.ctx, d_rows.data_ptr(), stride, r0, r1 - r0, n, msa.n_cols, code.ctypes.data, bits, planes.data_ptr(), nongap.data_ptr()
                ),
                "pa_msa_pack",
            )
            self.sync()  # d_rows is freed by the next iteration
        return DeviceMSA(planes, nongap, n, msa.n_cols, bits)


    def msa_pair_counts(self, dm: "DeviceMSA", q_range=None, s_range=None, *, symmetric: bool = False):
        """(M, B) as torch.int32 [nq, ns] on the device for rows q_range x s_range (uint32 values)."""
        t = self.torch
        q0, q1, s0, s1 = _pair_ranges(dm.n_rows, q_range, s_range)
        match = t.empty((q1 - q0, s1 - s0), dtype=t.int32, device=self.device)
        both = t.empty((q1 - q0, s1 - s0), dtype=t.int32, device=self.device)
        if match.numel() == 0:
            return match, both
        self._check(
            self.lib.pa_msa_pair_counts(
                self.ctx, dm.planes.data_ptr(), dm.n_rows, dm.n_cols, dm.bits, q0, q1, s0, s1, int(bool(symmetric)), match.data_ptr(), both.data_ptr()
            ),
            "pa_msa_pair_counts",
        )
        return match, both

    # -- bootstrap-run
    def msa_boot_counts(self, dm: "DeviceMSA", weights):
        """``pa_msa_boot_counts``: ``(M, B)`` of every pair of rows of ``dm`` under each row of ``weights`` (uint8,
        R x ``dm.n_cols`` on the host, each row adding up to the columns) as torch.int32 ``[R, n, n]`` on the device (uint32
        values), the diagonal included: the same integers as ``msa_boot_counts_host``."""
        t = self.torch
        w = _boot_weights(weights, dm.n_cols)
        n = dm.n_rows
        match = t.empty((len(w), n, n), dtype=t.int32, device=self.device)
        both = t.empty((len(w), n, n), dtype=t.int32, device=self.device)
        if match.numel():
            self._check(
                self.lib.pa_msa_boot_counts(self.ctx, dm.planes.data_ptr(), n, dm.n_cols, dm.bits, w.ctypes.data, len(w), match.data_ptr(), both.data_ptr()),
                "pa_msa_boot_counts",
            )
        return match, both

    def msa_boot_distances(self, match, both, missing: float = 1.0):
        """``pa_msa_boot_distances``: the replicates' distance matrices, float64 ``[R, n, n]`` on the device, from the
        counts of ``msa_boot_counts``; each ``D[r]`` is ready for ``nj_tree_inplace``.  The same bits as
        ``msa_boot_distances_host``."""
        t = self.torch
        reps, n = int(match.shape[0]), int(match.shape[1])
        d = t.empty((reps, n, n), dtype=t.float64, device=self.device)
        if d.numel():
            self._check(self.lib.pa_msa_boot_distances(self.ctx, match.data_ptr(), both.data_ptr(), n, reps, float(missing), d.data_ptr()),
                        "pa_msa_boot_distances")
        return d

    # -- phylo-run
    def msa_subst_upload(self, msa: "LoadedMSA", *, chunk_bytes: int = 1 << 29) -> "DeviceMSA":
        """``msa_upload`` with the nucleotide code of ``pa_subst_code`` at ``PA_SUBST_BITS``: the planes
        ``msa_subst_counts`` reads."""
        return self.msa_upload(msa, chunk_bytes=chunk_bytes, table=(subst_code_table(), _capi.PA_SUBST_BITS))

    def msa_subst_counts(self, dm: "DeviceMSA", weights=None):
        """``pa_msa_subst_counts``: ``(V, S, T)`` of every pair of rows of ``dm`` (from ``msa_subst_upload``) as
        torch.int32 ``[R, n, n]`` on the device (uint32 values): without ``weights`` R = 1 and every column counts once,
        with them (uint8, R x ``dm.n_cols`` on the host, each row adding up to the columns) a matrix per row.  The same
        integers as ``msa_subst_counts_host``."""
        t = self.torch
        if dm.bits != _capi.PA_SUBST_BITS:
            raise ValueError(f"planes of {dm.bits} bits: msa_subst_counts reads what msa_subst_upload packs ({_capi.PA_SUBST_BITS} bits)")
        w = None if weights is None else _boot_weights(weights, dm.n_cols)
        reps, n = 1 if w is None else len(w), dm.n_rows
        out = tuple(t.empty((reps, n, n), dtype=t.int32, device=self.device) for _ in range(3))
        if out[0].numel():
            self._check(
                self.lib.pa_msa_subst_counts(self.ctx, dm.planes.data_ptr(), n, dm.n_cols, None if w is None else w.ctypes.data, reps,
                                             *(x.data_ptr() for x in out)),
                "pa_msa_subst_counts",
            )  # fmt: skip
        return out

    def subst_distances(self, valid, ts, tv, model: str = "k80", missing: float = 3.0):
        """``pa_subst_distances``: ``(D, undefined)`` -- the distance matrices of ``model`` (``SUBST_MODELS``), float64
        ``[R, n, n]`` on the device, each ``D[r]`` ready for ``nj_tree_inplace``, and per matrix the unordered pairs
        without a shared nucleotide column and the saturated ones (uint64 ``[R, 2]``, host).  The same bits as
        ``subst_distances_host``."""
        t = self.torch
        reps, n = int(valid.shape[0]), int(valid.shape[1])
        d = t.empty((reps, n, n), dtype=t.float64, device=self.device)
        undefined = np.zeros((reps, 2), dtype=np.uint64)
        self._check(
            self.lib.pa_subst_distances(self.ctx, valid.data_ptr(), ts.data_ptr(), tv.data_ptr(), n, reps, _subst_model(model), float(missing), d.data_ptr(),
                                        undefined.ctypes.data),
            "pa_subst_distances",
        )  # fmt: skip
        return d, undefined

    def nj_tree_inplace(self, d) -> tuple[np.ndarray, np.ndarray, np.ndarray, float]:
        """``nj_tree`` of a contiguous n x n float64 tensor on this device, which the call overwrites: no copy is made."""
        n = int(d.shape[0])
        out = _nj_outputs(n)
        self._check(self.lib.pa_nj(self.ctx, d.data_ptr(), n, *(a.ctypes.data for a in out)), "pa_nj")
        return out[0], out[1], out[2], float(out[3][0])

    # -- classify
    def classify_edges_device(self, score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", cov_min: float = 0.5):
        """``pa_classify_edges``: the edges of the genome graph in removal order as device tensors ``(i, j, score, cov)``
        (int32 views of uint32, float64), trimmed to the number of edges.  ``score`` and ``cov`` are N x N float64,
        host arrays or tensors on this device."""
        t = self.torch
        d_score, d_cov = self._f64_on_device(score), self._f64_on_device(cov)
        n = d_score.shape[0]
        if d_score.shape != (n, n) or d_cov.shape != (n, n):
            raise ValueError(f"score {tuple(d_score.shape)} and coverage {tuple(d_cov.shape)} must be square and equal")
        agg_score, agg_cov = _pair_agg(score_edges, "score"), _pair_agg(coverage_edges, "coverage")
        cap = n * (n - 1) // 2
        e_i = t.empty(cap, dtype=t.int32, device=self.device)
        e_j = t.empty(cap, dtype=t.int32, device=self.device)
        e_s = t.empty(cap, dtype=t.float64, device=self.device)
        e_c = t.empty(cap, dtype=t.float64, device=self.device)
        count = C.c_uint64(0)
        self._check(
            self.lib.pa_classify_edges(
                self.ctx, d_score.data_ptr(), d_cov.data_ptr(), n, agg_score, agg_cov, float(cov_min), cap,
                e_i.data_ptr(), e_j.data_ptr(), e_s.data_ptr(), e_c.data_ptr(), C.byref(count),
            ),  # fmt: skip
            "pa_classify_edges",
        )
        m = count.value
        return e_i[:m], e_j[:m], e_s[:m], e_c[:m]

    def classify_edges(self, score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", cov_min: float = 0.5):
        """``classify_edges_device`` copied back: ``(i, j, score, cov)`` as host arrays (uint32, uint32, float64, float64)."""
        e_i, e_j, e_s, e_c = self.classify_edges_device(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, cov_min=cov_min)
        return e_i.cpu().numpy().view(np.uint32), e_j.cpu().numpy().view(np.uint32), e_s.cpu().numpy(), e_c.cpu().numpy()

    # -- plot-run
    def row_distances_device(self, matrix):
        """``pa_rowdist_euclid``: the condensed Euclidean distances between the rows of ``matrix`` (n x m float64, a
        host array or a tensor on this device; finite values) as a device tensor of n (n - 1) / 2 float64."""
        t = self.torch
        d_x = self._f64_on_device(matrix)
        if d_x.dim() != 2:
            raise ValueError(f"matrix has shape {tuple(d_x.shape)}, expected two dimensions")
        n, m = d_x.shape
        if n > 1 << 16:  # the library's limit, checked before n (n - 1) / 2 doubles are allocated for it to refuse
            raise ValueError(f"{n} rows; at most 65536")
        out = t.empty(n * (n - 1) // 2, dtype=t.float64, device=self.device)
        self._check(self.lib.pa_rowdist_euclid(self.ctx, d_x.data_ptr(), n, m, out.data_ptr()), "pa_rowdist_euclid")
        return out

    def row_distances(self, matrix) -> np.ndarray:
        """``row_distances_device`` copied back: the same bits as ``scipy.spatial.distance.pdist(matrix, "euclidean")``."""
        return self.row_distances_device(matrix).cpu().numpy()

    # -- plot-run-comp
    def _f64_on_device(self, values):
        t = self.torch
        if not isinstance(values, t.Tensor):
            values = t.from_numpy(np.ascontiguousarray(values, dtype=np.float64))
        return values.to(device=self.device, dtype=t.float64).contiguous()

    def _u32_on_device(self, index):
        """A u32 index array as an int32 tensor with the same bits (0xFFFFFFFF is -1)."""
        t = self.torch
        if not isinstance(index, t.Tensor):
            index = t.from_numpy(np.ascontiguousarray(index, dtype=np.uint32).view(np.int32))
        if index.dtype != t.int32:
            raise ValueError(f"index tensor of {index.dtype}, expected int32 (the bits of the u32 indices)")
        return index.to(device=self.device).contiguous()

    def run_join_device(self, ref, q, s, y):
        """``pa_runcomp_join``: ``(x, y, d)`` as device tensors trimmed to the rows in common, in input order.  ``ref``
        is the reference run's N x N float64 identity matrix (NaN: no value), ``q`` and ``s`` the u32 row and column of
        each comparison of the other run (0xFFFFFFFF: not a genome of the reference run; int32 tensors with those bits),
        ``y`` its identity (NaN: NULL); host arrays or tensors on this device."""
        t = self.torch
        d_ref, d_q, d_s, d_y = self._f64_on_device(ref), self._u32_on_device(q), self._u32_on_device(s), self._f64_on_device(y)
        n_ref = d_ref.shape[0] if d_ref.dim() == 2 else -1
        if d_ref.dim() != 2 or d_ref.shape != (n_ref, n_ref):
            raise ValueError(f"reference matrix of shape {tuple(d_ref.shape)}, expected a square one")
        n_rows = d_y.numel()
        if d_q.shape != (n_rows,) or d_s.shape != (n_rows,) or d_y.shape != (n_rows,):
            raise ValueError(f"q {tuple(d_q.shape)}, s {tuple(d_s.shape)} and y {tuple(d_y.shape)} must be vectors of one length")
        if n_ref > 1 << 16:  # the library's limit
            raise ValueError(f"{n_ref} genomes in the reference run; at most 65536")
        out =t.empty((3, n_rows), dtype=t.float64, device=self.device)
        count = C.c_uint64(0)
        self._check(
            self.lib.pa_runcomp_join(
                self.ctx, d_ref.data_ptr(), n_ref, d_q.data_ptr(), d_s.data_ptr(), d_y.data_ptr(), n_rows, out[0].data_ptr(), out[1].data_ptr(),
                out[2].data_ptr(), C.byref(count),
            ),  # fmt: skip
            "pa_runcomp_join",
        )
        m = count.value
        return out[0, :m], out[1, :m], out[2, :m]

    def run_join(self, ref, q, s, y):
        """``run_join_device`` copied back: ``(x, y, d)`` as host float64 arrays."""
        return tuple(v.cpu().numpy() for v in self.run_join_device(ref, q, s, y))

    def minmax(self, values) -> tuple[float, float, int]:
        """``pa_minmax_f64``: ``(minimum, maximum, n_valid)`` of the non-NaN values of ``values`` (a host array or a
        float64 tensor on this device, which is not copied); ``(nan, nan, 0)`` when there is none."""
        d_v = self._f64_on_device(values).reshape(-1)
        out = (C.c_double * 2)(float("nan"), float("nan"))
        valid = C.c_uint64(0)
        self._check(self.lib.pa_minmax_f64(self.ctx, d_v.data_ptr(), d_v.numel(), out, C.byref(valid)), "pa_minmax_f64")
        return float(out[0]), float(out[1]), int(valid.value)

    def _hist_uniform(self, symbol: str, values, edges) -> np.ndarray:
        d_v = self._f64_on_device(values).reshape(-1)
        h_edges = np.ascontiguousarray(edges, dtype=np.float64)
        if h_edges.ndim != 1 or len(h_edges) < 2:
            raise ValueError(f"edges of shape {h_edges.shape}, expected at least two in one dimension")
        counts = np.zeros(len(h_edges) - 1, dtype=np.uint64)
        self._check(getattr(self.lib, symbol)(self.ctx, d_v.data_ptr(), d_v.numel(), h_edges.ctypes.data, len(counts), counts.ctypes.data), symbol)
        return counts

    def hist_uniform(self, values, edges) -> np.ndarray:
        """``pa_hist_uniform_f64``: the uint64 counts of ``numpy.histogram`` over the uniform bins whose ascending
        ``edges`` the caller made (``run_comp.hist_edges``); ``values`` is a host array or a float64 tensor on this
        device, which is not copied.  NaN and values outside the edges are not counted."""
        return self._hist_uniform("pa_hist_uniform_f64", values, edges)

    # -- plot-run's distributions
    def select(self, values, ranks) -> np.ndarray:
        """``pa_select_f64``: the values at the zero-based ``ranks`` (at most 8, in any order) among the non-NaN
        elements of ``values`` in ascending order, ``numpy.sort(v)[ranks]``; ``values`` is a host array or a float64
        tensor on this device, which is neither copied nor sorted."""
        d_v = self._f64_on_device(values).reshape(-1)
        h_ranks = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
        out = np.empty(len(h_ranks), dtype=np.float64)
        self._check(self.lib.pa_select_f64(self.ctx, d_v.data_ptr(), d_v.numel(), h_ranks.ctypes.data, len(h_ranks), out.ctypes.data), "pa_select_f64")
        return out

    def moments(self, values) -> tuple[float, float]:
        """``pa_moments_f64``: the mean of the non-NaN elements of ``values`` and the sum of their squared deviations
        from it, the same bits every run; ``(nan, nan)`` when there is none."""
        d_v = self._f64_on_device(values).reshape(-1)
        out = (C.c_double * 2)(float("nan"), float("nan"))
        self._check(self.lib.pa_moments_f64(self.ctx, d_v.data_ptr(), d_v.numel(), out), "pa_moments_f64")
        return float(out[0]), float(out[1])

    def kde_gauss(self, values, grid, bw: float) -> np.ndarray:
        """``pa_kde_gauss_f64``: the Gaussian kernel density of the non-NaN elements of ``values`` with bandwidth ``bw``
        at the ``grid`` points (at most 1024), the same bits every run."""
        d_v = self._f64_on_device(values).reshape(-1)
        h_grid = np.ascontiguousarray(grid, dtype=np.float64).reshape(-1)
        density = np.empty(len(h_grid), dtype=np.float64)
        self._check(
            self.lib.pa_kde_gauss_f64(self.ctx, d_v.data_ptr(), d_v.numel(), h_grid.ctypes.data, len(h_grid), float(bw), density.ctypes.data), "pa_kde_gauss_f64"
        )
        return density

    def hist_uniform_wide(self, values, edges) -> np.ndarray:
        """``pa_hist_uniform_f64_wide``: ``hist_uniform`` for up to 2^20 bins."""
        return self._hist_uniform("pa_hist_uniform_f64_wide", values, edges)

    # -- plot-run's scatter figures
    def bin2d(self, x, y, xedges, yedges) -> tuple[np.ndarray, np.ndarray]:
        """``pa_bin2d_f64``: ``(counts, last)``, uint64 arrays of shape ``(len(xedges) - 1, len(yedges) - 1)``:
        ``numpy.histogram2d``'s counts of the points ``(x, y)`` over the uniform edges the caller made
        (``run_comp.hist_edges``, at most 1024 bins an axis) and the largest index among each cell's points
        (``scatter.NONE`` for an empty cell), the same bits every run.  ``x`` and ``y`` are host arrays or float64 tensors
        on this device, which are read in place."""
        d_x, d_y = self._f64_on_device(x).reshape(-1), self._f64_on_device(y).reshape(-1)
        if d_x.shape != d_y.shape:
            raise ValueError(f"{d_x.numel()} x values and {d_y.numel()} y values")
        h_xe, h_ye = np.ascontiguousarray(xedges, dtype=np.float64), np.ascontiguousarray(yedges, dtype=np.float64)
        for h_edges in (h_xe, h_ye):
            if h_edges.ndim != 1 or len(h_edges) < 2:
                raise ValueError(f"edges of shape {h_edges.shape}, expected at least two in one dimension")
        shape = (len(h_xe) - 1, len(h_ye) - 1)
        counts, last = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
        self._check(
            self.lib.pa_bin2d_f64(self.ctx, d_x.data_ptr(), d_y.data_ptr(), d_x.numel(), h_xe.ctypes.data, shape[0], h_ye.ctypes.data, shape[1],
                                  counts.ctypes.data, last.ctypes.data),
            "pa_bin2d_f64",
        )  # fmt: skip
        return counts, last

    # -- TETRA-hip
    def tetra_counts(self, arena, *, use_dirty: bool = True) -> np.ndarray:
        """``pa_tetra_counts``: the forward di-, tri- and tetranucleotide counts of every genome of ``arena`` (a
        ``DeviceArena``, or a ``HostArena`` that is uploaded first) as a host uint64 array ``[n_genomes, 336]``.
        ``use_dirty`` False hands the library no dirty bitmap (it then builds its own)."""
        t = self.torch
        if isinstance(arena, HostArena):
            arena = self.upload(arena)
        n = arena.n_genomes
        counts = t.empty((max(n, 1), _capi.PA_TETRA_BINS), dtype=t.int64, device=self.device)
        gs = np.ascontiguousarray(arena.genome_start, dtype=np.uint64)
        dirty = self.arena_dirty(arena).data_ptr() if use_dirty and arena.arena_bases else None
        self._check(
            self.lib.pa_tetra_counts(self.ctx, arena.packed.data_ptr(), arena.mask.data_ptr(), dirty, arena.arena_bases, gs.ctypes.data, n,
                                     counts.data_ptr()),
            "pa_tetra_counts",
        )  # fmt: skip
        return counts[:n].cpu().numpy().view(np.uint64)

    def tetra_correlations_device(self, U, q_range=None, s_range=None):
        """``pa_tetra_corr``: the correlations of the unit rows ``U`` (``[n, 256]`` float64, a host array or a tensor on
        this device), queries ``q_range`` against subjects ``s_range`` (default: all), as a device tensor; a square block
        on the diagonal is evaluated above the diagonal and mirrored."""
        t = self.torch
        d_u = self._f64_on_device(U)
        if d_u.dim() != 2 or d_u.shape[1] != _capi.PA_TETRA_WORDS:
            raise ValueError(f"U has shape {tuple(d_u.shape)}, expected (n, {_capi.PA_TETRA_WORDS})")
        n = d_u.shape[0]
        q0, q1, s0, s1 = _pair_ranges(n, q_range, s_range, tetra=True)
        out = t.empty((q1 - q0, s1 - s0), dtype=t.float64, device=self.device)
        self._check(self.lib.pa_tetra_corr(self.ctx, d_u.data_ptr(), n, q0, q1, s0, s1, int((q0, q1) == (s0, s1)), out.data_ptr()), "pa_tetra_corr")
        return out

    def tetra_correlations(self, U, q_range=None, s_range=None) -> np.ndarray:
        """``tetra_correlations_device`` copied back: the same bits as ``tetra_correlations_host``."""
        return self.tetra_correlations_device(U, q_range, s_range).cpu().numpy()

    # -- profiling
    # -- tree-run
    def nj_tree(self, D) -> tuple[np.ndarray, np.ndarray, np.ndarray, float]:
        """``pa_nj``: the neighbour-joining tree of the n x n float64 distance matrix ``D`` (a host array or a tensor on
        this device; finite, >= 0, bitwise symmetric, zero diagonal) as ``(child, length, last, last_len)``: join t makes
        node n + t from ``child[t]`` (uint32, (n - 2) x 2) with the branch lengths ``length[t]``; ``last`` is the edge
        between the two nodes that remain and ``last_len`` its length.  The library works on a copy of ``D``."""
        t = self.torch
        if isinstance(D, np.ndarray) and not D.flags.writeable:
            D = D.copy()  # torch wraps writable arrays only
        d = self._f64_on_device(D)
        if d.dim() != 2 or d.shape[0] != d.shape[1]:
            raise ValueError(f"distance matrix of shape {tuple(d.shape)}, expected a square one")
        n = d.shape[0]
        if n > 65535:  # the library's limit, checked before a copy of n^2 doubles is made for it to refuse
            raise ValueError(f"{n} nodes; at most 65535")
        work = d.clone() if isinstance(D, t.Tensor) and d.data_ptr() == D.data_ptr() else d  # the call overwrites its matrix
        out = _nj_outputs(n)
        self._check(self.lib.pa_nj(self.ctx, work.data_ptr(), n, *(a.ctypes.data for a in out)), "pa_nj")
        return out[0], out[1], out[2], float(out[3][0])

    # -- ordinate-run
    def _square_f64_on_device(self, M, what: str):
        if isinstance(M, np.ndarray) and not M.flags.writeable:
            M = M.copy()  # torch wraps writable arrays only
        m = self._f64_on_device(M)
        if m.dim() != 2 or m.shape[0] != m.shape[1]:
            raise ValueError(f"{what} of shape {tuple(m.shape)}, expected a square one")
        if m.shape[0] > 65535:
            raise ValueError(f"{m.shape[0]} rows; at most 65535")
        return m

    def mul_tall_device(self, A, Q):
        """``pa_mul_tall_f64``: ``A @ Q`` for the n x n float64 ``A`` and the n x p block ``Q`` (host arrays or tensors
        on this device; p <= 32) as a device tensor, added in the order of the contract: the same
        bits run to run and as ``mul_tall_host``."""
        t = self.torch
        a = self._square_f64_on_device(A, "matrix")
        q = self._f64_on_device(Q.copy() if isinstance(Q, np.ndarray) and not Q.flags.writeable else Q)
        if q.dim() != 2 or q.shape[0] != a.shape[0]:
            raise ValueError(f"block of shape {tuple(q.shape)} for a matrix of {a.shape[0]} rows")
        y = t.empty(q.shape, dtype=t.float64, device=self.device)
        self._check(self.lib.pa_mul_tall_f64(self.ctx, a.data_ptr(), a.shape[0], q.data_ptr(), q.shape[1], y.data_ptr()), "pa_mul_tall_f64")
        return y

    def mul_tall(self, A, Q) -> np.ndarray:
        """``mul_tall_device`` copied back."""
        return self.mul_tall_device(A, Q).cpu().numpy()

    def gower_center_device(self, D):
        """``pa_gower_center``: ``(B, trace, fro2)`` of the n x n float64 distance matrix ``D`` (a host array or a tensor
        on this device; finite, >= 0, bitwise symmetric, zero diagonal), ``B`` the doubly centred matrix of the squared
        distances as a device tensor, with its trace and its squared Frobenius norm.  ``D`` is not modified."""
        t = self.torch
        d = self._square_f64_on_device(D, "distance matrix")
        b = t.empty_like(d)
        trace, fro2 = C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.pa_gower_center(self.ctx, d.data_ptr(), d.shape[0], b.data_ptr(), C.byref(trace), C.byref(fro2)), "pa_gower_center")
        return b, trace.value, fro2.value

    def gower_center(self, D) -> tuple[np.ndarray, float, float]:
        """``gower_center_device`` with ``B`` copied back: the same bits as ``gower_center_host``."""
        b, trace, fro2 = self.gower_center_device(D)
        return b.cpu().numpy(), trace, fro2

    def symm_top_eigs(self, B, k: int, fro2: float, tol: float = 1e-10, max_iter: int = 10000):
        """``pa_symm_top_eigs``: the ``k`` algebraically largest eigenvalues of the symmetric n x n float64 ``B`` (a host
        array or a tensor on this device, only read) with ``fro2`` its squared Frobenius norm, as ``(values, vectors,
        residuals, info)``: descending values, the unit eigenvectors as the columns of the n x k ``vectors``, each pair's
        residual norm and ``info = (iterations of phase 1, iterations in all, shift used)``.  The products run on the
        GPU, the p-wide algebra on the host: the same bits as ``symm_top_eigs_host``.  A call that uses up ``max_iter``
        raises with status ``PA_E_NOCONVERGE``."""
        b = self._square_f64_on_device(B, "matrix")
        n = b.shape[0]
        out = _eigs_outputs(n, k)
        self._check(
            self.lib.pa_symm_top_eigs(self.ctx, b.data_ptr(), n, int(k), float(tol), int(max_iter), float(fro2), *(a.ctypes.data for a in out)),
            "pa_symm_top_eigs",
        )
        return _eigs_result(out)

    # -- mantel-run-comp
    def mantel(self, X, Y, perms) -> tuple[np.ndarray, np.ndarray]:
        """``pa_mantel``: ``(stats, cross)`` of the n x n float64 distance matrices ``X`` and ``Y`` (host arrays or tensors
        on this device, which are used as they are and left alone; each finite, >= 0, bitwise symmetric, zero diagonal)
        under the rows of ``perms`` (uint32, P x n, each a permutation of 0 .. n - 1; row q pairs row i of ``X`` with row
        ``perms[q, i]`` of ``Y``).  ``stats`` = (mean_x, mean_y, ss_x, ss_y); ``cross[0]`` is the identity's cross sum
        and ``cross[1 + q]`` that of row q: the same bits as ``mantel_host``."""
        x = self._square_f64_on_device(X, "distance matrix")
        y = self._square_f64_on_device(Y, "distance matrix")
        n, p = _mantel_arguments(x.shape, y.shape, perms)
        out = _mantel_outputs(len(p))
        self._check(self.lib.pa_mantel(self.ctx, x.data_ptr(), y.data_ptr(), n, p.ctypes.data, len(p), *(a.ctypes.data for a in out)), "pa_mantel")
        return out

    # -- dereplicate-run
    def derep_adjacency_device(self, score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", min_score: float = 0.95,
                               cov_min: float = 0.5):
        """``pa_derep_adjacency``: the threshold graph of the n x n float64 ``score`` and ``cov`` (host arrays or tensors on
        this device, left alone) as a device tensor of n x ceil(n / 64) int64 words (views of uint64): bit b of word w of
        row a says whether a and 64 w + b are adjacent."""
        t = self.torch
        s = self._square_f64_on_device(score, "score matrix")
        c = self._square_f64_on_device(cov, "coverage matrix")
        _derep_same_shape(s.shape, c.shape)
        n = s.shape[0]
        bits = t.empty((n, (n + 63) // 64), dtype=t.int64, device=self.device)
        self._check(
            self.lib.pa_derep_adjacency(self.ctx, s.data_ptr(), c.data_ptr(), n, _pair_agg(score_edges, "score"), _pair_agg(coverage_edges, "coverage"),
                                        float(min_score), float(cov_min), bits.data_ptr()),
            "pa_derep_adjacency",
        )  # fmt: skip
        return bits

    def _derep_bits_on_device(self, bits, n: int):
        """A bit matrix of n nodes (a host array of uint64, or an int64 tensor with the same bits) on this device."""
        t = self.torch
        b = bits if isinstance(bits, t.Tensor) else t.from_numpy(np.ascontiguousarray(bits, dtype=np.uint64).view(np.int64).copy())
        b = b.to(self.device).contiguous()
        if b.dtype != t.int64 or b.numel() != n * ((n + 63) // 64):
            raise ValueError(f"bit matrix of {b.numel()} {b.dtype} words for {n} nodes, expected {n} x {(n + 63) // 64} of 64 bits")
        return b

    def derep_select_device(self, bits, n: int, mode: str = "greedy"):
        """``pa_derep_select``: ``(is_rep, n_reps, n_rounds)`` of the bit matrix ``bits`` (n x ceil(n / 64) words, a host
        array or a tensor on this device): ``is_rep`` a device tensor of n uint8, the number of representatives, and the
        number of rounds the device took (a diagnostic)."""
        t = self.torch
        n = int(n)
        b = self._derep_bits_on_device(bits, n)
        is_rep = t.empty(max(n, 1), dtype=t.uint8, device=self.device)
        n_reps, n_rounds = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.pa_derep_select(self.ctx, b.data_ptr(), n, _derep_mode(mode), is_rep.data_ptr(), C.byref(n_reps), C.byref(n_rounds)),
                    "pa_derep_select")
        return is_rep[:n], n_reps.value, n_rounds.value

    def derep_assign_device(self, score, bits, is_rep, *, score_edges: str = "mean"):
        """``pa_derep_assign``: ``(rep, rep_score)`` as device tensors (int32 views of uint32, float64): every node's
        representative among the set bits of its row that ``is_rep`` marks, and the pair's score."""
        t = self.torch
        s = self._square_f64_on_device(score, "score matrix")
        n = s.shape[0]
        b = self._derep_bits_on_device(bits, n)
        r = (is_rep if isinstance(is_rep, t.Tensor) else t.from_numpy(np.ascontiguousarray(is_rep, dtype=np.uint8).copy())).to(self.device).contiguous()
        if r.dtype != t.uint8 or r.numel() != n:
            raise ValueError(f"{r.numel()} marks of {r.dtype} for {n} nodes, expected {n} of uint8")
        rep = t.empty(max(n, 1), dtype=t.int32, device=self.device)
        rep_score = t.empty(max(n, 1), dtype=t.float64, device=self.device)
        self._check(self.lib.pa_derep_assign(self.ctx, s.data_ptr(), n, _pair_agg(score_edges, "score"), b.data_ptr(), r.data_ptr(), rep.data_ptr(),
                                             rep_score.data_ptr()), "pa_derep_assign")  # fmt: skip
        return rep[:n], rep_score[:n]

    def dereplicate(self, score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", min_score: float = 0.95, cov_min: float = 0.5,  # noqa: PLR0913
                    mode: str = "greedy") -> Dereplication:
        """One representative per group of the threshold graph of ``score`` and ``cov`` (n x n float64, host arrays or
        tensors on this device, left alone; node p is row and column p, a lower index is the preferred genome): the
        three calls above, the matrices uploaded once and the bit matrix never leaving the device.  The same bits as
        ``dereplicate_host``."""
        s = self._square_f64_on_device(score, "score matrix")
        c = self._square_f64_on_device(cov, "coverage matrix")
        bits = self.derep_adjacency_device(s, c, score_edges=score_edges, coverage_edges=coverage_edges, min_score=min_score, cov_min=cov_min)
        is_rep, n_reps, n_rounds = self.derep_select_device(bits, s.shape[0], mode)
        rep, rep_score = self.derep_assign_device(s, bits, is_rep, score_edges=score_edges)
        return Dereplication(is_rep.cpu().numpy().astype(bool), rep.cpu().numpy().view(np.uint32), rep_score.cpu().numpy(), n_reps, n_rounds)

    # -- search-run
    def _u32_words_on_device(self, values, n: int, what: str):
        """``n`` uint32 words (a host array, or an int32 tensor with the same bits) on this device."""
        t = self.torch
        v = values if isinstance(values, t.Tensor) else t.from_numpy(_hit_sizes(values, what).view(np.int32).copy())
        v = v.to(self.device).contiguous()
        if v.dtype != t.int32 or v.numel() != n:
            raise ValueError(f"{what}: {v.numel()} words of {v.dtype}, expected {n} of 32 bits")
        return v

    def best_hits_device(self, counts, q_size, s_size, s_base: int, rank: str, top: int, state=None):  # noqa: PLR0913
        """``pa_best_hits``: ``(subject, shared, denom)``, three device tensors of nq x ``top`` int32 (views of uint32), the
        best ``top`` columns of every row of ``counts`` (a device tensor of nq x ns int32 as ``pair_counts`` returns it;
        a row stride above ns is taken as it is) under ``rank`` ("identity" or "containment"), best first, a missing rank
        ``PA_HITS_NONE``, 0, 0; column c is subject ``s_base`` + c.  ``q_size`` and ``s_size``: the sketch sizes, host
        arrays (checked: 1 to 2^32 - 1) or int32 tensors on this device (not checked).  ``state``: the three tensors an
        earlier call returned for other columns; they take part, are overwritten and returned."""
        t = self.torch
        if not isinstance(counts, t.Tensor) or counts.dtype != t.int32 or counts.dim() != 2 or counts.device != self.device:  # noqa: PLR2004
            raise ValueError("counts: expected an nq x ns int32 tensor on this device")
        nq, ns = counts.shape
        if ns and counts.stride(1) != 1:
            counts = counts.contiguous()
        ld = counts.stride(0) if nq > 1 and ns else ns
        q = self._u32_words_on_device(q_size, nq, "query sizes")
        s = self._u32_words_on_device(s_size, ns, "subject sizes")
        if state is None:
            out = tuple(t.empty((nq, max(int(top), 1)), dtype=t.int32, device=self.device) for _ in range(3))
        else:
            out = tuple(state)
            if len(out) != 3 or any(not isinstance(x, t.Tensor) or x.dtype != t.int32 or x.shape != (nq, int(top)) or not x.is_contiguous()  # noqa: PLR2004
                                    or x.device != self.device for x in out):
                raise ValueError(f"state: expected three contiguous {nq} x {top} int32 tensors on this device")
        self._check(self.lib.pa_best_hits(self.ctx, counts.data_ptr(), nq, ns, ld, q.data_ptr(), s.data_ptr(), int(s_base), _hits_rank(rank), int(top),
                                          int(state is not None), *(x.data_ptr() for x in out)), "pa_best_hits")  # fmt: skip
        return out

    def prof_enable(self, on: bool = True) -> None:
        self._check(self.lib.pa_prof_enable(self.ctx, int(on)), "pa_prof_enable")

    def prof_reset(self) -> None:
        self._check(self.lib.pa_prof_reset(self.ctx), "pa_prof_reset")

    def prof_get(self) -> dict[str, tuple[float, int]]:
        out = {}
        for name, idx in _capi.PROF_PHASES.items():
            ms, n = C.c_double(0), C.c_uint64(0)
            self._check(self.lib.pa_prof_get(self.ctx, idx, C.byref(ms), C.byref(n)), "pa_prof_get")
            out[name] = (ms.value, int(n.value))
        return out


def ani_host(counts: np.ndarray, q_sizes, s_sizes, k: int, *, symmetric: bool = False, threads: int = 0, out=None):
    """Strict (host libm ``pow``) containment-ANI transform used at the JSON/DB boundary.

    ``symmetric``: the block is square and rows and columns are the same genomes in the same order (one
    ``pow`` per ordered pair instead of two).  ``out`` = (identity, cov_query, is_null) arrays to fill."""
    lib = _capi.load_library()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    nq, ns = counts.shape
    q_sizes = np.ascontiguousarray(q_sizes, dtype=np.uint64)
    s_sizes = np.ascontiguousarray(s_sizes, dtype=np.uint64)
    if out is None:
        ident = np.empty((nq, ns), dtype=np.float64)
        cov = np.empty((nq, ns), dtype=np.float64)
        null = np.empty((nq, ns), dtype=np.uint8)
    else:
        ident, cov, null = out
        assert ident.shape == cov.shape == null.shape == (nq, ns) and ident.flags.c_contiguous and cov.flags.c_contiguous
    check(
        lib.pa_ani_host(
            counts.ctypes.data, q_sizes.ctypes.data, s_sizes.ctypes.data, nq, ns, k, ident.ctypes.data, cov.ctypes.data, null.ctypes.data,
            int(bool(symmetric)), int(threads),
        ),  # fmt: skip
        "pa_ani_host",
    )
    return ident, cov, null.view(np.bool_) if null.dtype == np.uint8 else null


# ------------------------------------------------------------------ search-run: the host form (no GPU needed)
def _hits_rank(rank) -> int:
    """``PA_HITS_RANK_*`` of a rank's name; an integer is handed to the library as it is (which refuses an unknown one)."""
    if isinstance(rank, (int, np.integer)) and not isinstance(rank, bool):
        return int(rank)
    if rank not in _capi.PA_HITS_RANK:
        raise ValueError(f"Unknown rank {rank!r}: expected one of {', '.join(_capi.PA_HITS_RANK)}")
    return _capi.PA_HITS_RANK[rank]


def _hit_sizes(sizes, what: str) -> np.ndarray:
    """Sketch sizes as contiguous uint32, each checked to be 1 to 2^32 - 1: the library's order needs both."""
    wide = np.asarray(sizes).astype(np.int64 if np.asarray(sizes).dtype.kind == "i" else np.uint64, copy=False).reshape(-1)
    if wide.size and (int(wide.min()) < 1 or int(wide.max()) >= 1 << 32):
        raise ValueError(f"{what}: sketch sizes must be 1 to 2^32 - 1, found {int(wide.min())} to {int(wide.max())}")
    return np.ascontiguousarray(wide, dtype=np.uint32)


def best_hits_host(counts, q_size, s_size, s_base: int, rank, top: int, state=None, *, ld: int | None = None, threads: int = 0):  # noqa: PLR0913
    """``pa_best_hits_host``: what ``HipEngine.best_hits_device`` returns, from numpy arrays into three nq x ``top``
    uint32 arrays, with the same bits.  ``counts`` is nq x ns, or -- with ``ld`` -- a flat array of rows ``ld`` apart.
    ``state``: the three arrays of an earlier call on other columns; they take part, are overwritten and returned."""
    lib = _capi.load_library()
    q = _hit_sizes(q_size, "query sizes")
    s = _hit_sizes(s_size, "subject sizes")
    nq, ns = len(q), len(s)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if ld is None:
        if counts.shape != (nq, ns):
            raise ValueError(f"counts of shape {counts.shape} for {nq} queries and {ns} subjects")
        ld = ns
    elif ld >= ns and counts.size < (nq - 1) * int(ld) + ns and nq:
        raise ValueError(f"{counts.size} counts for {nq} rows of {ns} columns, {ld} apart")
    if state is None:
        out = tuple(np.empty((nq, max(int(top), 1)), dtype=np.uint32) for _ in range(3))
    else:
        out = tuple(state)
        if len(out) != 3 or any(not isinstance(x, np.ndarray) or x.dtype != np.uint32 or x.shape != (nq, int(top)) or not x.flags.c_contiguous for x in out):  # noqa: PLR2004
            raise ValueError(f"state: expected three contiguous {nq} x {top} uint32 arrays")
    check(lib.pa_best_hits_host(counts.ctypes.data, nq, ns, int(ld), q.ctypes.data, s.ctypes.data, int(s_base), _hits_rank(rank), int(top),
                                int(state is not None), *(x.ctypes.data for x in out), int(threads)), "pa_best_hits_host")  # fmt: skip
    return out


# ------------------------------------------------------------------ TETRA-hip: the host forms (no GPU needed)
def _nj_outputs(n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    joins = max(n - 2, 0)
    return np.zeros((joins, 2), dtype=np.uint32), np.zeros((joins, 2), dtype=np.float64), np.zeros(2, dtype=np.uint32), np.zeros(1, dtype=np.float64)


def nj_tree_host(D, threads: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """``pa_nj_host``: what ``HipEngine.nj_tree`` returns, bit for bit, from plain loops on ``threads`` host threads (0: as
    many as the process may use); ``D`` is not modified."""
    d = np.ascontiguousarray(D, dtype=np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError(f"distance matrix of shape {d.shape}, expected a square one")
    n = d.shape[0]
    if n > 65535:
        raise ValueError(f"{n} nodes; at most 65535")
    out = _nj_outputs(n)
    check(_capi.load_library().pa_nj_host(d.ctypes.data, n, *(a.ctypes.data for a in out), int(threads)), "pa_nj_host")
    return out[0], out[1], out[2], float(out[3][0])


# ------------------------------------------------------------------ mantel-run-comp: the host forms (no GPU needed)
def _mantel_arguments(x_shape, y_shape, perms) -> tuple[int, np.ndarray]:
    """``(n, the permutations as a contiguous uint32 P x n array)``; the library checks n and the rows themselves."""
    n = int(x_shape[0])
    if tuple(y_shape) != tuple(x_shape):
        raise ValueError(f"distance matrices of shapes {tuple(x_shape)} and {tuple(y_shape)}, expected the same")
    p = np.ascontiguousarray(perms, dtype=np.uint32)
    if p.size == 0:
        p = p.reshape(0, n)
    if p.ndim != 2 or p.shape[1] != n:
        raise ValueError(f"permutations of shape {p.shape} for {n} genomes, expected (P, {n})")
    return n, p


def _mantel_outputs(n_perms: int) -> tuple[np.ndarray, np.ndarray]:
    return np.zeros(4, dtype=np.float64), np.zeros(n_perms + 1, dtype=np.float64)


def mantel_host(X, Y, perms, threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``pa_mantel_host``: what ``HipEngine.mantel`` returns, bit for bit, on ``threads`` host threads (0: as many as the
    process may use), whose number does not show in the result.  ``X`` and ``Y`` are not modified."""
    x = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(Y, dtype=np.float64)
    for m in (x, y):
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError(f"distance matrix of shape {m.shape}, expected a square one")
    n, p = _mantel_arguments(x.shape, y.shape, perms)
    out = _mantel_outputs(len(p))
    check(_capi.load_library().pa_mantel_host(x.ctypes.data, y.ctypes.data, n, p.ctypes.data, len(p), *(a.ctypes.data for a in out), int(threads)),
          "pa_mantel_host")
    return out


def mantel_permutations(seed: int, n: int, first: int, count: int) -> np.ndarray:
    """``pa_mantel_permutations``: rows ``first .. first + count - 1`` of the permutations of ``seed`` over ``n`` genomes
    (uint32, count x n).  A row depends on (seed, n, its number) alone."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed {seed!r}; 0 to 2^64 - 1")
    out = np.empty((int(count), int(n)), dtype=np.uint32)
    check(_capi.load_library().pa_mantel_permutations(int(seed), int(n), int(first), int(count), out.ctypes.data), "pa_mantel_permutations")
    return out


# ------------------------------------------------------------------ bootstrap-run: the host forms (no GPU needed)
def _boot_weights(weights, n_cols: int) -> np.ndarray:
    """The weights as a contiguous uint8 R x ``n_cols`` array; the library checks the rows' sums."""
    w = np.ascontiguousarray(weights, dtype=np.uint8)
    if w.ndim != 2 or w.shape[1] != int(n_cols):
        raise ValueError(f"weights of shape {w.shape} for {n_cols} columns, expected (R, {n_cols})")
    return w


def msa_boot_weights(seed: int, n_cols: int, first: int, count: int, *, lib=None) -> np.ndarray:
    """``pa_msa_boot_weights``: rows ``first .. first + count - 1`` of the bootstrap weights of ``seed`` over ``n_cols``
    columns (uint8, count x n_cols): how often each column is drawn among ``n_cols`` draws.  A row depends on (seed,
    n_cols, its number) alone."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"seed {seed!r}; 0 to 2^64 - 1")
    out = np.empty((int(count), int(n_cols)), dtype=np.uint8)
    lib = lib or _capi.load_library()
    check(lib.pa_msa_boot_weights(int(seed), int(n_cols), int(first), int(count), out.ctypes.data), "pa_msa_boot_weights", lib)
    return out


def msa_boot_counts_host(rows, n_cols: int, weights, threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``pa_msa_boot_counts_host``: what ``HipEngine.msa_boot_counts`` returns (uint32 ``[R, n, n]``) from the rows as
    bytes (``LoadedMSA.rows``: uint8, n x stride with stride >= ``n_cols``)."""
    r = np.ascontiguousarray(rows, dtype=np.uint8)
    if r.ndim != 2 or r.shape[1] < int(n_cols):
        raise ValueError(f"rows of shape {r.shape} for {n_cols} columns")
    w = _boot_weights(weights, n_cols)
    n = r.shape[0]
    match, both = np.zeros((len(w), n, n), dtype=np.uint32), np.zeros((len(w), n, n), dtype=np.uint32)
    check(
        _capi.load_library().pa_msa_boot_counts_host(r.ctypes.data, r.shape[1], n, int(n_cols), w.ctypes.data, len(w), match.ctypes.data, both.ctypes.data,
                                                     int(threads)),
        "pa_msa_boot_counts_host",
    )  # fmt: skip
    return match, both


def msa_boot_distances_host(match, both, missing: float = 1.0, threads: int = 0) -> np.ndarray:
    """``pa_msa_boot_distances_host``: what ``HipEngine.msa_boot_distances`` returns, bit for bit (float64 ``[R, n, n]``)."""
    m = np.ascontiguousarray(match, dtype=np.uint32)
    b = np.ascontiguousarray(both, dtype=np.uint32)
    if m.ndim != 3 or m.shape[1] != m.shape[2] or b.shape != m.shape:
        raise ValueError(f"counts of shapes {m.shape} and {b.shape}, expected the same (R, n, n)")
    d = np.zeros(m.shape, dtype=np.float64)
    check(_capi.load_library().pa_msa_boot_distances_host(m.ctypes.data, b.ctypes.data, m.shape[1], m.shape[0], float(missing), d.ctypes.data, int(threads)),
          "pa_msa_boot_distances_host")
    return d


def tree_support(n: int, ref_child, rep_child) -> np.ndarray:
    """``pa_tree_support``: per node ``n + t`` of the reference join table ``ref_child`` ((n - 2) x 2 uint32) the number of
    the replicate tables ``rep_child`` (R x (n - 2) x 2) that have the edge above it."""
    ref = np.ascontiguousarray(ref_child, dtype=np.uint32)
    rep = np.ascontiguousarray(rep_child, dtype=np.uint32)
    joins = max(int(n) - 2, 0)
    if ref.shape != (joins, 2) or rep.ndim != 3 or rep.shape[1:] != (joins, 2):
        raise ValueError(f"join tables of shapes {ref.shape} and {rep.shape} for {n} leaves")
    out = np.zeros(joins, dtype=np.uint32)
    check(_capi.load_library().pa_tree_support(int(n), ref.ctypes.data, len(rep), rep.ctypes.data, out.ctypes.data), "pa_tree_support")
    return out


# ------------------------------------------------------------------ phylo-run: the host forms (no GPU needed)
SUBST_MODELS = {"p": _capi.PA_SUBST_MODEL_P, "jc69": _capi.PA_SUBST_MODEL_JC69, "k80": _capi.PA_SUBST_MODEL_K80}


def _subst_model(model: str) -> int:
    if model not in SUBST_MODELS:
        raise ValueError(f"unknown substitution model {model!r}: expected one of {', '.join(SUBST_MODELS)}")
    return SUBST_MODELS[model]


def subst_code_table() -> np.ndarray:
    """``pa_subst_code``: byte -> nucleotide code (A 4, G 5, C 6, T and U 7, either case; every other byte 0), uint8[256]."""
    code = np.zeros(256, dtype=np.uint8)
    check(_capi.load_library().pa_subst_code(code.ctypes.data), "pa_subst_code")
    return code


def subst_log_host(x) -> np.ndarray:
    """``pa_subst_log_host``: the rule's own natural logarithm of every element."""
    v = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.empty_like(v)
    check(_capi.load_library().pa_subst_log_host(v.ctypes.data, v.size, out.ctypes.data), "pa_subst_log_host")
    return out


def msa_subst_counts_host(rows, n_cols: int, weights=None, threads: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``pa_msa_subst_counts_host``: what ``HipEngine.msa_subst_counts`` returns (uint32 ``[R, n, n]`` each) from the rows
    as bytes (uint8, n x stride with stride >= ``n_cols``)."""
    r = np.ascontiguousarray(rows, dtype=np.uint8)
    if r.ndim != 2 or r.shape[1] < int(n_cols):
        raise ValueError(f"rows of shape {r.shape} for {n_cols} columns")
    w = None if weights is None else _boot_weights(weights, n_cols)
    reps, n = 1 if w is None else len(w), r.shape[0]
    out = tuple(np.zeros((reps, n, n), dtype=np.uint32) for _ in range(3))
    check(
        _capi.load_library().pa_msa_subst_counts_host(r.ctypes.data, r.shape[1], n, int(n_cols), None if w is None else w.ctypes.data, reps,
                                                      *(x.ctypes.data for x in out), int(threads)),
        "pa_msa_subst_counts_host",
    )  # fmt: skip
    return out


def subst_distances_host(valid, ts, tv, model: str = "k80", missing: float = 3.0, threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``pa_subst_distances_host``: what ``HipEngine.subst_distances`` returns, bit for bit (float64 ``[R, n, n]``, uint64 ``[R, 2]``)."""
    v, s, t = (np.ascontiguousarray(x, dtype=np.uint32) for x in (valid, ts, tv))
    if v.ndim != 3 or v.shape[1] != v.shape[2] or s.shape != v.shape or t.shape != v.shape:
        raise ValueError(f"counts of shapes {v.shape}, {s.shape} and {t.shape}, expected the same (R, n, n)")
    d = np.zeros(v.shape, dtype=np.float64)
    undefined = np.zeros((v.shape[0], 2), dtype=np.uint64)
    check(
        _capi.load_library().pa_subst_distances_host(v.ctypes.data, s.ctypes.data, t.ctypes.data, v.shape[1], v.shape[0], _subst_model(model), float(missing),
                                                     d.ctypes.data, undefined.ctypes.data, int(threads)),
        "pa_subst_distances_host",
    )  # fmt: skip
    return d, undefined


# ------------------------------------------------------------------ dereplicate-run: the host forms (no GPU needed)
class Dereplication(NamedTuple):
    """``is_rep[p]``: node p is a representative; ``rep[p]`` the representative of p (itself for a representative;
    uint32); ``rep_score[p]`` the score of the pair (p, rep[p]); ``n_reps`` their number; ``rounds`` the rounds the device
    took (None on the host: a diagnostic, not a result)."""

    is_rep: np.ndarray
    rep: np.ndarray
    rep_score: np.ndarray
    n_reps: int
    rounds: int | None


def _pair_agg(name: str, role: str) -> int:
    if name not in _capi.PA_AGG:
        raise ValueError(f"Unknown {role} aggregator {name!r}: expected one of min, max, mean")
    return _capi.PA_AGG[name]


def _derep_mode(name: str) -> int:
    if name not in _capi.PA_DEREP_MODE:
        raise ValueError(f"Unknown dereplication mode {name!r}: expected one of greedy, cover")
    return _capi.PA_DEREP_MODE[name]


def _derep_same_shape(score_shape, cov_shape) -> None:
    if tuple(score_shape) != tuple(cov_shape):
        raise ValueError(f"score and coverage matrices of shapes {tuple(score_shape)} and {tuple(cov_shape)}, expected the same")


def derep_adjacency_host(score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", min_score: float = 0.95, cov_min: float = 0.5,  # noqa: PLR0913
                         threads: int = 0) -> np.ndarray:
    """``pa_derep_adjacency_host``: what ``HipEngine.derep_adjacency_device`` computes, bit for bit, as an n x ceil(n / 64)
    uint64 array."""
    s, c = _square_f64(score, "score matrix"), _square_f64(cov, "coverage matrix")
    _derep_same_shape(s.shape, c.shape)
    n = s.shape[0]
    bits = np.zeros((n, (n + 63) // 64), dtype=np.uint64)
    check(
        _capi.load_library().pa_derep_adjacency_host(s.ctypes.data, c.ctypes.data, n, _pair_agg(score_edges, "score"), _pair_agg(coverage_edges, "coverage"),
                                                     float(min_score), float(cov_min), bits.ctypes.data, int(threads)),
        "pa_derep_adjacency_host",
    )  # fmt: skip
    return bits


def derep_select_host(bits, n: int, mode: str = "greedy") -> tuple[np.ndarray, int]:
    """``pa_derep_select_host``: ``(is_rep as n uint8, n_reps)`` of the bit matrix, by the sequential rules."""
    n = int(n)
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    if b.size != n * ((n + 63) // 64):
        raise ValueError(f"bit matrix of {b.size} words for {n} nodes, expected {n} x {(n + 63) // 64}")
    is_rep = np.zeros(max(n, 1), dtype=np.uint8)
    n_reps = C.c_uint32(0)
    check(_capi.load_library().pa_derep_select_host(b.ctypes.data, n, _derep_mode(mode), is_rep.ctypes.data, C.byref(n_reps)), "pa_derep_select_host")
    return is_rep[:n], n_reps.value


def derep_assign_host(score, bits, is_rep, *, score_edges: str = "mean", threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``pa_derep_assign_host``: ``(rep as uint32, rep_score)``, what ``HipEngine.derep_assign_device`` computes, bit for bit."""
    s = _square_f64(score, "score matrix")
    n = s.shape[0]
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    r = np.ascontiguousarray(is_rep, dtype=np.uint8)
    if b.size != n * ((n + 63) // 64) or r.size != n:
        raise ValueError(f"bit matrix of {b.size} words and {r.size} marks for {n} nodes")
    rep, rep_score = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.float64)
    check(_capi.load_library().pa_derep_assign_host(s.ctypes.data, n, _pair_agg(score_edges, "score"), b.ctypes.data, r.ctypes.data, rep.ctypes.data,
                                                    rep_score.ctypes.data, int(threads)), "pa_derep_assign_host")  # fmt: skip
    return rep[:n], rep_score[:n]


def dereplicate_host(score, cov, *, score_edges: str = "mean", coverage_edges: str = "min", min_score: float = 0.95, cov_min: float = 0.5,  # noqa: PLR0913
                     mode: str = "greedy", threads: int = 0) -> Dereplication:
    """What ``HipEngine.dereplicate`` returns, bit for bit, from the three host twins on ``threads`` host threads (0: as
    many as the process may use), whose number does not show in the result.  The inputs are not modified."""
    _derep_mode(mode)
    bits = derep_adjacency_host(score, cov, score_edges=score_edges, coverage_edges=coverage_edges, min_score=min_score, cov_min=cov_min, threads=threads)
    is_rep, n_reps = derep_select_host(bits, len(bits), mode)
    rep, rep_score = derep_assign_host(score, bits, is_rep, score_edges=score_edges, threads=threads)
    return Dereplication(is_rep.astype(bool), rep, rep_score, n_reps, None)


# ------------------------------------------------------------------ ordinate-run: the host forms (no GPU needed)
def _square_f64(M, what: str) -> np.ndarray:
    m = np.ascontiguousarray(M, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"{what} of shape {m.shape}, expected a square one")
    if m.shape[0] > 65535:
        raise ValueError(f"{m.shape[0]} rows; at most 65535")
    return m


def _eigs_outputs(n: int, k: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    k = max(int(k), 0)
    return np.zeros(k, dtype=np.float64), np.zeros((n, k), dtype=np.float64), np.zeros(k, dtype=np.float64), np.zeros(3, dtype=np.float64)


def _eigs_result(out) -> tuple[np.ndarray, np.ndarray, np.ndarray, tuple[int, int, float]]:
    return out[0], out[1], out[2], (int(out[3][0]), int(out[3][1]), float(out[3][2]))


def mul_tall_host(A, Q, threads: int = 0) -> np.ndarray:
    """``pa_mul_tall_f64_host``: what ``HipEngine.mul_tall`` returns, bit for bit, on ``threads`` host threads (0: as many
    as the process may use), whose number does not show in the result."""
    a = _square_f64(A, "matrix")
    q = np.ascontiguousarray(Q, dtype=np.float64)
    if q.ndim != 2 or q.shape[0] != a.shape[0]:
        raise ValueError(f"block of shape {q.shape} for a matrix of {a.shape[0]} rows")
    y = np.empty_like(q)
    check(_capi.load_library().pa_mul_tall_f64_host(a.ctypes.data, a.shape[0], q.ctypes.data, q.shape[1], y.ctypes.data, int(threads)),
          "pa_mul_tall_f64_host")
    return y


def gower_center_host(D, threads: int = 0) -> tuple[np.ndarray, float, float]:
    """``pa_gower_center_host``: what ``HipEngine.gower_center`` returns, bit for bit."""
    d = _square_f64(D, "distance matrix")
    b = np.empty_like(d)
    trace, fro2 = C.c_double(0.0), C.c_double(0.0)
    check(_capi.load_library().pa_gower_center_host(d.ctypes.data, d.shape[0], b.ctypes.data, C.byref(trace), C.byref(fro2), int(threads)),
          "pa_gower_center_host")
    return b, trace.value, fro2.value


def symm_top_eigs_host(B, k: int, fro2: float, tol: float = 1e-10, max_iter: int = 10000, threads: int = 0):
    """``pa_symm_top_eigs_host``: what ``HipEngine.symm_top_eigs`` returns, bit for bit; the products run on ``threads``
    host threads."""
    b = _square_f64(B, "matrix")
    n = b.shape[0]
    out = _eigs_outputs(n, k)
    check(
        _capi.load_library().pa_symm_top_eigs_host(b.ctypes.data, n, int(k), float(tol), int(max_iter), float(fro2),
                                                   *(a.ctypes.data for a in out), int(threads)),
        "pa_symm_top_eigs_host",
    )
    return _eigs_result(out)


def tetra_counts_host(arena: HostArena, threads: int = 0) -> np.ndarray:
    """``pa_tetra_counts_host``: what ``HipEngine.tetra_counts`` returns, from a host arena on host threads."""
    n = arena.n_genomes
    counts = np.zeros((n, _capi.PA_TETRA_BINS), dtype=np.uint64)
    packed = np.ascontiguousarray(arena.packed, dtype=np.uint32)
    mask = np.ascontiguousarray(arena.mask, dtype=np.uint32)
    gs = np.ascontiguousarray(arena.genome_start, dtype=np.uint64)
    check(
        _capi.load_library().pa_tetra_counts_host(packed.ctypes.data, mask.ctypes.data, arena.arena_bases, gs.ctypes.data, n, counts.ctypes.data,
                                                  int(threads)),
        "pa_tetra_counts_host",
    )  # fmt: skip
    return counts


def tetra_zscores(counts) -> tuple[np.ndarray, np.ndarray]:
    """``pa_tetra_zscores_host``: ``(Z, U)``, the tetranucleotide Z-scores and their unit rows (``[n, 256]`` float64 each;
    a degenerate genome's U is all NaN) from the forward counts ``[n, 336]``.  Host only: 256 values per genome."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    if counts.ndim != 2 or counts.shape[1] != _capi.PA_TETRA_BINS:
        raise ValueError(f"counts have shape {counts.shape}, expected (n, {_capi.PA_TETRA_BINS})")
    n = counts.shape[0]
    z = np.zeros((n, _capi.PA_TETRA_WORDS), dtype=np.float64)
    u = np.zeros((n, _capi.PA_TETRA_WORDS), dtype=np.float64)
    check(_capi.load_library().pa_tetra_zscores_host(counts.ctypes.data, n, z.ctypes.data, u.ctypes.data), "pa_tetra_zscores_host")
    return z, u


def tetra_correlations_host(U, q_range=None, s_range=None, threads: int = 0) -> np.ndarray:
    """``pa_tetra_corr_host``: what ``HipEngine.tetra_correlations`` returns, the same bits, on host threads."""
    u = np.ascontiguousarray(U, dtype=np.float64)
    if u.ndim != 2 or u.shape[1] != _capi.PA_TETRA_WORDS:
        raise ValueError(f"U has shape {u.shape}, expected (n, {_capi.PA_TETRA_WORDS})")
    n = u.shape[0]
    q0, q1, s0, s1 = _pair_ranges(n, q_range, s_range, tetra=True)
    out = np.empty((q1 - q0, s1 - s0), dtype=np.float64)
    check(
        _capi.load_library().pa_tetra_corr_host(u.ctypes.data, n, q0, q1, s0, s1, int((q0, q1) == (s0, s1)), out.ctypes.data, int(threads)),
        "pa_tetra_corr_host",
    )
    return out


# ------------------------------------------------------------------ external alignment (external-alignment-hip)
GAP = ord("-")


@dataclass
class LoadedMSA:
    """A FASTA multiple alignment read by ``pa_msa_load``: md5 of the raw file, one title and residue count per record,
    a 256-bin histogram of the residue bytes, and the rows as an N x ``row_stride`` byte matrix (each row's tail after
    its residues is '-'; ``row_stride`` = the longest row rounded up to 32)."""

    md5: str
    titles: list[bytes]
    lengths: np.ndarray  # uint64 residues (gaps included) per record
    histogram: np.ndarray  # uint64[256]
    rows: np.ndarray  # uint8 [N, row_stride]
    n_cols: int  # longest record

    @property
    def n_rows(self) -> int:
        return len(self.titles)


def load_msa(path, threads: int = 0) -> LoadedMSA:
    """One pass over the alignment file: md5 beside a parallel parse (``pa_msa_load``), then the rows copied out."""
    lib = _capi.load_library()
    handle = C.c_void_p()
    check(lib.pa_msa_load(str(path).encode(), int(threads), C.byref(handle)), "pa_msa_load", lib)
    try:
        n = C.c_uint32(0)
        max_len = C.c_uint64(0)
        md5 = C.create_string_buffer(33)
        hist = np.zeros(256, dtype=np.uint64)
        check(lib.pa_msa_info(handle, C.byref(n), C.byref(max_len), md5, hist.ctypes.data_as(C.POINTER(C.c_uint64))), "pa_msa_info", lib)
        titles, lengths = [], np.zeros(n.value, dtype=np.uint64)
        title, tlen, length = C.c_char_p(), C.c_uint64(0), C.c_uint64(0)
        for i in range(n.value):
            check(lib.pa_msa_record(handle, i, C.byref(title), C.byref(tlen), C.byref(length)), "pa_msa_record", lib)
            titles.append(C.string_at(title, tlen.value))
            lengths[i] = length.value
        stride = max(32, (int(max_len.value) + 31) // 32 * 32)
        rows = np.empty((n.value, stride), dtype=np.uint8)
        if n.value:
            check(lib.pa_msa_copy_rows(handle, 0, n.value, stride, rows.ctypes.data), "pa_msa_copy_rows", lib)
        return LoadedMSA(md5.value.decode(), titles, lengths, hist, rows, int(max_len.value))
    finally:
        lib.pa_msa_free(handle)


def msa_code_table(histogram) -> tuple[np.ndarray, int]:
    """Byte -> code for the pack kernel: '-' 0, the residue bytes present 1..A in byte order; bits = ceil(log2(A + 1))
    (at least 1).  Comparison is on raw bytes: 'a' and 'A' are different residues, '.' is a residue."""
    hist = np.asarray(histogram, dtype=np.uint64)
    present = [b for b in range(256) if hist[b] and b != GAP]
    code = np.zeros(256, dtype=np.uint8)
    for i, b in enumerate(present, start=1):
        code[b] = i
    bits = max(1, int(len(present)).bit_length())
    return code, bits


@dataclass
class DeviceMSA:
    planes: object  # torch.int32 [pa_msa_plane_words] on the device
    nongap: object  # torch.int32 [n_rows]: residues (non-gap columns) per row
    n_rows: int
    n_cols: int
    bits: int


def msa_metrics(match, both, n_q, n_s, threads: int = 0):
    """(M, B, n_q, n_s) per pair -> (identity, aln_length, sim_errors, cov_query, cov_subject), ``pa_msa_metrics`` on the
    host thread pool; bit-identical to the reference's int / int divisions."""
    lib = _capi.load_library()
    match = np.ascontiguousarray(match, dtype=np.uint32)
    shape = match.shape  # n_q / n_s broadcast against it (a column of query lengths, a row of subject lengths)
    match = match.ravel()
    both = np.ascontiguousarray(both, dtype=np.uint32).ravel()
    n_q = np.ascontiguousarray(np.broadcast_to(np.asarray(n_q, dtype=np.uint64), shape)).ravel()
    n_s = np.ascontiguousarray(np.broadcast_to(np.asarray(n_s, dtype=np.uint64), shape)).ravel()
    n = match.size
    assert both.size == n
    ident, covq, covs = (np.empty(n, dtype=np.float64) for _ in range(3))
    aln, err = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    check(
        lib.pa_msa_metrics(
            match.ctypes.data, both.ctypes.data, n_q.ctypes.data, n_s.ctypes.data, n, ident.ctypes.data, aln.ctypes.data,
            err.ctypes.data, covq.ctypes.data, covs.ctypes.data, int(threads),
        ),  # fmt: skip
        "pa_msa_metrics",
        lib,
    )
    return ident, aln, err, covq, covs
