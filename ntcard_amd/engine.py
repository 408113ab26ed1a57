"""Python mirror of the reference seam over the C ABI (ctypes); torch is plumbing only
(device memory, streams, torch.distributed for the multi-GPU sketch merge).

Names follow the reference: an `Engine` owns t_Counter and F1 (ntcard.cpp:433-439), `submit*`
is a batch of ntRead/stRead calls (ntcard.cpp:147-171), `finish` returns what compEst consumes
(ntcard.cpp:237-247), `estimate` is compEst's recurrence (ntcard.cpp:249-274) and `write_hist`
is outDefault's body (ntcard.cpp:291-294).
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import NtcConfig, NtcError, check

FLAG_SIMPLE_KERNEL = 1  # NTC_FLAG_SIMPLE_KERNEL: run the simple validation kernel
FLAG_LANE_KERNEL = 32  # NTC_FLAG_LANE_KERNEL: the lane-per-read kernel K1 takes every batch (tiled ones are re-laid out as row slots)
FLAG_ALWAYS_LOG = 8  # NTC_FLAG_ALWAYS_LOG: never switch from the hit log to direct atomics
FLAG_PARTITION_ALWAYS = 16  # NTC_FLAG_PARTITION_ALWAYS: small logs go through the partition passes too (validation)
FLAG_DEFER_REDO = 128  # NTC_FLAG_DEFER_REDO: submit_device buffers stay unchanged until sync(); the handed-back reads of several batches share one pass
FLAG_REQUIRE_TILED = 64  # NTC_FLAG_REQUIRE_TILED: submit_tiled_device fails instead of falling back to the general kernel
FLAG_DIRECT_ATOMICS = 2  # NTC_FLAG_DIRECT_ATOMICS: no hit log, one device atomic per sampled k-mer
FLAG_STRAND_FORWARD = 512  # NTC_FLAG_STRAND_FORWARD: count the forward value fh of every window instead of the canonical min(fh, rh)
FLAG_STRAND_REVERSE = 1024  # NTC_FLAG_STRAND_REVERSE: count the reverse value rh (the forward value of the window's reverse complement)
FLAG_STRAND_TILED = 4096  # NTC_FLAG_STRAND_TILED: a one-strand engine whose planes are all the tiled kernels' counts on the one-strand K1h + K1f instead of K1
FLAG_HPC = 8192  # NTC_FLAG_HPC: homopolymer-compressed counting — every run of one base is collapsed to its first byte before the windows are taken
FLAG_SIGNATURE = 16384  # NTC_FLAG_SIGNATURE: keep every sampled 64-bit value with its exact count, per plane (Engine.signature)
_STRAND_FLAGS = {"canonical": 0, "forward": FLAG_STRAND_FORWARD, "reverse": FLAG_STRAND_REVERSE}
SIZE_RULE_BYTES = 50_000_000_000  # ntcard.cpp:430: total input < 50 GB => sBits = 7


def s_bits_for_input(total_bytes, requested=11):
    """The reference's size rule (ntcard.cpp:427-431); the caller applies it before Engine()."""
    return 7 if total_bytes < SIZE_RULE_BYTES else requested


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _strand_flags(flags, strand, strand_tiled=False):
    """`flags` with the bit of the `strand` keyword ORed in (None: whatever `flags` says), and FLAG_STRAND_TILED if `strand_tiled`; checked before the
    library is asked for a device"""
    flags = int(flags)
    if strand_tiled:
        if not (strand in ("forward", "reverse") or (strand is None and flags & (FLAG_STRAND_FORWARD | FLAG_STRAND_REVERSE))):
            raise ValueError("strand_tiled=True picks the kernels of a one-strand engine: it needs strand='forward' or 'reverse'")
        flags |= FLAG_STRAND_TILED
    if strand is None:
        return flags
    if not isinstance(strand, str) or strand not in _STRAND_FLAGS:
        raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
    given = flags & (FLAG_STRAND_FORWARD | FLAG_STRAND_REVERSE)
    if given and given != _STRAND_FLAGS[strand]:
        raise ValueError(f"strand={strand!r} contradicts the strand bits 0x{given:x} passed in flags")
    return flags | _STRAND_FLAGS[strand]


class Engine:
    def __init__(self, klist, gap=0, r_bits=27, s_bits=7, device=0, stream=None, ext_sketch=None, ext_f1=None, flags=0, log_entries=0, strand=None,
                 strand_tiled=False, hpc=False, signature=False):
        """strand: "canonical" (the default, what ntcard counts), "forward" or "reverse" — which value of a window is counted
        (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE).  strand_tiled: a one-strand engine whose planes are all the tiled kernels' (plain
        k = 12 .. 32, the two tiled gap seeds, sBits >= 7) counts on the one-strand K1h + K1f instead of the general kernel (NTC_FLAG_STRAND_TILED;
        the results are the same).  hpc: count homopolymer-compressed sequences (NTC_FLAG_HPC: submit / submit_spans compress on the host,
        submit_long_device on the device; the fixed-layout device batches are refused).  signature: keep every sampled 64-bit value with its exact count
        (NTC_FLAG_SIGNATURE: signature(), signature_inject(), signature_stats(); every plane is then the general kernel's)"""
        flags = _strand_flags(flags, strand, strand_tiled) | (FLAG_HPC if hpc else 0) | (FLAG_SIGNATURE if signature else 0)
        self._lib = _abi.lib()
        self.klist = [int(k) for k in klist]
        self.gap, self.r_bits, self.s_bits, self.device = int(gap), int(r_bits), int(s_bits), int(device)
        self._karr = (C.c_uint32 * len(self.klist))(*self.klist)
        cfg = NtcConfig()
        cfg.n_k = len(self.klist)
        cfg.k = C.cast(self._karr, C.POINTER(C.c_uint32))
        cfg.gap, cfg.r_bits, cfg.s_bits, cfg.device = self.gap, self.r_bits, self.s_bits, self.device
        cfg.stream = C.c_void_p(stream) if stream else None
        self._keep = (ext_sketch, ext_f1)  # keep torch tensors alive
        cfg.ext_sketch = C.c_void_p(ext_sketch.data_ptr()) if ext_sketch is not None else None
        cfg.ext_f1 = C.c_void_p(ext_f1.data_ptr()) if ext_f1 is not None else None
        cfg.flags = int(flags)
        cfg.log_entries = int(log_entries)
        h = C.c_void_p()
        check(self._lib.ntc_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.seeds = None

    @classmethod
    def from_seeds(cls, seeds, r_bits=27, s_bits=7, device=0, stream=None, ext_sketch=None, ext_f1=None, flags=0, log_entries=0, strand=None,
                   strand_tiled=False, hpc=False, signature=False):
        """an engine whose planes are spaced seeds given as masks of '0' / '1' (include/ntcard_hip.h: ntc_create_seeded); its klist is
        the masks' lengths, so finish, merge_counters and the rest work as for a k list; strand, strand_tiled, hpc and signature as for Engine()"""
        flags = _strand_flags(flags, strand, strand_tiled) | (FLAG_HPC if hpc else 0) | (FLAG_SIGNATURE if signature else 0)
        self = cls.__new__(cls)
        self._lib = _abi.lib()
        self.seeds = [s.decode() if isinstance(s, bytes) else str(s) for s in seeds]
        self.klist = [len(s) for s in self.seeds]
        self.gap, self.r_bits, self.s_bits, self.device = 0, int(r_bits), int(s_bits), int(device)
        cfg = NtcConfig()
        cfg.n_k, cfg.k, cfg.gap = 0, None, 0
        cfg.r_bits, cfg.s_bits, cfg.device = self.r_bits, self.s_bits, self.device
        cfg.stream = C.c_void_p(stream) if stream else None
        self._keep = (ext_sketch, ext_f1)
        cfg.ext_sketch = C.c_void_p(ext_sketch.data_ptr()) if ext_sketch is not None else None
        cfg.ext_f1 = C.c_void_p(ext_f1.data_ptr()) if ext_f1 is not None else None
        cfg.flags = int(flags)
        cfg.log_entries = int(log_entries)
        self._sarr = (C.c_char_p * len(self.seeds))(*[s.encode() for s in self.seeds])
        h = C.c_void_p()
        self._h = None
        check(self._lib.ntc_create_seeded(C.byref(cfg), len(self.seeds), self._sarr, C.byref(h)))
        self._h = h
        return self

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.ntc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        check(self._lib.ntc_reset(self._h))

    # -- the seam ----------------------------------------------------------------------------
    def submit(self, bases, offsets):
        """bases: uint8 array / bytes of concatenated reads; offsets: uint64[n+1]."""
        b = np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        if b.size == 0:
            b = np.zeros(1, dtype=np.uint8)
        check(self._lib.ntc_submit(self._h, _np_ptr(b), _np_ptr(o), len(o) - 1))

    def submit_spans(self, buf, starts, lens):
        """reads as spans of one host buffer: read i = buf[starts[i] : starts[i] + lens[i]]"""
        b = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf, dtype=np.uint8)
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        assert len(st) == len(ln)
        check(self._lib.ntc_submit_spans(self._h, _np_ptr(b), _np_ptr(st), _np_ptr(ln), len(st)))

    def submit_reads(self, reads):
        offs = np.zeros(len(reads) + 1, dtype=np.uint64)
        if reads:
            offs[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
        self.submit(b"".join(reads), offs)

    def submit_device(self, d_slots_ptr, n_reads, read_len, stride):
        check(self._lib.ntc_submit_device(self._h, C.c_void_p(d_slots_ptr), n_reads, read_len, stride))

    def submit_tiled_device(self, d_tiles_ptr, n_reads, read_len):
        """a device-resident batch in the tiled layout (include/ntcard_hip.h: ntc_submit_tiled_device)"""
        check(self._lib.ntc_submit_tiled_device(self._h, C.c_void_p(d_tiles_ptr), n_reads, read_len))

    def submit_tiled_ragged_device(self, d_tiles_ptr, n_reads, n_chunks, d_tails_ptr):
        """a device-resident RAGGED batch: reads of 16 n_chunks - 15 .. 16 n_chunks bases in the tiled layout, every tile sorted longest first,
        d_tails = uint32[n_tiles][16] (include/ntcard_hip.h: ntc_submit_tiled_ragged_device; tile_reads_ragged builds both)"""
        check(self._lib.ntc_submit_tiled_ragged_device(self._h, C.c_void_p(d_tiles_ptr), n_reads, n_chunks, C.c_void_p(d_tails_ptr)))

    def submit_tiled_bins_device(self, bins):
        """several device-resident tiled batches in one call (include/ntcard_hip.h: ntc_submit_tiled_bins_device); bins: (d_tiles_ptr, n_reads, read_len,
        d_tails_ptr or 0) — d_tails_ptr = 0: an equal-length batch, else a ragged one with read_len = 16 x its chunks"""
        n = len(bins)
        tiles = (C.c_void_p * n)(*[b[0] for b in bins])
        nr = (C.c_uint64 * n)(*[b[1] for b in bins])
        rl = (C.c_uint32 * n)(*[b[2] for b in bins])
        tails = (C.c_void_p * n)(*[(b[3] or None) for b in bins])
        check(self._lib.ntc_submit_tiled_bins_device(self._h, n, tiles, nr, rl, tails))

    def submit_long_device(self, d_ptr, offsets, piece_len=0):
        """device-resident long sequences: sequence i = the bytes [offsets[i], offsets[i + 1]) from d_ptr (device memory, raw bytes of any alignment);
        offsets: host uint64[n + 1]; piece_len: 0 or a multiple of 16 from kmax + 15 on.  An engine whose planes are all the tiled kernels' — one plane, or a
        list of plain k with kmax - kmin <= 15 — cuts every sequence ONCE, as long_plan(kmax, piece_len, n) says, and counts every k from the same tiles; a
        remainder is counted iff it holds a window of kmin; the host sends 16 B per sequence, not per piece.  Every other engine gathers the sequences
        whole (long_stats stays (0, 0); FLAG_REQUIRE_TILED refuses).  include/ntcard_hip.h: ntc_submit_long_device"""
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(self._lib.ntc_submit_long_device(self._h, C.c_void_p(d_ptr) if d_ptr else None, _np_ptr(o), max(len(o) - 1, 0), int(piece_len)))

    def long_stats(self):
        """-> (full pieces cut for the tiled kernels, sequences that contributed one) since create / reset (ntc_long_stats)"""
        pieces, seqs = C.c_uint64(), C.c_uint64()
        check(self._lib.ntc_long_stats(self._h, C.byref(pieces), C.byref(seqs)))
        return pieces.value, seqs.value

    def long_time(self):
        """-> (cut ms, gather ms) of submit_long_device's re-layout kernels while profiling (ntc_long_time)"""
        cut, gather = C.c_double(), C.c_double()
        check(self._lib.ntc_long_time(self._h, C.byref(cut), C.byref(gather)))
        return cut.value, gather.value

    def hpc_stats(self):
        """-> (sequence bytes given, bytes kept) by homopolymer compression since create / reset; (0, 0) on an engine without hpc=True (ntc_hpc_stats)"""
        b_in, b_out = C.c_uint64(), C.c_uint64()
        check(self._lib.ntc_hpc_stats(self._h, C.byref(b_in), C.byref(b_out)))
        return b_in.value, b_out.value

    def hpc_time(self):
        """-> ms of submit_long_device's compaction kernels while profiling (ntc_hpc_time)"""
        ms = C.c_double()
        check(self._lib.ntc_hpc_time(self._h, C.byref(ms)))
        return ms.value

    # -- signatures (NTC_FLAG_SIGNATURE) -------------------------------------------------------
    def signature_size(self, plane=0):
        """the distinct sampled values of a plane; brings pending work in (ntc_signature_size)"""
        n = C.c_uint64()
        check(self._lib.ntc_signature_size(self._h, int(plane), C.byref(n)))
        return n.value

    def signature(self, plane=0):
        """-> (hashes uint64[n] strictly ascending, counts uint32[n]): every sampled value of the plane with its exact count (ntc_signature)"""
        cap = self.signature_size(plane)
        h = np.zeros(max(cap, 1), dtype=np.uint64)
        c = np.zeros(max(cap, 1), dtype=np.uint32)
        n = C.c_uint64()
        check(self._lib.ntc_signature(self._h, int(plane), _np_ptr(h), _np_ptr(c), cap, C.byref(n)))
        return h[:n.value].copy(), c[:n.value].copy()

    def signature_device(self, plane=0):
        """-> (hashes torch.int64[n] — the uint64 values' bits —, counts torch.int32[n] — uint32 likewise —, n): signature() with the sorted pairs left on the
        engine's device (ntc_signature_device)"""
        import torch
        cap = self.signature_size(plane)
        dev = torch.device("cuda", self.device)
        h = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        c = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        n = C.c_uint64()
        check(self._lib.ntc_signature_device(self._h, int(plane), C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), cap, C.byref(n)))
        return h[:n.value], c[:n.value], n.value

    def signature_sort_time(self):
        """-> ms of the device sorts of signature() / signature_device() while profiling (ntc_signature_sort_time)"""
        ms = C.c_double()
        check(self._lib.ntc_signature_sort_time(self._h, C.byref(ms)))
        return ms.value

    def signature_inject(self, hashes, counts=None, plane=0, device=False):
        """add pairs to a plane's signature: counts None = 1 each, duplicates add up, zeros are skipped (ntc_signature_inject).  device=True: hashes and
        counts are (device pointer, n) and device pointer or None, read stream-ordered (ntc_signature_inject_device)"""
        if device:
            ptr, n = hashes
            check(self._lib.ntc_signature_inject_device(self._h, int(plane), C.c_void_p(ptr) if n else None, C.c_void_p(counts) if counts else None, int(n)))
            return
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        c = np.ascontiguousarray(counts, dtype=np.uint32) if counts is not None else None
        assert c is None or c.size == h.size
        check(self._lib.ntc_signature_inject(self._h, int(plane), _np_ptr(h) if h.size else None, _np_ptr(c) if c is not None and c.size else None, h.size))

    def signature_stats(self):
        """-> (table slots of all planes, doublings of a table since create / reset) (ntc_signature_stats)"""
        slots, grows = C.c_uint64(), C.c_uint64()
        check(self._lib.ntc_signature_stats(self._h, C.byref(slots), C.byref(grows)))
        return slots.value, grows.value

    def signature_time(self):
        """-> (insert ms, grow ms) of the signature passes while profiling (ntc_signature_time)"""
        a, b = C.c_double(), C.c_double()
        check(self._lib.ntc_signature_time(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def signature_header(self, plane=0):
        """-> dict(k, gap, strand, hpc, s_bits, mask, n=0): how this plane is counted, as a signature file records it (ntc_signature_header)"""
        h = _abi.NtcSigHeader()
        check(self._lib.ntc_signature_header(self._h, int(plane), C.byref(h)))
        return _sig_header_dict(h)

    def sync(self):
        check(self._lib.ntc_sync(self._h))

    def flush(self):
        """apply the pending hit log to the device sketch (asynchronous on the engine's stream)"""
        check(self._lib.ntc_flush(self._h))

    def finish(self, counters=False, p_hist=True):
        """-> (t_counter uint16[nk,2,2^r] | None, p_hist uint32[nk,2,65536] | None, f1 uint64[nk])"""
        nk = len(self.klist)
        tc = np.zeros((nk, 2, 1 << self.r_bits), dtype=np.uint16) if counters else None
        ph = np.zeros((nk, 2, 65536), dtype=np.uint32) if p_hist else None
        f1 = np.zeros(nk, dtype=np.uint64)
        check(self._lib.ntc_finish(self._h, _np_ptr(tc) if counters else None, _np_ptr(ph) if p_hist else None, _np_ptr(f1)))
        return tc, ph, f1

    def merge_counters(self, t_counter, f1=None):
        """add a dumped t_Counter image (uint16[nk,2,2^r], from finish(counters=True)) and its F1 into this engine"""
        tc = np.ascontiguousarray(t_counter, dtype=np.uint16)
        assert tc.size == len(self.klist) * (2 << self.r_bits)
        f = np.ascontiguousarray(f1, dtype=np.uint64) if f1 is not None else None
        check(self._lib.ntc_merge_counters(self._h, _np_ptr(tc), _np_ptr(f) if f is not None else None))

    def device_state(self):
        sk, n, f1 = C.c_void_p(), C.c_uint64(), C.c_void_p()
        check(self._lib.ntc_device_state(self._h, C.byref(sk), C.byref(n), C.byref(f1)))
        return sk.value, n.value, f1.value

    def log_export(self, n_parts, d_keys_ptr=None, part_offset=None):
        """the pending hit log split by counter-range owner (include/ntcard_hip.h: ntc_log_export_device) -> counts per owner (list of int); with d_keys_ptr
        (device uint32 buffer) and part_offset (n_parts ints) the keys are written as well.  NtcError(NTC_ERR_STATE) when the sketch already holds counts."""
        counts = (C.c_uint64 * n_parts)()
        offs = (C.c_uint64 * n_parts)(*[int(x) for x in part_offset]) if part_offset is not None else None
        check(self._lib.ntc_log_export_device(self._h, n_parts, C.c_void_p(d_keys_ptr) if d_keys_ptr else None, offs, counts))
        return [int(c) for c in counts]

    def log_replace(self, d_keys_ptr, n_keys):
        """the n_keys counter indices at d_keys_ptr (device uint32) become the pending hit log (ntc_log_replace_device)"""
        check(self._lib.ntc_log_replace_device(self._h, C.c_void_p(d_keys_ptr) if n_keys else None, n_keys))

    def set_profiling(self, on=True):
        check(self._lib.ntc_set_profiling(self._h, 1 if on else 0))

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.ntc_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def update_mode(self):
        """0: hit log + partitioned apply, 1: direct atomics (waits for the stream)"""
        m = C.c_uint32()
        check(self._lib.ntc_update_mode(self._h, C.byref(m)))
        return m.value

    def merge_allocations(self):
        """buffers / streams / events ntc_merge_devices has created for this engine (kept between merges)"""
        n = C.c_uint64()
        check(self._lib.ntc_merge_allocations(self._h, C.byref(n)))
        return n.value

    def fixup_time(self):
        """milliseconds of the K1f launches (a span of their own on the engine's stream, not part of kernel_time: one per K1h launch, or with FLAG_DEFER_REDO
        one per up to 8)"""
        ms = C.c_double()
        check(self._lib.ntc_fixup_time(self._h, C.byref(ms)))
        return ms.value

    def apply_time(self):
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.ntc_apply_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


_STRAND_INDEX = {"canonical": 0, "forward": 1, "reverse": 2}


class HllEngine(Engine):
    """nthll: per plane a uint8 M[1<<n_bits] of max leading-zero runs (nthll.cpp:92-105,212-243).  k: an int (one plane; finish() -> (regs 1-D, f1 int))
    or a list of k (finish() -> (regs [n_planes, 1<<n_bits], f1 uint64[n_planes])); from_seeds: spaced seeds given as masks; strand as for Engine()
    (include/ntcard_hip.h: ntc_hll_create_ex)"""

    def __init__(self, k, n_bits=16, device=0, stream=None, strand="canonical", hpc=False):
        single = not isinstance(k, (list, tuple, np.ndarray))
        self._setup([int(k)] if single else [int(x) for x in k], None, n_bits, device, stream, strand, single, hpc)

    @classmethod
    def from_seeds(cls, masks, n_bits=16, device=0, stream=None, strand="canonical", hpc=False):
        self = cls.__new__(cls)
        self._h = None
        seeds = [s.decode() if isinstance(s, bytes) else str(s) for s in masks]
        self._setup([len(s) for s in seeds], seeds, n_bits, device, stream, strand, False, hpc)
        return self

    def _setup(self, klist, seeds, n_bits, device, stream, strand, single, hpc=False):
        self._h = None
        flags = _strand_flags(0, strand) | (FLAG_HPC if hpc else 0)  # (checked before the library is asked for a device)
        self._lib = _abi.lib()
        self.klist, self.seeds, self.gap, self.n_bits, self.device = klist, seeds, 0, int(n_bits), int(device)
        self.strand = "canonical" if strand is None else strand
        self._single = single
        cfg = _abi.NtcHllConfig()
        if seeds is None:
            self._karr = (C.c_uint32 * len(klist))(*klist)
            cfg.n_k, cfg.k = len(klist), C.cast(self._karr, C.POINTER(C.c_uint32))
        else:
            self._sarr = (C.c_char_p * len(seeds))(*[s.encode() for s in seeds])
            cfg.n_seeds, cfg.seeds = len(seeds), C.cast(self._sarr, C.POINTER(C.c_char_p))
        cfg.n_bits, cfg.device, cfg.flags = self.n_bits, self.device, flags
        cfg.stream = C.c_void_p(stream) if stream else None
        h = C.c_void_p()
        check(self._lib.ntc_hll_create_ex(C.byref(cfg), C.byref(h)))
        self._h = h

    def finish(self):
        n = len(self.klist)
        regs = np.zeros((n, 1 << self.n_bits), dtype=np.uint8)
        f1 = np.zeros(n, dtype=np.uint64)
        check(self._lib.ntc_hll_finish(self._h, _np_ptr(regs), _np_ptr(f1)))
        if self._single:
            return regs[0], int(f1[0])
        return regs, f1


def hll_estimate(regs, n_bits=16, strand="canonical"):
    """nthll's estimate of one plane's registers; strand: the engine's (a one-strand value is uniform, so its alpha is not halved)"""
    if not isinstance(strand, str) or strand not in _STRAND_INDEX:
        raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
    est = C.c_double()
    r = np.ascontiguousarray(regs, dtype=np.uint8)
    check(_abi.lib().ntc_hll_estimate_strand(_np_ptr(r), int(n_bits), _STRAND_INDEX[strand], C.byref(est)))
    return est.value


def merge_devices(engines):
    """sum (mod 2^16, like t_Counter) of the engines' sketches and F1 into engines[0] by a 16-bit slice exchange over peer copies;
    the others are reset (ntc_merge_devices)"""
    arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
    check(_abi.lib().ntc_merge_devices(arr, len(engines)))


def _sig_header_dict(h):
    return dict(k=h.k, gap=h.gap, strand=h.strand, hpc=h.hpc, s_bits=h.s_bits, mask=h.mask.decode(), n=h.n)


def signature_compare(a, b):
    """two hash lists (strictly ascending uint64) -> (common, jaccard, containment_a_in_b, containment_b_in_a); host only (ntc_signature_compare)"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    c = C.c_uint64()
    check(_abi.lib().ntc_signature_compare(_np_ptr(a) if a.size else None, a.size, _np_ptr(b) if b.size else None, b.size, C.byref(c)))
    common, union = c.value, a.size + b.size - c.value
    return common, (common / union if union else 0.0), (common / a.size if a.size else 0.0), (common / b.size if b.size else 0.0)


def signature_sort_device(ptr_keys, ptr_vals, n, device=0, stream=None):
    """n device pairs (uint64 key, uint32 value; ptr_vals None or 0: keys only) sorted in place, ascending by key and stable; synchronous
    (ntc_signature_sort_device)"""
    check(_abi.lib().ntc_signature_sort_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(ptr_keys) if ptr_keys else None,
                                               C.c_void_p(ptr_vals) if ptr_vals else None, int(n)))


def signature_compare_device(ptr_a, ptr_counts_a, na, ptr_b, ptr_counts_b, nb, device=0, stream=None):
    """two device hash lists (strictly ascending uint64; counts uint32 or None) -> (common, min_sum): |A n B| and, when both have counts, the sum of
    min(count_a, count_b) over the common hashes, else None; synchronous (ntc_signature_compare_device)"""
    c, m = C.c_uint64(), C.c_uint64()
    both = bool(ptr_counts_a) and bool(ptr_counts_b)
    check(_abi.lib().ntc_signature_compare_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(ptr_a) if ptr_a else None,
                                                  C.c_void_p(ptr_counts_a) if ptr_counts_a else None, int(na), C.c_void_p(ptr_b) if ptr_b else None,
                                                  C.c_void_p(ptr_counts_b) if ptr_counts_b else None, int(nb), C.byref(c), C.byref(m) if both else None))
    return c.value, (m.value if both else None)


def _device_lists(ptrs, ns):
    """-> (how many, void* array, uint64 array) of device lists for the C ABI (arrays of one element for no list)"""
    assert len(ptrs) == len(ns)
    k = len(ptrs)
    return k, (C.c_void_p * max(k, 1))(*[C.c_void_p(int(p)) if p else None for p in ptrs]), (C.c_uint64 * max(k, 1))(*[int(x) for x in ns])


def signature_matrix_device(ptrs, ns, device=0, stream=None):
    """device hash lists ptrs[i] of ns[i] strictly ascending uint64 each -> np.ndarray[uint64] (len, len): the size of every pair's intersection, the diagonal
    ns; synchronous (ntc_signature_matrix_device)"""
    k, arr, n = _device_lists(ptrs, ns)
    out = np.zeros((k, k), dtype=np.uint64)
    check(_abi.lib().ntc_signature_matrix_device(device, C.c_void_p(stream) if stream else None, k, arr, n, _np_ptr(out) if k else None))
    return out


# ntc_gather_row as a structured array
GATHER_ROW_DTYPE = np.dtype([("ref", np.uint32), ("reserved", np.uint32), ("common", np.uint64), ("unique", np.uint64), ("unique_weight", np.uint64)])


def signature_gather_device(ptr_q, ptr_counts_q, nq, ptrs, ns, threshold=1, max_rows=None, device=0, stream=None):
    """gather: the greedy decomposition of a device query (nq strictly ascending uint64 hashes; counts uint32, or None / 0: 1 each) over the device lists
    ptrs[i] of ns[i] strictly ascending uint64 each -> (rows, unassigned, unassigned_weight).  rows: a structured array (GATHER_ROW_DTYPE) in pick order,
    at most max_rows of them (None: as many as there are references); a round's pick is the reference with the most query entries no earlier pick took,
    the lowest index among equals, and the run ends when that count falls below `threshold` hashes; synchronous (ntc_signature_gather_device)"""
    k, arr, n = _device_lists(ptrs, ns)
    cap = k if max_rows is None else int(max_rows)
    rows = np.zeros(max(cap, 1), dtype=GATHER_ROW_DTYPE)
    n_rows, rest, rest_w = C.c_uint32(), C.c_uint64(), C.c_uint64()
    check(_abi.lib().ntc_signature_gather_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(ptr_q) if ptr_q else None,
                                                 C.c_void_p(ptr_counts_q) if ptr_counts_q else None, int(nq), k, arr, n, int(threshold),
                                                 rows.ctypes.data_as(C.POINTER(_abi.NtcGatherRow)) if cap else None, cap, C.byref(n_rows), C.byref(rest),
                                                 C.byref(rest_w)))
    return rows[:n_rows.value].copy(), rest.value, rest_w.value


def _device_pairs_out(call, device):
    """the output protocol of union and select: call(d_hashes, d_counts, cap, n_out) once for the size and once into fresh torch tensors
    -> (hashes torch.int64[n] — the uint64 values' bits —, counts torch.int32[n] — uint32 likewise —, n)"""
    import torch
    n = C.c_uint64()
    check(call(None, None, 0, C.byref(n)))
    cap = n.value
    dev = torch.device("cuda", device)
    h = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    c = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    check(call(C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), cap, C.byref(n)))
    return h[:n.value], c[:n.value], n.value


def signature_union_device(ptrs, count_ptrs, ns, device=0, stream=None):
    """the union of the device lists ptrs[i] of ns[i] strictly ascending uint64 each; count_ptrs: None, or per list a device uint32 array or None / 0
    (1 each) -> (hashes, counts, n) as Engine.signature_device gives them: the distinct hashes ascending, counts added and saturating at 2^32 - 1;
    synchronous (ntc_signature_union_device)"""
    k, arr, n = _device_lists(ptrs, ns)
    carr = None
    if count_ptrs is not None:
        assert len(count_ptrs) == k
        carr = (C.c_void_p * max(k, 1))(*[C.c_void_p(int(p)) if p else None for p in count_ptrs])
    st = C.c_void_p(stream) if stream else None
    return _device_pairs_out(lambda h, c, cap, n_out: _abi.lib().ntc_signature_union_device(device, st, k, arr, carr, n, h, c, cap, n_out), device)


_SELECT_MODES = {"all": 0, "none": 1, "any": 2}  # NTC_SIG_IN_ALL, _NONE, _ANY


def signature_select_device(ptr_a, ptr_ca, na, ptrs, ns, mode="all", min_count=0, max_count=0, device=0, stream=None):
    """the entries of the device signature A (na strictly ascending uint64 hashes; counts uint32, or None / 0: 1 each) that pass the count test
    (min_count <= c, and c <= max_count unless max_count is 0) and the membership rule over the device lists ptrs[i] of ns[i] strictly ascending uint64 each:
    mode "all" — every list holds the hash (intersect) —, "none" — no list does (subtract) —, "any" — at least one does -> (hashes, counts, n) in A's
    order; synchronous (ntc_signature_select_device)"""
    k, arr, n = _device_lists(ptrs, ns)
    st = C.c_void_p(stream) if stream else None
    a, ca = (C.c_void_p(ptr_a) if ptr_a else None), (C.c_void_p(ptr_ca) if ptr_ca else None)
    m = _SELECT_MODES[mode]
    return _device_pairs_out(lambda h, c, cap, n_out: _abi.lib().ntc_signature_select_device(device, st, a, ca, int(na), k, arr if k else None, n if k else None, m,
                                                                                               int(min_count), int(max_count), h, c, cap, n_out), device)


def signature_hist_device(ptr_counts, n, cov_max=1000, device=0, stream=None):
    """the abundance spectrum of n device counts (uint32) -> (hist np.uint64[cov_max + 2], weight np.uint64): hist[v] = the entries with count v,
    hist[cov_max + 1] = those with a larger count, weight = the sum of the counts; synchronous (ntc_signature_hist_device)"""
    cov_max = int(cov_max)
    hist = np.zeros(max(cov_max, 0) + 2, dtype=np.uint64)
    w = C.c_uint64()
    check(_abi.lib().ntc_signature_hist_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(ptr_counts) if ptr_counts else None, int(n), cov_max,
                                               _np_ptr(hist), C.byref(w)))
    return hist, np.uint64(w.value)


def signature_write(path, header, hashes, counts):
    """a signature file; header: dict(k, gap, strand, hpc, s_bits, mask) as Engine.signature_header() gives it (ntc_signature_write)"""
    hs = np.ascontiguousarray(hashes, dtype=np.uint64)
    cs = np.ascontiguousarray(counts, dtype=np.uint32)
    assert hs.size == cs.size
    h = _abi.NtcSigHeader()
    h.k, h.gap, h.strand, h.hpc, h.s_bits, h.n = int(header["k"]), int(header["gap"]), int(header["strand"]), int(header["hpc"]), int(header["s_bits"]), hs.size
    h.mask = header["mask"].encode()
    check(_abi.lib().ntc_signature_write(str(path).encode(), C.byref(h), _np_ptr(hs) if hs.size else None, _np_ptr(cs) if cs.size else None))


def signature_read(path):
    """-> (header dict, hashes uint64[n], counts uint32[n]) of a signature file (ntc_signature_read)"""
    h = _abi.NtcSigHeader()
    check(_abi.lib().ntc_signature_read(str(path).encode(), C.byref(h), None, None, 0))
    hs = np.zeros(max(h.n, 1), dtype=np.uint64)
    cs = np.zeros(max(h.n, 1), dtype=np.uint32)
    check(_abi.lib().ntc_signature_read(str(path).encode(), C.byref(h), _np_ptr(hs), _np_ptr(cs), max(h.n, 1)))
    return _sig_header_dict(h), hs[:h.n].copy(), cs[:h.n].copy()


# -- stateless entry points ---------------------------------------------------------------------
def estimate(p_hist_k, r_bits, s_bits, cov_max=1000):
    """compEst for one k from p[2][65536] -> (F0, f[0..cov_max])"""
    p = np.ascontiguousarray(p_hist_k, dtype=np.uint32)
    assert p.shape == (2, 65536)
    cov_max = min(int(cov_max), 65535)
    f0 = C.c_double()
    f = np.zeros(cov_max + 1, dtype=np.float64)
    check(_abi.lib().ntc_estimate(_np_ptr(p), r_bits, s_bits, cov_max, C.byref(f0), _np_ptr(f)))
    return f0.value, f


def write_hist(path, f1, F0, f, cov_max=1000):
    f = np.ascontiguousarray(f, dtype=np.float64)
    check(_abi.lib().ntc_write_hist(str(path).encode(), int(f1), float(F0), _np_ptr(f), min(int(cov_max), 65535)))


def gen_reads_device(d_ptr, seed, first, n, read_len, stride, dist, genome_len=100_000_000, device=0, stream=None):
    check(_abi.lib().ntc_gen_reads_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_ptr), seed, first, n,
                                          read_len, stride, dist, genome_len))


def long_plan(k, piece_len, n):
    """the cut of one sequence of n bytes into pieces of piece_len -> (full pieces m, start of the remainder [m S, n)), S = piece_len - (k - 1); k: the
    engine's k, for a k list its largest (one cut serves the list).  ntc_long_plan, host only"""
    m, rem = C.c_uint64(), C.c_uint64()
    check(_abi.lib().ntc_long_plan(int(k), int(piece_len), int(n), C.byref(m), C.byref(rem)))
    return m.value, rem.value


def hpc_compress(seq):
    """homopolymer compression of one sequence (bytes) -> bytes: every byte that repeats the base class (A, C, G, T = U, either case) of the byte in front
    of it is dropped (ntc_hpc_compress, host only)"""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    out = np.empty(max(a.size, 1), dtype=np.uint8)
    n = C.c_uint64()
    check(_abi.lib().ntc_hpc_compress(_np_ptr(a) if a.size else None, a.size, _np_ptr(out), C.byref(n)))
    return out[:n.value].tobytes()


def hpc_compress_device(d_in_ptr, offsets, d_out_ptr, device=0, stream=None):
    """the same for device-resident sequences [offsets[i], offsets[i + 1]) of d_in (host offsets, any alignment) into d_out (room for
    offsets[-1] - offsets[0] bytes) -> the new offsets, uint64[n + 1] from 0; synchronous (ntc_hpc_compress_device)"""
    o = np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(len(o), dtype=np.uint64)
    check(_abi.lib().ntc_hpc_compress_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_in_ptr) if d_in_ptr else None, _np_ptr(o),
                                             len(o) - 1, C.c_void_p(d_out_ptr) if d_out_ptr else None, _np_ptr(out)))
    return out


K1_REGIMES = ("PREFETCH", "BLOCKING", "PARTIAL", "META", "SMALL_BLOCK", "IDLE", "MULTI", "LOG")  # ntc_k1_variant_info::regime, in order


def k1_variant_stats():
    """what the general kernel K1 has launched in this process, one dict per row of its table of instantiations: row (multi, mode, pref, dump, tiled, one,
    sig), launches, regime {name: launches in it, K1_REGIMES}, last_grid, last_wpb, last_stride, last_n_slots (ntc_k1_variant_stats; host only)"""
    L, out, info = _abi.lib(), [], _abi.NtcK1VariantInfo()
    while L.ntc_k1_variant_stats(len(out), C.byref(info)) == 0:
        out.append(dict(row=(bool(info.multi), info.mode, info.pref, bool(info.dump), bool(info.tiled), bool(info.one), bool(info.sig)),
                        launches=info.launches, regime=dict(zip(K1_REGIMES, info.regime)), last_grid=info.last_grid, last_wpb=info.last_wpb,
                        last_stride=info.last_stride, last_n_slots=info.last_n_slots))
    return out


def tiled_bytes(n_reads, read_len):
    """size of a batch in the tiled layout"""
    return int(_abi.lib().ntc_tiled_bytes(n_reads, read_len))


def gen_reads_tiled_device(d_ptr, seed, first, n, read_len, dist, genome_len=100_000_000, device=0, stream=None):
    """the reads of gen_reads_device (bit-identical bases) in the tiled layout"""
    check(_abi.lib().ntc_gen_reads_tiled_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_ptr), seed, first, n,
                                                read_len, dist, genome_len))


def tile_reads(reads, read_len=None):
    """host-side packing of equal-length reads (list of bytes) into the tiled layout -> uint8 array (tests, small inputs)"""
    n = len(reads)
    L = read_len if read_len is not None else (len(reads[0]) if n else 0)
    C16 = (L + 15) // 16
    nt = (n + 2047) // 2048
    out = np.full((nt, C16, 2048, 16), ord("A"), dtype=np.uint8)
    if n:
        a = np.full((nt * 2048, C16 * 16), ord("A"), dtype=np.uint8)
        a[:n, :L] = np.frombuffer(b"".join(reads), dtype=np.uint8).reshape(n, L)
        out[:] = a.reshape(nt, 2048, C16, 16).transpose(0, 2, 1, 3)
    return out.reshape(-1)


def tile_reads_ragged(reads, n_chunks):
    """host-side packing of a RAGGED batch (reads of 16 n_chunks - 15 .. 16 n_chunks bases, list of bytes) -> (tiles uint8 array, tails uint32
    [n_tiles, 16], order): the reads are sorted longest first (order[j] = index of the read in slot j), tails[t, d] = reads of tile t with more than d
    bases in their last piece (tests, small inputs)"""
    n, C16 = len(reads), int(n_chunks)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    assert n == 0 or (lens.min() > 16 * (C16 - 1) and lens.max() <= 16 * C16)
    order = np.argsort(-lens, kind="stable")
    nt = (n + 2047) // 2048
    a = np.full((nt * 2048, C16 * 16), ord("A"), dtype=np.uint8)
    for j, i in enumerate(order):
        a[j, :lens[i]] = np.frombuffer(reads[i], dtype=np.uint8)
    tails = np.zeros((nt, 16), dtype=np.uint32)
    tl = lens[order] - 16 * (C16 - 1)
    for t in range(nt):
        part = tl[t * 2048:(t + 1) * 2048]
        for d in range(16):
            tails[t, d] = int(np.count_nonzero(part > d))
    tiles = np.ascontiguousarray(a.reshape(nt, 2048, C16, 16).transpose(0, 2, 1, 3)).reshape(-1)
    return tiles, tails, order


def value_hist_device(d_counters_ptr, n, d_hist_ptr, device=0, stream=None):
    """accumulate the value histogram (counter & 0xffff) of n device uint32 counters into a device uint32[65536]"""
    check(_abi.lib().ntc_value_hist_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_counters_ptr), n,
                                           C.c_void_p(d_hist_ptr)))


def narrow_u16_device(d_counters_ptr, n, d_out_ptr, device=0, stream=None):
    """d_out (uint16[n]) = the low halves of n device uint32 counters (t_Counter wraps at 16 bits: all the merge has to move)"""
    check(_abi.lib().ntc_narrow_u16_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_counters_ptr), n, C.c_void_p(d_out_ptr)))


def sum_slices_u16_device(d_slices_ptr, stride, n_slices, length, device=0, stream=None):
    """slice 0 += slices 1 .. n_slices - 1 with wrapping 16-bit adds; slice r = uint16[r * stride : r * stride + length]"""
    check(_abi.lib().ntc_sum_slices_u16_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_slices_ptr), stride, n_slices, length))


def value_hist_u16_device(d_counters_ptr, n, d_hist_ptr, device=0, stream=None):
    """accumulate the value histogram of n device uint16 counters into a device uint32[65536]"""
    check(_abi.lib().ntc_value_hist_u16_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_counters_ptr), n, C.c_void_p(d_hist_ptr)))


def hash_dump_device(d_slots_ptr, n_reads, read_len, stride, k, gap, max_win, d_hash_ptr, d_count_ptr, device=0, stream=None, k1=False):
    """every canonical (spaced-seed when gap != 0) hash of every clean window; k1=True: out of the production kernel K1"""
    fn = _abi.lib().ntc_hash_dump_k1_device if k1 else _abi.lib().ntc_hash_dump_device
    check(fn(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_slots_ptr), n_reads,
                                          read_len, stride, k, gap, max_win, C.c_void_p(d_hash_ptr), C.c_void_p(d_count_ptr)))


def hash_dump_seed_device(d_slots_ptr, n_reads, read_len, stride, seed, max_win, d_hash_ptr, d_count_ptr, device=0, stream=None):
    """every canonical spaced-seed hash of every clean window under a mask of '0' / '1', out of the production kernel K1
    (include/ntcard_hip.h: ntc_hash_dump_seed_device)"""
    seed = seed.encode() if isinstance(seed, str) else bytes(seed)
    check(_abi.lib().ntc_hash_dump_seed_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_slots_ptr), n_reads, read_len, stride, seed,
                                               max_win, C.c_void_p(d_hash_ptr), C.c_void_p(d_count_ptr)))


def hash_dump_strand_device(d_slots_ptr, n_reads, read_len, stride, seed, strand, max_win, d_hash_ptr, d_count_ptr, device=0, stream=None):
    """hash_dump_seed_device with a strand: 0 the canonical value, 1 the forward, 2 the reverse value of every clean window
    (include/ntcard_hip.h: ntc_hash_dump_strand_device)"""
    seed = seed.encode() if isinstance(seed, str) else bytes(seed)
    check(_abi.lib().ntc_hash_dump_strand_device(device, C.c_void_p(stream) if stream else None, C.c_void_p(d_slots_ptr), n_reads, read_len, stride, seed,
                                                 int(strand), max_win, C.c_void_p(d_hash_ptr), C.c_void_p(d_count_ptr)))
