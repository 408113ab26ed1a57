"""Bloom filters of every k-mer on the device (include/ntcard_hip.h: ntc_bloom_*; DESIGN.md §4 "Bloom filters"): the step behind ntCard's F0 — and
counting filters (ntc_cbloom_*; DESIGN.md §4 "Counting filters and solid k-mers"): the step behind its f_i, k-mer counts and the filter of the solid k-mers.

The layout is the reference's vendor/ntHash/lib/BloomFilter.hpp — position h_i % m, bit 7 - loc % 8 of byte loc / 8, h_i the multi-hash of
nthash.hpp:381-390 — so `BloomFilter.bytes()` is what `storeFilter` writes.  BlockedBloomFilter (ntc_bbloom_*; DESIGN.md §4 "Blocked filters") is a
second kind beside it, in a layout of its own: every bit of a k-mer in one 64-byte block.  torch is plumbing only: it owns the filter's device memory.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import BBLOOM_BLOCK_BITS, BLOOM_BLOCK, NtcBloomHeader, check  # noqa: F401  (BLOOM_BLOCK is re-exported)

_STRANDS = {"canonical": 0, "forward": 1, "reverse": 2}
_STRAND_NAMES = {v: s for s, v in _STRANDS.items()}


def bloom_size(n_distinct, fpr, n_hash=3):
    """ntc_bloom_size: the bits of a filter — or the counters of a counting filter — that holds n_distinct k-mers at false positive rate fpr with n_hash
    hashes, a multiple of 64"""
    m = C.c_uint64(0)
    check(_abi.lib().ntc_bloom_size(int(n_distinct), int(n_hash), float(fpr), C.byref(m)))
    return int(m.value)


def _offsets(offsets):
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets: a 1-d array of n_seqs + 1 values")
    return off


class BloomFilter:
    """A Bloom filter of m_bits bits on one device, n_hash positions per k-mer, the k-mers' values taken as an Engine of that strand takes them.

    insert / query take a torch uint8 tensor of bases on the filter's device and HOST offsets (n_seqs + 1, non-decreasing; sequence i is
    bases[offsets[i]:offsets[i + 1]]), the layout of Engine.submit_long_device."""

    def __init__(self, m_bits, n_hash, k, strand="canonical", device=0):
        import torch
        if strand not in _STRANDS:
            raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
        m_bits, n_hash, k = int(m_bits), int(n_hash), int(k)
        if not 1 <= m_bits < 1 << 40:
            raise ValueError(f"m_bits={m_bits} outside 1 .. 2^40 - 1")
        if not 1 <= n_hash <= 32:
            raise ValueError(f"n_hash={n_hash} outside 1 .. 32")
        if not 1 <= k <= _abi.lib().ntc_max_k():
            raise ValueError(f"k={k} outside 1 .. {_abi.lib().ntc_max_k()}")
        self.m_bits, self.n_hash, self.k, self.strand, self.device = m_bits, n_hash, k, strand, int(device)
        self.n_inserted = 0
        self.n_bytes = (m_bits + 7) // 8
        self.filter = torch.zeros((self.n_bytes + 3) // 4 * 4, dtype=torch.uint8, device=f"cuda:{self.device}")

    @classmethod
    def for_distinct(cls, n, fpr, n_hash, k, strand="canonical", device=0):
        """A filter sized by ntc_bloom_size for n distinct k-mers at false positive rate fpr.  n is what ntCard estimates: the F0 that
        `estimate(p_hist, r_bits, s_bits)` returns for the value histogram of `Engine.finish()` — or the F0 line of the `.hist` file."""
        return cls(bloom_size(n, fpr, n_hash), n_hash, k, strand, device)

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _bases(self, bases):
        import torch
        if not isinstance(bases, torch.Tensor) or bases.dtype != torch.uint8 or not bases.is_cuda or bases.device.index != self.device or not bases.is_contiguous():
            raise ValueError("bases: a contiguous torch uint8 tensor on the filter's device")
        return bases

    def insert(self, bases, offsets):
        """Inserts every k-mer of the sequences; -> the windows inserted"""
        off = _offsets(offsets)
        bases = self._bases(bases)
        if int(off[-1]) > bases.numel():
            raise ValueError("offsets reach behind the end of bases")
        n = C.c_uint64(0)
        check(_abi.lib().ntc_bloom_insert_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                 bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n)))
        self.n_inserted += int(n.value)
        return int(n.value)

    def query(self, bases, offsets):
        """-> (windows, hits): numpy uint32 [n_seqs] each, the k-mers of every sequence and those of them the filter holds"""
        import torch
        off = _offsets(offsets)
        bases = self._bases(bases)
        if int(off[-1]) > bases.numel():
            raise ValueError("offsets reach behind the end of bases")
        n_seqs = off.size - 1
        out = torch.empty((2, max(n_seqs, 1)), dtype=torch.int32, device=self.filter.device)
        check(_abi.lib().ntc_bloom_query_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                bases.data_ptr(), off.ctypes.data_as(C.c_void_p), n_seqs, out[0].data_ptr(), out[1].data_ptr()))
        host = out[:, :n_seqs].cpu().numpy().view(np.uint32)
        return host[0].copy(), host[1].copy()

    def _hashes(self, h0):
        import torch
        if isinstance(h0, torch.Tensor):
            if h0.dtype not in (torch.int64, torch.uint64) or not h0.is_cuda or h0.device.index != self.device or not h0.is_contiguous():
                raise ValueError("hashes: a contiguous 64-bit torch tensor on the filter's device, or a numpy array")
            return h0
        return torch.from_numpy(np.ascontiguousarray(h0, dtype=np.uint64).view(np.int64)).to(self.filter.device)

    def insert_hashes(self, h0):
        """Sets the n_hash bits of every given value h_0 (numpy uint64, or a 64-bit tensor on the device) — a signature's hashes, say"""
        d = self._hashes(h0)
        check(_abi.lib().ntc_bloom_insert_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                        d.data_ptr() if d.numel() else None, d.numel()))
        self.n_inserted += d.numel()

    def query_hashes(self, h0):
        """-> numpy bool [n]: whether all n_hash bits of each given h_0 are set"""
        import torch
        d = self._hashes(h0)
        flags = torch.empty(max(d.numel(), 1), dtype=torch.uint8, device=self.filter.device)
        check(_abi.lib().ntc_bloom_query_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                       d.data_ptr() if d.numel() else None, d.numel(), flags.data_ptr()))
        return flags[: d.numel()].cpu().numpy().astype(bool)

    def popcount(self):
        pop = C.c_uint64(0)
        check(_abi.lib().ntc_bloom_popcount_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, C.byref(pop)))
        return int(pop.value)

    def fpr(self):
        """(popcount / m_bits) ** n_hash: the chance that a k-mer that was never inserted finds all its bits set"""
        return (self.popcount() / self.m_bits) ** self.n_hash

    def merge(self, other):
        """ORs another filter of the same shape into this one (shards of one input, peers' filters)"""
        if (other.m_bits, other.n_hash, other.k, other.strand) != (self.m_bits, self.n_hash, self.k, self.strand):
            raise ValueError("merge: the filters differ in m_bits, n_hash, k or strand")
        src = other.filter if other.device == self.device else other.filter.to(self.filter.device)
        check(_abi.lib().ntc_bloom_or_device(self.device, self._stream(), self.filter.data_ptr(), src.data_ptr(), self.m_bits))
        self.n_inserted += other.n_inserted

    def bytes(self):
        """The reference's byte image, (m_bits + 7) // 8 bytes, as numpy uint8"""
        return self.filter[: self.n_bytes].cpu().numpy()

    def save(self, path):
        h = NtcBloomHeader(k=self.k, n_hash=self.n_hash, strand=_STRANDS[self.strand], reserved=0, m_bits=self.m_bits, n_inserted=self.n_inserted)
        image = np.ascontiguousarray(self.bytes())
        check(_abi.lib().ntc_bloom_write(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p)))

    @classmethod
    def load(cls, path, device=0):
        import torch
        h, image = read_file(path)
        f = cls(h["m_bits"], h["n_hash"], h["k"], h["strand"], device)
        f.n_inserted = h["n_inserted"]
        f.filter[: f.n_bytes] = torch.from_numpy(image).to(f.filter.device)
        return f


def read_file(path):
    """ntc_bloom_read -> (header dict, the byte image as numpy uint8): pure host"""
    h = NtcBloomHeader()
    L = _abi.lib()
    check(L.ntc_bloom_read(str(path).encode(), C.byref(h), None, 0))
    image = np.zeros((h.m_bits + 7) // 8, dtype=np.uint8)
    check(L.ntc_bloom_read(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p), image.size))
    return {"k": h.k, "n_hash": h.n_hash, "strand": _STRAND_NAMES[h.strand], "m_bits": int(h.m_bits), "n_inserted": int(h.n_inserted)}, image


def bbloom_fpr(n_distinct, m_bits, n_hash=3):
    """ntc_bbloom_fpr: the false positive rate of a blocked filter of m_bits bits that holds n_distinct k-mers"""
    fpr = C.c_double(0.0)
    check(_abi.lib().ntc_bbloom_fpr(int(n_distinct), int(m_bits), int(n_hash), C.byref(fpr)))
    return float(fpr.value)


def bbloom_size(n_distinct, fpr, n_hash=3):
    """ntc_bbloom_size: the bits of a blocked filter that holds n_distinct k-mers at false positive rate fpr, the smallest multiple of 512 that does"""
    m = C.c_uint64(0)
    check(_abi.lib().ntc_bbloom_size(int(n_distinct), int(n_hash), float(fpr), C.byref(m)))
    return int(m.value)


class BlockedBloomFilter:
    """A BLOCKED Bloom filter of m_bits bits (a multiple of 512) on one device: all n_hash bits of a k-mer lie in one aligned 512-bit block — one random
    cache line per k-mer where BloomFilter fetches n_hash — at the price of a somewhat larger filter for the same false positive rate (bbloom_size) and
    of a format of its own (include/ntcard_hip.h: ntc_bbloom_*).  Constructor, inputs and streams as BloomFilter's; the image is an ordinary bit image,
    so popcount and merge are BloomFilter's calls."""

    def __init__(self, m_bits, n_hash, k, strand="canonical", device=0):
        import torch
        if strand not in _STRANDS:
            raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
        m_bits, n_hash, k = int(m_bits), int(n_hash), int(k)
        if not BBLOOM_BLOCK_BITS <= m_bits < 1 << 40 or m_bits % BBLOOM_BLOCK_BITS:
            raise ValueError(f"m_bits={m_bits} is no multiple of 512 in 512 .. 2^40 - 512")
        if not 1 <= n_hash <= 32:
            raise ValueError(f"n_hash={n_hash} outside 1 .. 32")
        if not 1 <= k <= _abi.lib().ntc_max_k():
            raise ValueError(f"k={k} outside 1 .. {_abi.lib().ntc_max_k()}")
        self.m_bits, self.n_hash, self.k, self.strand, self.device = m_bits, n_hash, k, strand, int(device)
        self.n_inserted = 0
        self.n_bytes = m_bits // 8
        self.n_blocks = m_bits // BBLOOM_BLOCK_BITS
        self.filter = torch.zeros(self.n_bytes, dtype=torch.uint8, device=f"cuda:{self.device}")

    @classmethod
    def for_distinct(cls, n, fpr, n_hash, k, strand="canonical", device=0):
        """A filter sized by ntc_bbloom_size for n distinct k-mers at false positive rate fpr (n: ntCard's F0, as for BloomFilter.for_distinct)"""
        return cls(bbloom_size(n, fpr, n_hash), n_hash, k, strand, device)

    _stream = BloomFilter._stream
    _bases = BloomFilter._bases
    _hashes = BloomFilter._hashes
    popcount = BloomFilter.popcount
    bytes = BloomFilter.bytes

    def merge(self, other):
        """ORs another blocked filter of the same shape into this one (ntc_bloom_or_device: the image is an ordinary bit image)"""
        if not isinstance(other, BlockedBloomFilter):
            raise ValueError("merge: the other filter is no blocked filter")
        BloomFilter.merge(self, other)

    def _input(self, bases, offsets):
        off = _offsets(offsets)
        bases = self._bases(bases)
        if int(off[-1]) > bases.numel():
            raise ValueError("offsets reach behind the end of bases")
        return bases, off

    def insert(self, bases, offsets):
        """Inserts every k-mer of the sequences; -> the windows inserted"""
        bases, off = self._input(bases, offsets)
        n = C.c_uint64(0)
        check(_abi.lib().ntc_bbloom_insert_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                  bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n)))
        self.n_inserted += int(n.value)
        return int(n.value)

    def query(self, bases, offsets):
        """-> (windows, hits): numpy uint32 [n_seqs] each, the k-mers of every sequence and those of them the filter holds"""
        import torch
        bases, off = self._input(bases, offsets)
        n_seqs = off.size - 1
        out = torch.empty((2, max(n_seqs, 1)), dtype=torch.int32, device=self.filter.device)
        check(_abi.lib().ntc_bbloom_query_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                 bases.data_ptr(), off.ctypes.data_as(C.c_void_p), n_seqs, out[0].data_ptr(), out[1].data_ptr()))
        host = out[:, :n_seqs].cpu().numpy().view(np.uint32)
        return host[0].copy(), host[1].copy()

    def insert_hashes(self, h0):
        """Sets the n_hash bits of every given value h_0 (numpy uint64, or a 64-bit tensor on the device)"""
        d = self._hashes(h0)
        check(_abi.lib().ntc_bbloom_insert_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                         d.data_ptr() if d.numel() else None, d.numel()))
        self.n_inserted += d.numel()

    def query_hashes(self, h0):
        """-> numpy bool [n]: whether all n_hash bits of each given h_0 are set"""
        import torch
        d = self._hashes(h0)
        flags = torch.empty(max(d.numel(), 1), dtype=torch.uint8, device=self.filter.device)
        check(_abi.lib().ntc_bbloom_query_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                        d.data_ptr() if d.numel() else None, d.numel(), flags.data_ptr()))
        return flags[: d.numel()].cpu().numpy().astype(bool)

    def insert_solid(self, counting, bases, offsets, min_count):
        """Inserts every k-mer of the sequences whose count in the CountingBloomFilter `counting` (this filter's k, strand and device) is >= min_count;
        -> the windows that passed"""
        if not isinstance(counting, CountingBloomFilter) or (counting.k, counting.strand, counting.device) != (self.k, self.strand, self.device):
            raise ValueError("insert_solid: `counting` is a CountingBloomFilter of this filter's k, strand and device")
        bases, off = self._input(bases, offsets)
        n = C.c_uint64(0)
        check(_abi.lib().ntc_bbloom_insert_solid_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, counting.filter.data_ptr(),
                                                        counting.m_bits, counting.n_hash, CountingBloomFilter._min_count(min_count), self.k, _STRANDS[self.strand],
                                                        bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n)))
        self.n_inserted += int(n.value)
        return int(n.value)

    def block_hist(self):
        """-> numpy uint64 [513]: how many blocks hold 0, 1, .. 512 set bits"""
        h = np.zeros(BBLOOM_BLOCK_BITS + 1, dtype=np.uint64)
        check(_abi.lib().ntc_bbloom_hist_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, h.ctypes.data_as(C.c_void_p)))
        return h

    def fpr(self):
        """sum_v hist[v] (v / 512)^n_hash / n_blocks: the chance that a k-mer that was never inserted finds all its bits set — per block, not from the
        overall popcount: a block fuller than the average answers wrongly more often than the average says"""
        h = self.block_hist()
        v = np.arange(BBLOOM_BLOCK_BITS + 1, dtype=np.float64) / BBLOOM_BLOCK_BITS
        return float((h.astype(np.float64) * v ** self.n_hash).sum() / self.n_blocks)

    def write(self, path):
        h = NtcBloomHeader(k=self.k, n_hash=self.n_hash, strand=_STRANDS[self.strand], reserved=BBLOOM_BLOCK_BITS, m_bits=self.m_bits, n_inserted=self.n_inserted)
        image = np.ascontiguousarray(self.bytes())
        check(_abi.lib().ntc_bbloom_write(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p)))

    @classmethod
    def read(cls, path, device=0):
        import torch
        h, image = read_blocked_file(path)
        f = cls(h["m_bits"], h["n_hash"], h["k"], h["strand"], device)
        f.n_inserted = h["n_inserted"]
        f.filter[: f.n_bytes] = torch.from_numpy(image).to(f.filter.device)
        return f


def read_blocked_file(path):
    """ntc_bbloom_read -> (header dict, the byte image as numpy uint8): pure host"""
    h = NtcBloomHeader()
    L = _abi.lib()
    check(L.ntc_bbloom_read(str(path).encode(), C.byref(h), None, 0))
    image = np.zeros(h.m_bits // 8, dtype=np.uint8)
    check(L.ntc_bbloom_read(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p), image.size))
    return {"k": h.k, "n_hash": h.n_hash, "strand": _STRAND_NAMES[h.strand], "m_bits": int(h.m_bits), "n_inserted": int(h.n_inserted),
            "block_bits": int(h.reserved)}, image


class CountingBloomFilter:
    """A counting Bloom filter of m_bits 8-bit counters on one device (m_bits: the NUMBER OF COUNTERS, the name BloomFilter uses for its positions): an
    insert adds one to each of a k-mer's n_hash counters, saturating at 255; the count of a k-mer is the minimum of its counters.  Constructor, inputs and
    streams as BloomFilter's."""

    def __init__(self, m_bits, n_hash, k, strand="canonical", device=0):
        import torch
        if strand not in _STRANDS:
            raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
        m_bits, n_hash, k = int(m_bits), int(n_hash), int(k)
        if not 1 <= m_bits < 1 << 40:
            raise ValueError(f"m_bits={m_bits} outside 1 .. 2^40 - 1")
        if not 1 <= n_hash <= 32:
            raise ValueError(f"n_hash={n_hash} outside 1 .. 32")
        if not 1 <= k <= _abi.lib().ntc_max_k():
            raise ValueError(f"k={k} outside 1 .. {_abi.lib().ntc_max_k()}")
        self.m_bits, self.n_hash, self.k, self.strand, self.device = m_bits, n_hash, k, strand, int(device)
        self.n_inserted = 0
        self.n_bytes = m_bits
        self.filter = torch.zeros((self.n_bytes + 3) // 4 * 4, dtype=torch.uint8, device=f"cuda:{self.device}")

    @classmethod
    def for_distinct(cls, n, fpr, n_hash, k, strand="canonical", device=0):
        """A filter of ntc_bloom_size(n, n_hash, fpr) counters: a k-mer that was never inserted reads a count >= 1 at rate fpr"""
        return cls(bloom_size(n, fpr, n_hash), n_hash, k, strand, device)

    _stream = BloomFilter._stream
    _bases = BloomFilter._bases
    _hashes = BloomFilter._hashes

    def _input(self, bases, offsets):
        off = _offsets(offsets)
        bases = self._bases(bases)
        if int(off[-1]) > bases.numel():
            raise ValueError("offsets reach behind the end of bases")
        return bases, off

    @staticmethod
    def _min_count(min_count):
        min_count = int(min_count)
        if not 1 <= min_count <= 255:
            raise ValueError(f"min_count={min_count} outside 1 .. 255")
        return min_count

    def insert(self, bases, offsets):
        """Counts every k-mer of the sequences; -> the windows inserted"""
        bases, off = self._input(bases, offsets)
        n = C.c_uint64(0)
        check(_abi.lib().ntc_cbloom_insert_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                  bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n)))
        self.n_inserted += int(n.value)
        return int(n.value)

    def query(self, bases, offsets, min_count=1):
        """-> (windows, hits): numpy uint32 [n_seqs] each, the k-mers of every sequence and those of them whose count is >= min_count"""
        import torch
        bases, off = self._input(bases, offsets)
        n_seqs = off.size - 1
        out = torch.empty((2, max(n_seqs, 1)), dtype=torch.int32, device=self.filter.device)
        check(_abi.lib().ntc_cbloom_query_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                 bases.data_ptr(), off.ctypes.data_as(C.c_void_p), n_seqs, self._min_count(min_count), out[0].data_ptr(),
                                                 out[1].data_ptr()))
        host = out[:, :n_seqs].cpu().numpy().view(np.uint32)
        return host[0].copy(), host[1].copy()

    def profile(self, bases, offsets):
        """-> numpy uint8 [offsets[-1] - offsets[0]]: byte p is the count of the k-mer that starts at position p, 0 where none starts"""
        import torch
        bases, off = self._input(bases, offsets)
        n = int(off[-1]) - int(off[0])
        out = torch.empty(max(n, 1), dtype=torch.uint8, device=self.filter.device)
        check(_abi.lib().ntc_cbloom_profile_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k, _STRANDS[self.strand],
                                                   bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, out.data_ptr()))
        return out[:n].cpu().numpy()

    def insert_hashes(self, h0):
        """Increments the n_hash counters of every given value h_0 (numpy uint64, or a 64-bit tensor on the device)"""
        d = self._hashes(h0)
        check(_abi.lib().ntc_cbloom_insert_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                         d.data_ptr() if d.numel() else None, d.numel()))
        self.n_inserted += d.numel()

    def counts_of_hashes(self, h0):
        """-> numpy uint8 [n]: the count of each given h_0"""
        import torch
        d = self._hashes(h0)
        counts = torch.empty(max(d.numel(), 1), dtype=torch.uint8, device=self.filter.device)
        check(_abi.lib().ntc_cbloom_query_hashes_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self.n_hash, self.k,
                                                        d.data_ptr() if d.numel() else None, d.numel(), counts.data_ptr()))
        return counts[: d.numel()].cpu().numpy()

    def hist(self):
        """-> numpy uint64 [256]: how many counters hold each value"""
        h = np.zeros(256, dtype=np.uint64)
        check(_abi.lib().ntc_cbloom_hist_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, h.ctypes.data_as(C.c_void_p)))
        return h

    def fpr(self, min_count=1):
        """(the counters >= min_count / m_bits) ** n_hash: the chance that a k-mer that was never inserted reads a count >= min_count"""
        h = self.hist()
        return (int(h[self._min_count(min_count):].sum()) / self.m_bits) ** self.n_hash

    def merge(self, other):
        """Adds another filter of the same shape into this one, counter by counter, saturating (shards of one input, peers' filters)"""
        if (other.m_bits, other.n_hash, other.k, other.strand) != (self.m_bits, self.n_hash, self.k, self.strand):
            raise ValueError("merge: the filters differ in m_bits, n_hash, k or strand")
        src = other.filter if other.device == self.device else other.filter.to(self.filter.device)
        check(_abi.lib().ntc_cbloom_add_device(self.device, self._stream(), self.filter.data_ptr(), src.data_ptr(), self.m_bits))
        self.n_inserted += other.n_inserted

    def counters(self):
        """The m_bits counters as numpy uint8"""
        return self.filter[: self.n_bytes].cpu().numpy()

    def threshold(self, min_count):
        """-> a BloomFilter of the same m_bits, n_hash, k and strand: the bit of a position is set iff its counter is >= min_count"""
        f = BloomFilter(self.m_bits, self.n_hash, self.k, self.strand, self.device)
        check(_abi.lib().ntc_cbloom_threshold_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, self._min_count(min_count), f.filter.data_ptr()))
        f.n_inserted = self.n_inserted
        return f

    def solid(self, bases, offsets, min_count, into):
        """Inserts into the BloomFilter `into` (its own m_bits and n_hash; this filter's k and strand) every k-mer of the sequences whose count here is
        >= min_count; -> the windows that passed"""
        if not isinstance(into, BloomFilter) or (into.k, into.strand, into.device) != (self.k, self.strand, self.device):
            raise ValueError("solid: `into` is a BloomFilter of this filter's k, strand and device")
        bases, off = self._input(bases, offsets)
        n = C.c_uint64(0)
        check(_abi.lib().ntc_bloom_insert_solid_device(self.device, self._stream(), into.filter.data_ptr(), into.m_bits, into.n_hash, self.filter.data_ptr(), self.m_bits,
                                                       self.n_hash, self._min_count(min_count), self.k, _STRANDS[self.strand], bases.data_ptr(),
                                                       off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n)))
        into.n_inserted += int(n.value)
        return int(n.value)

    def save(self, path):
        h = NtcBloomHeader(k=self.k, n_hash=self.n_hash, strand=_STRANDS[self.strand], reserved=0, m_bits=self.m_bits, n_inserted=self.n_inserted)
        image = np.ascontiguousarray(self.counters())
        check(_abi.lib().ntc_cbloom_write(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p)))

    @classmethod
    def load(cls, path, device=0):
        import torch
        h, image = read_counting_file(path)
        f = cls(h["m_bits"], h["n_hash"], h["k"], h["strand"], device)
        f.n_inserted = h["n_inserted"]
        f.filter[: f.n_bytes] = torch.from_numpy(image).to(f.filter.device)
        return f


def read_counting_file(path):
    """ntc_cbloom_read -> (header dict, the counters as numpy uint8): pure host"""
    h = NtcBloomHeader()
    L = _abi.lib()
    check(L.ntc_cbloom_read(str(path).encode(), C.byref(h), None, 0))
    image = np.zeros(h.m_bits, dtype=np.uint8)
    check(L.ntc_cbloom_read(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p), image.size))
    return {"k": h.k, "n_hash": h.n_hash, "strand": _STRAND_NAMES[h.strand], "m_bits": int(h.m_bits), "n_inserted": int(h.n_inserted)}, image
