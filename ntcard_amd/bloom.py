"""Bloom filters of every k-mer on the device (include/ntcard_hip.h: ntc_bloom_*; DESIGN.md §4 "Bloom filters"): the step behind ntCard's F0 — and
counting filters (ntc_cbloom_*; DESIGN.md §4 "Counting filters and solid k-mers"): the step behind its f_i, k-mer counts and the filter of the solid k-mers.

The layout is the reference's vendor/ntHash/lib/BloomFilter.hpp — position h_i % m, bit 7 - loc % 8 of byte loc / 8, h_i the multi-hash of
nthash.hpp:381-390 — so `BloomFilter.bytes()` is what `storeFilter` writes.  BlockedBloomFilter (ntc_bbloom_*; DESIGN.md §4 "Blocked filters") is a
second kind beside it, in a layout of its own: every bit of a k-mer in one 64-byte block.  torch is plumbing only: it owns the filter's device memory.

The three kinds are siblings under one private base, _DeviceFilter, which holds what they share; a kind states its entry points' prefix, its rule for
m_bits, its size function, the bytes of its image and its file's `reserved` as class attributes.
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


def _offsets(offsets):
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("offsets: a 1-d array of n_seqs + 1 values")
    return off


def _min_count(min_count):
    min_count = int(min_count)
    if not 1 <= min_count <= 255:
        raise ValueError(f"min_count={min_count} outside 1 .. 255")
    return min_count


class _DeviceFilter:
    """What the three kinds of filter share: m_bits positions on one device, n_hash of them per k-mer, the k-mers' values taken as an Engine of that
    strand takes them.

    insert / query take a torch uint8 tensor of bases on the filter's device and HOST offsets (n_seqs + 1, non-decreasing; sequence i is
    bases[offsets[i]:offsets[i + 1]]), the layout of Engine.submit_long_device."""

    # the kind: every public class states these
    _prefix = None               # its entry points are ntc_<prefix>_insert_device, _query_device, _insert_hashes_device, _query_hashes_device, _write, _read
    _merge_call = None           # the entry point that merges two images of the kind
    _size = None                 # m_bits for n distinct k-mers at a false positive rate
    _reserved = 0                # the file header's `reserved`, and the name it has in the header dict of the reader (None: not shown)
    _reserved_name = None

    @staticmethod
    def _m_error(m_bits):
        """What is wrong with m_bits, or None"""
        return None if 1 <= m_bits < 1 << 40 else f"m_bits={m_bits} outside 1 .. 2^40 - 1"

    @staticmethod
    def _image_bytes(m_bits):
        """The bytes of the kind's image"""
        raise NotImplementedError

    def __init__(self, m_bits, n_hash, k, strand="canonical", device=0):
        import torch
        if strand not in _STRANDS:
            raise ValueError(f"strand must be 'canonical', 'forward' or 'reverse', not {strand!r}")
        m_bits, n_hash, k = int(m_bits), int(n_hash), int(k)
        if self._m_error(m_bits):
            raise ValueError(self._m_error(m_bits))
        if not 1 <= n_hash <= 32:
            raise ValueError(f"n_hash={n_hash} outside 1 .. 32")
        if not 1 <= k <= _abi.lib().ntc_max_k():
            raise ValueError(f"k={k} outside 1 .. {_abi.lib().ntc_max_k()}")
        self.m_bits, self.n_hash, self.k, self.strand, self.device = m_bits, n_hash, k, strand, int(device)
        self.n_inserted = 0
        self.n_bytes = self._image_bytes(m_bits)
        self.filter = torch.zeros((self.n_bytes + 3) // 4 * 4, dtype=torch.uint8, device=f"cuda:{self.device}")

    @classmethod
    def for_distinct(cls, n, fpr, n_hash, k, strand="canonical", device=0):
        """A filter sized by the kind's size function (ntc_bloom_size; a blocked filter: ntc_bbloom_size) for n distinct k-mers at false positive rate
        fpr — for a counting filter the rate at which a k-mer that was never inserted reads a count >= 1.  n is what ntCard estimates: the F0 that
        `estimate(p_hist, r_bits, s_bits)` returns for the value histogram of `Engine.finish()` — or the F0 line of the `.hist` file."""
        return cls(cls._size(n, fpr, n_hash), n_hash, k, strand, device)

    def _call(self, name, *args):
        """ntc_<prefix>_<name> on this filter: device, stream, filter, m_bits, then `args`"""
        check(getattr(_abi.lib(), f"ntc_{self._prefix}_{name}")(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, *args))

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _bases(self, bases):
        import torch
        if not isinstance(bases, torch.Tensor) or bases.dtype != torch.uint8 or not bases.is_cuda or bases.device.index != self.device or not bases.is_contiguous():
            raise ValueError("bases: a contiguous torch uint8 tensor on the filter's device")
        return bases

    def _input(self, bases, offsets):
        off = _offsets(offsets)
        bases = self._bases(bases)
        if int(off[-1]) > bases.numel():
            raise ValueError("offsets reach behind the end of bases")
        return bases, off

    def _hashes(self, h0):
        import torch
        if isinstance(h0, torch.Tensor):
            if h0.dtype not in (torch.int64, torch.uint64) or not h0.is_cuda or h0.device.index != self.device or not h0.is_contiguous():
                raise ValueError("hashes: a contiguous 64-bit torch tensor on the filter's device, or a numpy array")
            return h0
        return torch.from_numpy(np.ascontiguousarray(h0, dtype=np.uint64).view(np.int64)).to(self.filter.device)

    def insert(self, bases, offsets):
        """Inserts every k-mer of the sequences (a counting filter: counts it); -> the windows inserted"""
        bases, off = self._input(bases, offsets)
        n = C.c_uint64(0)
        self._call("insert_device", self.n_hash, self.k, _STRANDS[self.strand], bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n))
        self.n_inserted += int(n.value)
        return int(n.value)

    def query(self, bases, offsets):
        """-> (windows, hits): numpy uint32 [n_seqs] each, the k-mers of every sequence and those of them the filter holds"""
        return self._query(*self._input(bases, offsets))

    def _query(self, bases, off, *extra):
        """The kind's query over a checked input; `extra`: what the kind's entry point takes between n_seqs and the outputs"""
        import torch
        n_seqs = off.size - 1
        out = torch.empty((2, max(n_seqs, 1)), dtype=torch.int32, device=self.filter.device)
        self._call("query_device", self.n_hash, self.k, _STRANDS[self.strand], bases.data_ptr(), off.ctypes.data_as(C.c_void_p), n_seqs, *extra, out[0].data_ptr(),
                   out[1].data_ptr())
        host = out[:, :n_seqs].cpu().numpy().view(np.uint32)
        return host[0].copy(), host[1].copy()

    def insert_hashes(self, h0):
        """Inserts every given value h_0 (numpy uint64, or a 64-bit tensor on the device) — a signature's hashes, say: sets its n_hash bits, or
        increments its n_hash counters"""
        d = self._hashes(h0)
        self._call("insert_hashes_device", self.n_hash, self.k, d.data_ptr() if d.numel() else None, d.numel())
        self.n_inserted += d.numel()

    def _answers(self, h0):
        """-> numpy uint8 [n]: what the kind's query answers for each given h_0 (a bit kind: 0 / 1; a counting filter: the count)"""
        import torch
        d = self._hashes(h0)
        out = torch.empty(max(d.numel(), 1), dtype=torch.uint8, device=self.filter.device)
        self._call("query_hashes_device", self.n_hash, self.k, d.data_ptr() if d.numel() else None, d.numel(), out.data_ptr())
        return out[: d.numel()].cpu().numpy()

    def merge(self, other):
        """Merges another filter of the same kind and shape into this one (shards of one input, peers' filters): ORs a bit image, adds counters, saturating"""
        if type(other) is not type(self):
            raise ValueError(f"merge: the other filter is a {type(other).__name__}, not a {type(self).__name__}")
        if (other.m_bits, other.n_hash, other.k, other.strand) != (self.m_bits, self.n_hash, self.k, self.strand):
            raise ValueError("merge: the filters differ in m_bits, n_hash, k or strand")
        src = other.filter if other.device == self.device else other.filter.to(self.filter.device)
        check(getattr(_abi.lib(), self._merge_call)(self.device, self._stream(), self.filter.data_ptr(), src.data_ptr(), self.m_bits))
        self.n_inserted += other.n_inserted

    def _image(self):
        return self.filter[: self.n_bytes].cpu().numpy()

    def save(self, path):
        h = NtcBloomHeader(k=self.k, n_hash=self.n_hash, strand=_STRANDS[self.strand], reserved=self._reserved, m_bits=self.m_bits, n_inserted=self.n_inserted)
        image = np.ascontiguousarray(self._image())
        check(getattr(_abi.lib(), f"ntc_{self._prefix}_write")(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p)))

    @classmethod
    def load(cls, path, device=0):
        import torch
        h, image = _read_file(cls, path)
        f = cls(h["m_bits"], h["n_hash"], h["k"], h["strand"], device)
        f.n_inserted = h["n_inserted"]
        f.filter[: f.n_bytes] = torch.from_numpy(image).to(f.filter.device)
        return f


def _read_file(kind, path):
    """ntc_<prefix>_read of the kind -> (header dict, the image as numpy uint8): pure host"""
    h = NtcBloomHeader()
    read = getattr(_abi.lib(), f"ntc_{kind._prefix}_read")
    check(read(str(path).encode(), C.byref(h), None, 0))
    image = np.zeros(kind._image_bytes(h.m_bits), dtype=np.uint8)
    check(read(str(path).encode(), C.byref(h), image.ctypes.data_as(C.c_void_p), image.size))
    header = {"k": h.k, "n_hash": h.n_hash, "strand": _STRAND_NAMES[h.strand], "m_bits": int(h.m_bits), "n_inserted": int(h.n_inserted)}
    if kind._reserved_name:
        header[kind._reserved_name] = int(h.reserved)
    return header, image


def _insert_solid(into, counting, bases, offsets, min_count):
    """ntc_<into's prefix>_insert_solid_device: every k-mer of the sequences whose count in `counting` is >= min_count goes into `into`"""
    bases, off = into._input(bases, offsets)
    n = C.c_uint64(0)
    into._call("insert_solid_device", into.n_hash, counting.filter.data_ptr(), counting.m_bits, counting.n_hash, _min_count(min_count), into.k, _STRANDS[into.strand],
               bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, C.byref(n))
    into.n_inserted += int(n.value)
    return int(n.value)


class _BitFilter(_DeviceFilter):
    """What the two kinds with a bit image share: the image is an ordinary one in the plain filter's bit rule, so popcount and merge are one call each"""
    _merge_call = "ntc_bloom_or_device"

    def query_hashes(self, h0):
        """-> numpy bool [n]: whether all n_hash bits of each given h_0 are set"""
        return self._answers(h0).astype(bool)

    def popcount(self):
        pop = C.c_uint64(0)
        check(_abi.lib().ntc_bloom_popcount_device(self.device, self._stream(), self.filter.data_ptr(), self.m_bits, C.byref(pop)))
        return int(pop.value)

    def bytes(self):
        """The byte image (a plain filter: the reference's, (m_bits + 7) // 8 bytes) as numpy uint8"""
        return self._image()


class BloomFilter(_BitFilter):
    """A Bloom filter of m_bits bits on one device, n_hash positions per k-mer, in the reference's layout."""
    _prefix = "bloom"
    _size = staticmethod(bloom_size)

    @staticmethod
    def _image_bytes(m_bits):
        return (m_bits + 7) // 8

    def fpr(self):
        """(popcount / m_bits) ** n_hash: the chance that a k-mer that was never inserted finds all its bits set"""
        return (self.popcount() / self.m_bits) ** self.n_hash


def read_file(path):
    """ntc_bloom_read -> (header dict, the byte image as numpy uint8): pure host"""
    return _read_file(BloomFilter, path)


class BlockedBloomFilter(_BitFilter):
    """A BLOCKED Bloom filter of m_bits bits (a multiple of 512) on one device: all n_hash bits of a k-mer lie in one aligned 512-bit block — one random
    cache line per k-mer where BloomFilter fetches n_hash — at the price of a somewhat larger filter for the same false positive rate (bbloom_size) and
    of a format of its own (include/ntcard_hip.h: ntc_bbloom_*).  Constructor, inputs and streams as BloomFilter's; write / read are save / load."""
    _prefix = "bbloom"
    _size = staticmethod(bbloom_size)
    _reserved = BBLOOM_BLOCK_BITS
    _reserved_name = "block_bits"

    @staticmethod
    def _m_error(m_bits):
        ok = BBLOOM_BLOCK_BITS <= m_bits < 1 << 40 and m_bits % BBLOOM_BLOCK_BITS == 0
        return None if ok else f"m_bits={m_bits} is no multiple of 512 in 512 .. 2^40 - 512"

    @staticmethod
    def _image_bytes(m_bits):
        return m_bits // 8

    def __init__(self, m_bits, n_hash, k, strand="canonical", device=0):
        super().__init__(m_bits, n_hash, k, strand, device)
        self.n_blocks = self.m_bits // BBLOOM_BLOCK_BITS

    def insert_solid(self, counting, bases, offsets, min_count):
        """Inserts every k-mer of the sequences whose count in the CountingBloomFilter `counting` (this filter's k, strand and device) is >= min_count;
        -> the windows that passed"""
        if not isinstance(counting, CountingBloomFilter) or (counting.k, counting.strand, counting.device) != (self.k, self.strand, self.device):
            raise ValueError("insert_solid: `counting` is a CountingBloomFilter of this filter's k, strand and device")
        return _insert_solid(self, counting, bases, offsets, min_count)

    def block_hist(self):
        """-> numpy uint64 [513]: how many blocks hold 0, 1, .. 512 set bits"""
        h = np.zeros(BBLOOM_BLOCK_BITS + 1, dtype=np.uint64)
        self._call("hist_device", h.ctypes.data_as(C.c_void_p))
        return h

    def fpr(self):
        """sum_v hist[v] (v / 512)^n_hash / n_blocks: the chance that a k-mer that was never inserted finds all its bits set — per block, not from the
        overall popcount: a block fuller than the average answers wrongly more often than the average says"""
        h = self.block_hist()
        v = np.arange(BBLOOM_BLOCK_BITS + 1, dtype=np.float64) / BBLOOM_BLOCK_BITS
        return float((h.astype(np.float64) * v ** self.n_hash).sum() / self.n_blocks)

    def write(self, path):
        """save, under the name this kind had first"""
        self.save(path)

    @classmethod
    def read(cls, path, device=0):
        """load, under the name this kind had first"""
        return cls.load(path, device)


def read_blocked_file(path):
    """ntc_bbloom_read -> (header dict, the byte image as numpy uint8): pure host"""
    return _read_file(BlockedBloomFilter, path)


class CountingBloomFilter(_DeviceFilter):
    """A counting Bloom filter of m_bits 8-bit counters on one device (m_bits: the NUMBER OF COUNTERS, the name BloomFilter uses for its positions): an
    insert adds one to each of a k-mer's n_hash counters, saturating at 255; the count of a k-mer is the minimum of its counters.  Constructor, inputs and
    streams as BloomFilter's."""
    _prefix = "cbloom"
    _merge_call = "ntc_cbloom_add_device"
    _size = staticmethod(bloom_size)

    @staticmethod
    def _image_bytes(m_bits):
        return m_bits

    def query(self, bases, offsets, min_count=1):
        """-> (windows, hits): numpy uint32 [n_seqs] each, the k-mers of every sequence and those of them whose count is >= min_count"""
        bases, off = self._input(bases, offsets)
        return self._query(bases, off, _min_count(min_count))

    def profile(self, bases, offsets):
        """-> numpy uint8 [offsets[-1] - offsets[0]]: byte p is the count of the k-mer that starts at position p, 0 where none starts"""
        import torch
        bases, off = self._input(bases, offsets)
        n = int(off[-1]) - int(off[0])
        out = torch.empty(max(n, 1), dtype=torch.uint8, device=self.filter.device)
        self._call("profile_device", self.n_hash, self.k, _STRANDS[self.strand], bases.data_ptr(), off.ctypes.data_as(C.c_void_p), off.size - 1, out.data_ptr())
        return out[:n].cpu().numpy()

    def counts_of_hashes(self, h0):
        """-> numpy uint8 [n]: the count of each given h_0"""
        return self._answers(h0)

    def hist(self):
        """-> numpy uint64 [256]: how many counters hold each value"""
        h = np.zeros(256, dtype=np.uint64)
        self._call("hist_device", h.ctypes.data_as(C.c_void_p))
        return h

    def fpr(self, min_count=1):
        """(the counters >= min_count / m_bits) ** n_hash: the chance that a k-mer that was never inserted reads a count >= min_count"""
        h = self.hist()
        return (int(h[_min_count(min_count):].sum()) / self.m_bits) ** self.n_hash

    def counters(self):
        """The m_bits counters as numpy uint8"""
        return self._image()

    def threshold(self, min_count):
        """-> a BloomFilter of the same m_bits, n_hash, k and strand: the bit of a position is set iff its counter is >= min_count"""
        f = BloomFilter(self.m_bits, self.n_hash, self.k, self.strand, self.device)
        self._call("threshold_device", _min_count(min_count), f.filter.data_ptr())
        f.n_inserted = self.n_inserted
        return f

    def solid(self, bases, offsets, min_count, into):
        """Inserts into the BloomFilter `into` (its own m_bits and n_hash; this filter's k and strand) every k-mer of the sequences whose count here is
        >= min_count; -> the windows that passed"""
        if not isinstance(into, BloomFilter) or (into.k, into.strand, into.device) != (self.k, self.strand, self.device):
            raise ValueError("solid: `into` is a BloomFilter of this filter's k, strand and device")
        return _insert_solid(into, self, bases, offsets, min_count)


def read_counting_file(path):
    """ntc_cbloom_read -> (header dict, the counters as numpy uint8): pure host"""
    return _read_file(CountingBloomFilter, path)
