"""Model of homopolymer compression (include/ntcard_hip.h: NTC_FLAG_HPC) in pure Python / numpy, and the sequences the tests compress.

class(b): A a -> 0, C c -> 1, G g -> 2, T t U u -> 3, every other byte none.  Within ONE sequence byte j is dropped iff j > 0 and class(b[j]) exists
and equals class(b[j - 1]); kept bytes keep value and order."""
import functools
import random

import numpy as np

from support import offsets_of

NONE = 255
CLASS = np.full(256, NONE, dtype=np.uint8)
for letters, c in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"TtUu", 3)):
    for b in letters:
        CLASS[b] = c


def compress(seq):
    """one sequence (bytes) -> its homopolymer-compressed form (bytes)"""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    if a.size == 0:
        return b""
    c = CLASS[a]
    keep = np.ones(a.size, dtype=bool)
    keep[1:] = ~((c[1:] != NONE) & (c[1:] == c[:-1]))
    return a[keep].tobytes()


def compress_slow(seq):
    """the definition, byte by byte (pins the vectorised form)"""
    out = bytearray()
    for j, b in enumerate(bytes(seq)):
        if j > 0 and CLASS[b] != NONE and CLASS[b] == CLASS[seq[j - 1]]:
            continue
        out.append(b)
    return bytes(out)


def model(seqs):
    return [compress(s) for s in seqs]


def compress_many(buf, offsets):
    """the sequences [offsets[i], offsets[i + 1]) of buf (uint8 array) in ONE vectorised pass -> (their compressed forms behind one another, the new
    offsets from 0): the keep rule over the whole concatenation, with every sequence's first byte forced to "kept" (a run never continues across a
    boundary).  For inputs of megabytes and of hundreds of thousands of sequences; tests/test_hpc_host.py pins it to compress() per sequence"""
    offs = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    a = np.asarray(buf, dtype=np.uint8)[offs[0]:offs[-1]]
    c = CLASS[a]
    keep = np.ones(a.size, dtype=bool)
    keep[1:] = ~((c[1:] != NONE) & (c[1:] == c[:-1]))
    starts = offs[:-1] - offs[0]
    keep[starts[starts < a.size]] = True  # (empty sequences at the very end start nowhere)
    pre = np.zeros(a.size + 1, dtype=np.uint64)
    np.cumsum(keep, dtype=np.uint64, out=pre[1:])
    return a[keep], pre[offs - offs[0]]


def runs_seq(rng, n, p_more=0.5, p_low=0.1, p_other=0.01):
    """about n bytes: runs of one base whose length is geometric (P(one more) = p_more), case flips inside, now and then a byte without a class"""
    out = bytearray()
    while len(out) < n:
        if rng.random() < p_other:
            out += rng.choice([b"N", b"n", b"R", b"\r", b"\x01", b"\x03", b"NN"])
            continue
        base = rng.choice("ACGTU")
        while True:
            out.append(ord(base.lower() if rng.random() < p_low else base))
            if rng.random() >= p_more:
                break
    return bytes(out[:n])


STRADDLE = (4, 64, 256, 4096)  # the dword, a wave's step, (64 lanes x 4 B) and a wave's chunk of the compaction kernels


def straddle_seq():
    """runs of three that begin 2, 1 bytes in front of, on, and 1 byte behind a buffer position that is a multiple of 4 / 64 / 256 / 4096, for every lead
    0 .. 3 in front of this sequence (it comes FIRST: byte j sits at buffer position lead + j); no other run in it"""
    targets = [(4, 100 + 12 * i) for i in range(16)] + [(64, 64 * (5 + i)) for i in range(16)] + [(256, 256 * (6 + i)) for i in range(16)] + \
              [(4096, 4096 * (2 + i)) for i in range(16)]
    n = 4096 * 18 + 40
    s = bytearray(b"ACGT" * (n // 4))
    for (B, t), (lead, d) in zip(targets, [(lead, d) for lead in range(4) for d in (-2, -1, 0, 1)] * 4):
        assert t % B == 0
        j = t - lead + d
        x = next(c for c in b"ACGT" if c != s[j - 1] and c != s[j + 3])
        s[j:j + 3] = bytes([x, x | 0x20 if d == 0 else x, x])
    return bytes(s)


@functools.lru_cache(maxsize=None)
def device_set():
    """the sequences of the GPU tests (tests/test_hpc_gpu.py lists what they hold), a few hundred KB"""
    rng = random.Random(2024)
    flips = bytes(rng.choice(b"AAAa") for _ in range(70_000))
    seqs = [
        straddle_seq(),
        b"", b"A",
        b"GATTCCCA", b"AGGTC",                      # neighbours that end and begin with the same base: both bytes are kept
        b"CG" + flips + b"TC",                      # a run of 70 000 x A, longer than any workgroup's block
        b"GTUGtUGaAGUTCuTg",                        # TU, tU and aA pairs
        b"ACGT" * 20 + b"N" * 70 + b"GGCA" * 20,    # an N run longer than a piece of 48
        b"ACRRGT\r\rAC\x01\x01G\x03\x03TT\x04\x04\x05\x05\x07\x07A" * 5,
        b"TtUu" * 50,                               # compresses to one byte
        b"", b"",
    ]
    seqs += [runs_seq(rng, rng.randrange(1, 401)) for _ in range(40)]
    seqs.append(runs_seq(rng, 300_000))
    seqs += [b"C", b""]                             # (an empty sequence at the very end starts nowhere)
    return tuple(seqs)


SLOT_BYTES = (1, 3, 4, 5, 7)  # bases to the reference's seed table (nthash.hpp:32), without a class here; no sequence parser produces them


@functools.lru_cache(maxsize=None)
def engine_set():
    """device_set() with the bytes 1, 3, 4, 5, 7 replaced by letters that are no bases either (N R Y K M): the same runs, the same compressed lengths.
    The general kernel K1 takes those five bytes for non-bases where the reference's seed table — and so tests/orc.py — takes them for bases, with or
    without homopolymer compression, so the counts of sequences that hold them are not the oracle's on any route through K1 (row slots, remainders).
    The compaction is tested on device_set() itself; the counting on this set, and on slot_piece_set() where the tiled kernels alone see such bytes."""
    table = bytes.maketrans(bytes(SLOT_BYTES), b"NRYKM")
    return tuple(s.translate(table) for s in device_set())


def slot_piece_set(k=32, piece_len=48):
    """sequences whose bytes 1 and 3 lie in front of the remainder of the cut (ntc_long_plan): every window that holds one belongs to a full piece, which the
    tiled kernels count as the reference does"""
    rng = random.Random(77)
    step = piece_len - k + 1
    out = []
    for m in (1, 2, 7, 300):
        n = piece_len + (m - 1) * step + rng.randrange(0, step)
        s = bytearray(runs_seq(rng, 3 * n, p_other=0.0))  # (compresses to about n: trimmed below)
        s = bytearray(compress(bytes(s))[:n])
        assert len(s) == n and (n - piece_len) // step + 1 == m
        for _ in range(1 + m // 3):
            j = rng.randrange(0, m * step)
            s[j] = rng.choice((1, 3))
        # (s is compressed: stretch every base into a run of 1 .. 3 again, so that the model gives s back)
        out.append(b"".join(bytes([b]) * (rng.randrange(1, 4) if CLASS[b] != NONE else 1) for b in s))
        assert compress(out[-1]) == bytes(s)
    return tuple(out)


# ---- inputs beyond the compaction kernels' thresholds (tests/test_hpc_gpu.py; ntc_hpc.hip) ----
CHUNK = 4096          # positions of a wave's chunk (kHpcChunk)
SCAN_THREADS = 1024   # hpc_scan_kernel: one workgroup; thread t sums `per` = ceil(chunks / 1024) chunks
SEQ_THREADS = 2048 * 256  # hpc_mark_kernel / hpc_offsets_kernel: at most 2048 workgroups of 256 threads, a thread per offset and turn


def chunks_of(lead, n):
    """chunks of a compaction of n bytes whose first byte sits `lead` bytes behind an aligned dword (launch_hpc_compact)"""
    words = (lead + n + 3) // 4
    return (words + CHUNK // 4 - 1) // (CHUNK // 4)


def runs_array(gen, n, p_more=0.5, p_low=0.1, p_other=0.01):
    """runs_seq in numpy, for megabytes: n bytes (uint8 array) of runs of one base with a geometric length, case flips inside, bytes without a class"""
    base = np.frombuffer(b"ACGTU", dtype=np.uint8)[gen.integers(0, 5, size=n)]
    a = np.repeat(base, gen.geometric(1.0 - p_more, size=n))[:n].copy()
    a[gen.random(n) < p_low] |= 0x20
    other = np.flatnonzero(gen.random(n) < p_other)
    a[other] = np.frombuffer(b"NnR\r\x01\x03", dtype=np.uint8)[gen.integers(0, 6, size=other.size)]
    assert a.size == n
    return a


@functools.lru_cache(maxsize=None)
def pair_seq():
    """one sequence that holds every ordered pair of byte values: (a, b) for a, b = 0 .. 255 behind one another, 131072 bytes"""
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    b = np.tile(np.arange(256, dtype=np.uint8), 256)
    s = np.stack([a, b], axis=1).reshape(-1)
    return s, np.array([0, s.size], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def pair_seqs():
    """the same pairs as 65536 sequences of two bytes"""
    return pair_seq()[0], np.arange(65537, dtype=np.uint64) * np.uint64(2)


def pair_want():
    """what the definition leaves of the pair (a, b) as a sequence of its own, for every pair: a alone iff b repeats a's class -> (bytes, offsets)"""
    s = pair_seq()[0].reshape(-1, 2)
    drop = (CLASS[s[:, 1]] != NONE) & (CLASS[s[:, 1]] == CLASS[s[:, 0]])
    keep = np.ones(s.shape, dtype=bool)
    keep[:, 1] = ~drop
    return s[keep], offsets_of(2 - drop.astype(np.int64))


@functools.lru_cache(maxsize=None)
def many_short():
    """530 000 sequences of 0 .. 20 bytes over ACGTacgtUuNR, 5.3 MB: more sequences than the mark and offsets kernels have threads, more chunks than the scan
    kernel has threads"""
    gen = np.random.default_rng(530)
    offs = offsets_of(gen.integers(0, 21, size=530_000))
    return np.frombuffer(b"ACGTacgtUuNR", dtype=np.uint8)[gen.integers(0, 12, size=int(offs[-1]))], offs


@functools.lru_cache(maxsize=None)
def three_seqs(total):
    """three sequences of `total` bytes in all; a run of G / g covers the last 5000 bytes and the join of the second and the third sequence 2000 bytes
    in front of the end (the byte behind the join is kept, the rest of the run is not)"""
    gen = np.random.default_rng(total % 1000)
    a = runs_array(gen, total)
    a[total - 5000:] = np.frombuffer(b"GGGg", dtype=np.uint8)[gen.integers(0, 4, size=5000)]
    return a, np.array([0, 1_500_000, total - 2000, total], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def few_large():
    """about 8.5 MiB in four sequences"""
    gen = np.random.default_rng(85)
    lens = [3_000_001, 2_500_003, 7, 3_412_000]
    return runs_array(gen, sum(lens)), offsets_of(lens)
