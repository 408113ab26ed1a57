"""Model of one-strand counting (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE) built from the oracle's primitives:
per read, every window of k bases -> fh, rh (orc_window_hash; under a mask the don't-care terms XORed out with orc_srol(orc_seed(b), k-1-i) /
orc_srol(orc_seed_comp(b), i), nthash.hpp:641-646), the strand's pick, ntComp (ntcard.cpp:132-145) -> t_Counter, F1.
window_values makes one ctypes call per window: keep its inputs small.  window_blocks / array_sketches are the array form for equal-length reads
(table look-ups over arr[n, L] in row blocks; tests/test_strand_host.py pins it to window_values window by window): millions of short reads."""
import ctypes as C
import functools
import random

import numpy as np

import orc
from support import GOLD, gap_mask, mask_with, masks_for, nt_comp, rseq, sketch_from_values, small_reads  # noqa: F401  (re-exported: sm.GOLD, sm.masks_for, ...)

CANONICAL, FORWARD, REVERSE = 0, 1, 2
STRANDS = {"canonical": CANONICAL, "forward": FORWARD, "reverse": REVERSE}


def window_values(seq, mask):
    """-> (fs u64[n], rs u64[n], pos u32[n]): forward and reverse value of every window of len(mask) bases of the read, in window order;
    mask: '0' / '1' per window offset ('1' * k: plain k-mers)"""
    L = orc.lib()
    k = len(mask)
    dc = [i for i, c in enumerate(mask) if c == "0"]
    fs, rs, pos = [], [], []
    fh, rh, bad = C.c_uint64(), C.c_uint64(), C.c_uint()
    for p in range(0, len(seq) - k + 1):
        w = seq[p:p + k]
        if not L.orc_window_hash(w, k, C.byref(fh), C.byref(rh), C.byref(bad)):
            continue
        f, r = fh.value, rh.value
        for i in dc:
            f ^= L.orc_srol(L.orc_seed(w[i]), k - 1 - i)
            r ^= L.orc_srol(L.orc_seed_comp(w[i]), i)
        fs.append(f)
        rs.append(r)
        pos.append(p)
    return np.array(fs, dtype=np.uint64), np.array(rs, dtype=np.uint64), np.array(pos, dtype=np.uint32)


# ---- the array form: equal-length reads arr[n, L], table look-ups instead of one ctypes call per window ----
@functools.lru_cache(maxsize=None)
def base_table():
    """bool[256]: the bytes the oracle takes for a base (orc_window_hash over the one-byte window)"""
    L = orc.lib()
    fh, rh, bad = C.c_uint64(), C.c_uint64(), C.c_uint()
    return np.array([bool(L.orc_window_hash(bytes([b]), 1, C.byref(fh), C.byref(rh), C.byref(bad))) for b in range(256)])


@functools.lru_cache(maxsize=None)
def offset_tables(mask):
    """[(i, F_i, R_i)] per '1' offset i of the mask: F_i[c] = orc_srol(orc_seed(c), k-1-i), R_i[c] = orc_srol(orc_seed_comp(c), i), uint64[256] each"""
    L = orc.lib()
    k = len(mask)
    out = []
    for i, m in enumerate(mask):
        if m == "0":
            continue
        out.append((i, np.array([L.orc_srol(L.orc_seed(c), k - 1 - i) for c in range(256)], dtype=np.uint64),
                    np.array([L.orc_srol(L.orc_seed_comp(c), i) for c in range(256)], dtype=np.uint64)))
    return out


def window_blocks(arr, mask, rows=1 << 16):
    """arr uint8[n, L] -> per block of `rows` reads (fs, rs, ok), each [rows, L - k + 1] in window order: the forward and the reverse value of every
    window and whether it is one (no non-base byte at any of its k offsets, the mask's '0' ones included); fs, rs mean nothing where ok is False"""
    n, L = arr.shape
    k = len(mask)
    nwin = L - k + 1
    if nwin <= 0:
        return
    tabs, base = offset_tables(mask), base_table()
    for r0 in range(0, n, rows):
        a = arr[r0:r0 + rows]
        fs = np.zeros((a.shape[0], nwin), dtype=np.uint64)
        rs = np.zeros((a.shape[0], nwin), dtype=np.uint64)
        for i, F, R in tabs:
            w = a[:, i:i + nwin]
            fs ^= F[w]
            rs ^= R[w]
        bad = np.zeros((a.shape[0], L + 1), dtype=np.int32)
        np.cumsum(~base[a], axis=1, out=bad[:, 1:])
        yield fs, rs, bad[:, k:] == bad[:, :nwin]


def array_window_values(arr, mask):
    """(fs, rs, ok), each [n, L - k + 1], of all reads at once (small inputs; window_blocks for large ones)"""
    parts = list(window_blocks(arr, mask))
    if not parts:
        z = np.zeros((arr.shape[0], 0), dtype=np.uint64)
        return z, z.copy(), z.astype(bool)
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def array_sketches(arr, mask, configs):
    """{(strand, r_bits, s_bits): (t_Counter [1][2][1 << r_bits] uint16, F1 [1])} for every configuration, in one pass over the reads"""
    cnt = {c: np.zeros(2 << c[1], dtype=np.int64) for c in configs}
    f1 = 0
    for fs, rs, ok in window_blocks(arr, mask):
        f1 += int(ok.sum())
        vals = {}
        for c in configs:
            strand, r_bits, s_bits = c
            if strand not in vals:
                vals[strand] = pick(fs[ok], rs[ok], strand)
            sample, index = nt_comp(vals[strand], r_bits, s_bits)
            keep = sample < 2
            cnt[c] += np.bincount((sample[keep].astype(np.int64) << r_bits) + index[keep], minlength=2 << r_bits)
    return {c: (cnt[c].astype(np.uint16).reshape(1, 2, 1 << c[1]), np.array([f1], dtype=np.uint64)) for c in configs}


def pad_reads(reads, L=None, fill=ord("#")):
    """reads of any lengths -> uint8[n, L] with a non-base byte behind every read's end: window_blocks then yields exactly the reads' own windows"""
    L = max(len(r) for r in reads) if L is None else L
    arr = np.full((len(reads), L), fill, dtype=np.uint8)
    for i, r in enumerate(reads):
        arr[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return arr


def pick(fs, rs, strand):
    if strand == FORWARD:
        return fs
    if strand == REVERSE:
        return rs
    return np.minimum(fs, rs)  # rh < fh ? rh : fh (nthash.hpp:275-279)


def strand_hash(seq, mask, strand):
    fs, rs, _ = window_values(seq, mask)
    return pick(fs, rs, strand)


def values_of(reads, masks):
    """[(fs, rs)] per mask over all reads, to be pushed through sketch_of for several strands"""
    out = []
    for m in masks:
        v = [window_values(r, m) for r in reads]
        out.append((np.concatenate([x[0] for x in v]) if v else np.zeros(0, np.uint64), np.concatenate([x[1] for x in v]) if v else np.zeros(0, np.uint64)))
    return out


def sketch_of(values, strand, r_bits, s_bits):
    """ntComp over the strand's values: t_Counter [n][2][1 << r_bits] (uint16, as the engine reports it), F1 [n]"""
    return sketch_from_values([pick(fs, rs, strand) for fs, rs in values], r_bits, s_bits)


def model_sketch(reads, masks, strand, r_bits, s_bits):
    return sketch_of(values_of(reads, masks), strand, r_bits, s_bits)


def revcomp(seq):
    return seq.translate(bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa"))[::-1]


# ---- the read sets and configurations of tests/test_strand_gpu.py's sketch tests (tests/test_strand_host.py asserts they tell the strands apart) ----
def sketch_reads_equal(n=320, L=150, seed=21):
    rng = random.Random(seed)
    return [rseq(rng, L, pn=rng.choice([0.0, 0.0, 0.004])) for _ in range(n)]


def sketch_reads_ragged(n=320, seed=22):
    rng = random.Random(seed)
    return [rseq(rng, rng.randint(145, 160), pn=rng.choice([0.0, 0.0, 0.004])) for _ in range(n)]


SEED_MASKS = ["1110011100111", "0" + "1" * 30 + "0", "1" * 24, ("01" * 20)[:39] + "1"]
# (name, masks, gap for Engine(..., gap=), s_bits): single k, a fused list across K1h's range, the two -g seeds, a list of masks
SKETCH_CONFIGS = [
    ("k32", ["1" * 32], 0, 7),
    ("k32_dense", ["1" * 32], 0, 3),
    ("k64", ["1" * 64], 0, 4),
    ("klist", ["1" * 16, "1" * 24, "1" * 32, "1" * 48], 0, 4),
    ("gap12_2", [gap_mask(12, 2)], 2, 3),
    ("gap32_8", [gap_mask(32, 8)], 8, 7),
    ("seeds", SEED_MASKS, -1, 4),
]
R_BITS = 14
