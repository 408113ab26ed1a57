"""Model of one-strand counting (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE) built from the oracle's primitives:
per read, every window of k bases -> fh, rh (orc_window_hash; under a mask the don't-care terms XORed out with orc_srol(orc_seed(b), k-1-i) /
orc_srol(orc_seed_comp(b), i), nthash.hpp:641-646), the strand's pick, ntComp (ntcard.cpp:132-145) -> t_Counter, F1.
One ctypes call per window: keep the inputs small."""
import ctypes as C
import gzip
import os
import random

import numpy as np

import orc

CANONICAL, FORWARD, REVERSE = 0, 1, 2
STRANDS = {"canonical": CANONICAL, "forward": FORWARD, "reverse": REVERSE}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    tc = np.zeros((len(values), 2, 1 << r_bits), dtype=np.uint16)
    f1 = np.zeros(len(values), dtype=np.uint64)
    s_mask = np.uint64((1 << (s_bits - 1)) - 1)
    for mi, (fs, rs) in enumerate(values):
        h = pick(fs, rs, strand)
        f1[mi] = h.size
        s0 = (h >> np.uint64(63 - s_bits)) == np.uint64(1)
        s1 = (h >> np.uint64(64 - s_bits)) == s_mask
        sample = np.where(s1, 1, np.where(s0, 0, 2))
        keep = sample < 2
        np.add.at(tc[mi], (sample[keep], (h[keep] & np.uint64((1 << r_bits) - 1)).astype(np.int64)), np.uint16(1))
    return tc, f1


def model_sketch(reads, masks, strand, r_bits, s_bits):
    return sketch_of(values_of(reads, masks), strand, r_bits, s_bits)


def revcomp(seq):
    return seq.translate(bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa"))[::-1]


def rseq(rng, n, pn=0.0, plow=0.1):
    out = []
    for _ in range(n):
        r = rng.random()
        if r < pn:
            out.append(rng.choice("NnRY-"))
        elif r < pn + plow:
            out.append(rng.choice("acgtu"))
        else:
            out.append(rng.choice("ACGTU"))
    return "".join(out).encode()


def mask_with(k, zeros):
    m = ["1"] * k
    for i in zeros:
        m[i] = "0"
    return "".join(m)


# the mask shapes the kernel distinguishes (tests/test_seeds_gpu.py: masks_for)
def masks_for(k):
    if k == 1:
        return ["1"]
    out = {"1" * k, mask_with(k, [k // 2]), "1" * (k - 1) + "0", "0" + "1" * (k - 1), ("01" * k)[:k - 1] + "1", "0" * (k - 1) + "1"}
    if k >= 4:
        out.add(mask_with(k, range(k // 4, k // 2)))
        out.add(mask_with(k, list(range(0, k // 4)) + [k - 1]))
        out.add(mask_with(k, list(range(1, 2)) + list(range(k // 2, k // 2 + 2)) + [k - 2]))
    return sorted(out)


def gap_mask(k, gap):
    return "1" * ((k - gap) // 2) + "0" * gap + "1" * ((k - gap) // 2)


def small_reads():
    with gzip.open(os.path.join(GOLD, "reads_small.fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    return [lines[i] for i in range(1, len(lines) - 1, 4)]


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
