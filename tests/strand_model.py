"""Model of one-strand counting (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE) built from the oracle's primitives:
per read, every window of k bases -> fh, rh (orc_window_hash; under a mask the don't-care terms XORed out with orc_srol(orc_seed(b), k-1-i) /
orc_srol(orc_seed_comp(b), i), nthash.hpp:641-646), the strand's pick, ntComp (ntcard.cpp:132-145) -> t_Counter, F1.
One ctypes call per window: keep the inputs small."""
import ctypes as C
import random

import numpy as np

import orc
from support import GOLD, gap_mask, mask_with, masks_for, rseq, sketch_from_values, small_reads  # noqa: F401  (re-exported: sm.GOLD, sm.masks_for, ...)

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
