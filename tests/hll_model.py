"""Model of an nthll engine with planes, spaced seeds and a strand (include/ntcard_hip.h: ntc_hll_create_ex): per plane the values of
tests/strand_model.py (window_values -> pick) pushed through nthll's ntComp (nthll.cpp:92-97) in numpy.  tests/test_nthll_ext_host.py pins it to the
oracle.  One ctypes call per window (strand_model.window_values): keep the inputs small."""
import functools

import numpy as np

import strand_model as sm


def clz64(x):
    """leading zeros of every (non-zero) uint64 of x"""
    x = x.astype(np.uint64).copy()
    n = np.zeros(x.shape, dtype=np.uint8)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (x >> np.uint64(64 - s)) == np.uint64(0)
        n[top_clear] += s
        x[top_clear] <<= np.uint64(s)
    return n


def registers(h, n_bits):
    """nthll.cpp:92-97 over the values h (uint64): rest = h & ~(2^b - 1); where rest != 0, M[h & (2^b - 1)] = max(.., clz64(rest))"""
    low = np.uint64((1 << n_bits) - 1)
    M = np.zeros(1 << n_bits, dtype=np.uint8)
    rest = h & ~low
    keep = rest != np.uint64(0)
    np.maximum.at(M, (h[keep] & low).astype(np.int64), clz64(rest[keep]))
    return M


def planes_of(values, strand, n_bits):
    """values: [(fs, rs)] per plane (strand_model.values_of) -> (regs uint8 [n_planes, 1 << n_bits], f1 uint64 [n_planes]); F1 = the number of values"""
    regs = np.zeros((len(values), 1 << n_bits), dtype=np.uint8)
    f1 = np.zeros(len(values), dtype=np.uint64)
    for i, (fs, rs) in enumerate(values):
        h = sm.pick(fs, rs, strand)
        regs[i] = registers(h, n_bits)
        f1[i] = h.size
    return regs, f1


def model(reads, masks, strand, n_bits):
    return planes_of(sm.values_of(reads, masks), strand, n_bits)


# ---- the read sets and configurations of tests/test_nthll_ext_gpu.py (tests/test_nthll_ext_host.py shows that they tell the cases apart) ----
# (name, masks, from_seeds?, n_bits)
CONFIGS = [
    ("k32", ["1" * 32], False, 10),
    ("k64", ["1" * 64], False, 10),
    ("klist", ["1" * 16, "1" * 24, "1" * 32, "1" * 48], False, 9),
    ("gap12_2", [sm.gap_mask(12, 2)], True, 10),
    ("gap32_8", [sm.gap_mask(32, 8)], True, 10),
    ("seeds", sm.SEED_MASKS, True, 9),
]


@functools.lru_cache(maxsize=None)
def config_values(name, which):
    """the planes' values of a CONFIGS row over sketch_reads_equal ("equal") / sketch_reads_ragged ("ragged"): computed once, never changed"""
    masks = next(c[1] for c in CONFIGS if c[0] == name)
    return sm.values_of(sm.sketch_reads_equal() if which == "equal" else sm.sketch_reads_ragged(), masks)


@functools.lru_cache(maxsize=None)
def small_values(masks):
    """the same over tests/golden/reads_small.fq.gz; masks: a tuple"""
    return sm.values_of(sm.small_reads(), list(masks))
