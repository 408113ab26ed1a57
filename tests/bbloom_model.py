"""The blocked Bloom filter of include/ntcard_hip.h (ntc_bbloom_*) as numpy, host only, on tests/bloom_model.py's windows and multi-hash.

Block b = h_0 mod n_blocks in exact integer arithmetic; in-block position p_i = (g >> (55 - 9 (i mod 4))) & 511 with g = bloom_model.multihash's column
1 + i // 4 (tests/test_bloom_host.py pins that column to the oracle's orc_multihash); bit loc_i = 512 b + p_i by bloom_model's bit rule.  The false
positive rate formula is summed with math.fsum over every term that is not zero in double precision.  tests/test_bbloom_host.py pins the positions to a
scalar restatement in Python integers."""
import math

import numpy as np

import bloom_model as bm

BLOCK = 512


def positions(h0, n_hash, k, m):
    """uint64 [n, n_hash]: loc_i = 512 (h_0 mod n_blocks) + p_i"""
    assert m % BLOCK == 0 and m >= BLOCK
    h0 = np.asarray(h0, dtype=np.uint64)
    mh = bm.multihash(h0, 2 + (n_hash - 1) // 4, k)  # columns 1 .. ceil(n_hash / 4) are used
    base = (h0 % np.uint64(m // BLOCK)) * np.uint64(BLOCK)
    out = np.zeros((h0.size, n_hash), dtype=np.uint64)
    for i in range(n_hash):
        out[:, i] = base + ((mh[:, 1 + i // 4] >> np.uint64(55 - 9 * (i % 4))) & np.uint64(BLOCK - 1))
    return out


def positions_scalar(h0, n_hash, k, m):
    """the same for ONE value in Python integers, from the definition"""
    mask = 2**64 - 1
    out = []
    for i in range(n_hash):
        t = (h0 * ((1 + i // 4) ^ ((k * bm.MULTI_SEED) & mask))) & mask
        g = t ^ (t >> 27)
        out.append(BLOCK * (h0 % (m // BLOCK)) + ((g >> (55 - 9 * (i % 4))) & 511))
    return out


def image_of(h0, n_hash, k, m, into=None):
    return bm.image_of(positions(h0, n_hash, k, m), m, into)


def test_values(img, h0, n_hash, k, m):
    """bool [n]: whether all n_hash bits of each value are set"""
    h0 = np.asarray(h0, dtype=np.uint64)
    if h0.size == 0:
        return np.zeros(0, dtype=bool)
    return bm.bits_set(img, positions(h0, n_hash, k, m)).all(axis=1)


test_values.__test__ = False  # (a helper, not a test)


def build(seqs, k, strand, n_hash, m, into=None):
    """-> (image, windows inserted)"""
    vals = bm.h0_values(list(seqs), k, strand)
    allv = np.concatenate(vals) if vals else np.zeros(0, dtype=np.uint64)
    return image_of(allv, n_hash, k, m, into), int(allv.size)


def query(img, seqs, k, strand, n_hash, m):
    """-> (windows uint32 [n], hits uint32 [n]) — false positives included"""
    vals = bm.h0_values(list(seqs), k, strand)
    w = np.array([v.size for v in vals], dtype=np.uint32)
    h = np.array([int(test_values(img, v, n_hash, k, m).sum()) for v in vals], dtype=np.uint32)
    return w, h


def block_popcounts(img):
    """int64 [n_blocks]: the set bits of every block"""
    return np.unpackbits(img).reshape(-1, BLOCK).sum(axis=1).astype(np.int64)


def block_hist(img):
    return np.bincount(block_popcounts(img), minlength=BLOCK + 1).astype(np.uint64)


def realised_fpr(img, n_hash):
    """the chance that a value never inserted finds its bits set: the mean over the blocks of (set bits / 512)^n_hash"""
    return float(((block_popcounts(img) / BLOCK) ** n_hash).mean())


def fpr(n, m, n_hash):
    """sum_j Poisson(j; l) (1 - (1 - 1/512)^(j n_hash))^n_hash, l = 512 n / m: every j from 0 to l + 40 sqrt(l) + 200, whose Poisson weights beyond are
    below 1e-300"""
    lam = BLOCK * n / m
    if lam == 0:
        return 0.0
    j = np.arange(0, int(lam + 40 * math.sqrt(lam) + 200), dtype=np.float64)
    lg = np.array([math.lgamma(x + 1.0) for x in j]) if j.size < 100000 else np.vectorize(math.lgamma)(j + 1.0)
    w = np.exp(j * math.log(lam) - lam - lg)
    f = (-np.expm1(j * n_hash * math.log1p(-1.0 / BLOCK))) ** n_hash
    return math.fsum((w * f).tolist())
