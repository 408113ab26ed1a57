"""The Bloom filter of include/ntcard_hip.h (ntc_bloom_*) as numpy, host only.

Windows and h_0: canonical from orc.hash_read (the oracle's ntHashIterator); one strand from strand_model's array form (fh, rh of every window and whether
it is one) through strand_model.pick.  h_i = orc_multihash(h_0, i, k) (nthash.hpp:381-390), evaluated in wrapping uint64 arithmetic for whole arrays;
positions h_i % m in exact integer arithmetic; the byte image by the reference's bit rule, bit 7 - loc % 8 of byte loc / 8
(vendor/ntHash/lib/BloomFilter.hpp:56-66).  tests/test_bloom_host.py pins the array forms to orc_multihash, to Python integers, to
strand_model.window_values and to the reference tool's recorded rows."""
import functools

import numpy as np

import orc
import strand_model as sm

MULTI_SEED = 0x90B45D39FB6DA1FA  # nthash.hpp:381-390


@functools.lru_cache(maxsize=1 << 14)
def _strand_windows(seq, k):
    """(fs, rs) of every window of ONE sequence, in window order, read-only: strand_model's array form over the sequence alone.  Kept: the models of a
    test ask for the windows of the same sequences once per call, and at k = 600 one pass costs k table look-ups per position"""
    fs, rs, ok = sm.array_window_values(sm.pad_reads([seq], max(len(seq), 1)), "1" * k)
    out = (fs[0][ok[0]], rs[0][ok[0]]) if fs.shape[1] else (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))
    for a in out:
        a.flags.writeable = False
    return out


def h0_values(seqs, k, strand=0):
    """[uint64 array per sequence]: the value of every window of k bases, in window order"""
    if strand == sm.CANONICAL:
        return [orc.hash_read(s, k)[0] for s in seqs]
    return [sm.pick(*_strand_windows(bytes(s), k), strand) for s in seqs]


def multihash(h0, n_hash, k):
    """uint64 [n] -> uint64 [n, n_hash]: column 0 is h_0, column i is orc_multihash(h_0, i, k)"""
    h0 = np.asarray(h0, dtype=np.uint64)
    out = np.zeros((h0.size, n_hash), dtype=np.uint64)
    out[:, 0] = h0
    km = (k * MULTI_SEED) & (2**64 - 1)
    with np.errstate(over="ignore"):
        for i in range(1, n_hash):
            t = h0 * np.uint64(i ^ km)
            out[:, i] = t ^ (t >> np.uint64(27))
    return out


def positions(h0, n_hash, k, m):
    """uint64 [n, n_hash]: loc_i = h_i % m"""
    return multihash(h0, n_hash, k) % np.uint64(m)


def n_bytes(m):
    return (m + 7) // 8


def image_of(pos, m, into=None):
    """the byte image with the bits of `pos` set (ORed into `into` when given)"""
    img = np.zeros(n_bytes(m), dtype=np.uint8) if into is None else into
    p = np.asarray(pos, dtype=np.uint64).ravel()
    np.bitwise_or.at(img, (p >> np.uint64(3)).astype(np.int64), (0x80 >> (p & np.uint64(7)).astype(np.int64)).astype(np.uint8))
    return img


def bits_set(img, pos):
    """bool, the shape of pos: whether each position's bit is set"""
    p = np.asarray(pos, dtype=np.uint64)
    return (img[(p >> np.uint64(3)).astype(np.int64)] & (0x80 >> (p & np.uint64(7)).astype(np.int64)).astype(np.uint8)) != 0


def build(seqs, k, strand, n_hash, m, into=None):
    """-> (image, windows inserted)"""
    vals = h0_values(seqs, k, strand)
    allv = np.concatenate(vals) if vals else np.zeros(0, dtype=np.uint64)
    return image_of(positions(allv, n_hash, k, m), m, into), int(allv.size)


def query(img, seqs, k, strand, n_hash, m):
    """-> (windows uint32 [n], hits uint32 [n]): a window hits iff all its n_hash bits are set in img — false positives included"""
    vals = h0_values(seqs, k, strand)
    w = np.array([v.size for v in vals], dtype=np.uint32)
    h = np.array([int(bits_set(img, positions(v, n_hash, k, m)).all(axis=1).sum()) if v.size else 0 for v in vals], dtype=np.uint32)
    return w, h


def popcount(img):
    return int(np.unpackbits(img).sum())
