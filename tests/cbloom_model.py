"""The counting Bloom filter of include/ntcard_hip.h (ntc_cbloom_*) as numpy, host only, on tests/bloom_model.py's windows and positions.

Counters: every position of every window gets one increment — np.add.at on a wide integer array, so a position that two hashes of one k-mer share counts
twice — then min(., 255) as uint8.  A merge is a saturating add.  The count of a k-mer is the minimum of its counters.  tests/test_cbloom_host.py pins
the model thresholded at 1 to bloom_model.build's image."""
import numpy as np

import bloom_model as bm


def all_values(seqs, k, strand):
    vals = bm.h0_values(list(seqs), k, strand)
    return np.concatenate(vals) if vals else np.zeros(0, dtype=np.uint64)


def counters_of(h0, n_hash, k, m, into=None):
    """uint8 [m]: min(255, into + the increments of the given h_0 values)"""
    wide = np.zeros(m, dtype=np.int64) if into is None else into.astype(np.int64)
    np.add.at(wide, bm.positions(h0, n_hash, k, m).ravel().astype(np.int64), 1)
    return np.minimum(wide, 255).astype(np.uint8)


def counters(seqs, k, strand, n_hash, m, into=None):
    """-> (counters uint8 [m], windows inserted)"""
    v = all_values(seqs, k, strand)
    return counters_of(v, n_hash, k, m, into), int(v.size)


def merge(a, b):
    return np.minimum(a.astype(np.int64) + b.astype(np.int64), 255).astype(np.uint8)


def counts(cnt, h0, n_hash, k):
    """uint8 [n]: the minimum over each value's positions"""
    h0 = np.asarray(h0, dtype=np.uint64)
    if h0.size == 0:
        return np.zeros(0, dtype=np.uint8)
    return cnt[bm.positions(h0, n_hash, k, cnt.size).astype(np.int64)].min(axis=1)


def query(cnt, seqs, k, strand, n_hash, min_count=1):
    """-> (windows uint32 [n], hits uint32 [n]): a window hits iff its count is >= min_count — false answers included"""
    vals = bm.h0_values(list(seqs), k, strand)
    w = np.array([v.size for v in vals], dtype=np.uint32)
    h = np.array([int((counts(cnt, v, n_hash, k) >= min_count).sum()) for v in vals], dtype=np.uint32)
    return w, h


def window_starts(seq, k):
    """bool [len(seq)]: whether a window of k bases (A C G T U, either case) starts at each position"""
    ok = np.isin(np.frombuffer(seq, dtype=np.uint8), np.frombuffer(b"ACGTUacgtu", dtype=np.uint8))
    out = np.zeros(len(seq), dtype=bool)
    if len(seq) >= k:
        bad = np.concatenate([[0], np.cumsum(~ok)])
        out[: len(seq) - k + 1] = (bad[k:] - bad[: len(seq) - k + 1]) == 0
    return out


def profile(cnt, seqs, k, strand, n_hash):
    """uint8 [sum of the lengths]: byte p = the count of the window that starts at p, 0 where none starts"""
    vals = bm.h0_values(list(seqs), k, strand)
    parts = []
    for s, v in zip(seqs, vals):
        row = np.zeros(len(s), dtype=np.uint8)
        at = window_starts(s, k)
        assert int(at.sum()) == v.size
        row[at] = counts(cnt, v, n_hash, k)
        parts.append(row)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def threshold(cnt, min_count):
    """the plain filter's byte image of m_bits = len(cnt): the bit of loc is set iff cnt[loc] >= min_count"""
    return bm.image_of(np.nonzero(cnt >= min_count)[0], cnt.size)


def solid_values(cnt, seqs, k, strand, n_hash, min_count):
    """the h_0 of every window whose count is >= min_count, in window order (with repeats)"""
    v = all_values(seqs, k, strand)
    return v[counts(cnt, v, n_hash, k) >= min_count]


def hist(cnt):
    return np.bincount(cnt, minlength=256).astype(np.uint64)
