"""numpy models of the set algebra and the spectrum of signatures (include/ntcard_hip.h: ntc_signature_union_device, ntc_signature_select_device,
ntc_signature_hist_device), the reference of tests/test_sig_algebra_*.py.  tests/test_sig_algebra_host.py checks them against a dict-based brute force and on
cases worked by hand."""
import numpy as np

U32_MAX = 2**32 - 1


def union(lists, counts=None):
    """lists: uint64 arrays, each strictly ascending; counts: None, or per list a uint32 array or None (1 each)
    -> (the distinct hashes ascending uint64, min(the sum of their counts, 2^32 - 1) uint32)"""
    lists = [np.asarray(h, dtype=np.uint64) for h in lists]
    counts = [None] * len(lists) if counts is None else counts
    cs = [np.ones(h.size, np.uint64) if c is None else np.asarray(c).astype(np.uint64) for h, c in zip(lists, counts)]
    allh = np.concatenate(lists) if lists else np.zeros(0, np.uint64)
    allc = np.concatenate(cs) if cs else np.zeros(0, np.uint64)
    hashes, inverse = np.unique(allh, return_inverse=True)
    total = np.zeros(hashes.size, dtype=np.uint64)
    np.add.at(total, inverse, allc)
    return hashes, np.minimum(total, np.uint64(U32_MAX)).astype(np.uint32)


def select(a, ca, refs, mode="all", min_count=0, max_count=0):
    """a: uint64 ascending; ca: uint32 or None (1 each); refs: uint64 arrays; mode "all" / "none" / "any" -> (hashes, counts uint32) of the kept entries"""
    a = np.asarray(a, dtype=np.uint64)
    c = np.ones(a.size, np.uint32) if ca is None else np.asarray(ca, dtype=np.uint32)
    keep = c >= np.uint32(min_count)
    if max_count:
        keep &= c <= np.uint32(max_count)
    held = [np.isin(a, np.asarray(r, dtype=np.uint64)) for r in refs]
    if mode == "all":
        member = np.logical_and.reduce(held) if held else np.ones(a.size, bool)
    elif mode == "none":
        member = ~np.logical_or.reduce(held) if held else np.ones(a.size, bool)
    else:
        assert mode == "any"
        member = np.logical_or.reduce(held) if held else np.zeros(a.size, bool)
    keep &= member
    return a[keep], c[keep]


def hist(counts, cov_max=1000):
    """-> (hist uint64[cov_max + 2]: hist[v] = the entries with count v, hist[cov_max + 1] = those with a larger one; weight = the sum of the counts)"""
    c = np.asarray(counts).astype(np.uint64)
    h = np.bincount(np.minimum(c, np.uint64(cov_max + 1)).astype(np.int64), minlength=cov_max + 2).astype(np.uint64)
    return h, int(c.sum(dtype=np.uint64))
