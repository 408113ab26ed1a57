"""Host tests of the set algebra and the spectrum of signatures (include/ntcard_hip.h: ntc_signature_union_device, ntc_signature_select_device,
ntc_signature_hist_device): the symbols, every refusal that is decided before the device is touched — so it is NTC_ERR_ARG on a machine without a GPU too,
with the outputs left alone — and the numpy models the GPU tests trust (tests/sig_algebra_model.py) against a dict-based brute force and on cases worked by
hand."""
import ctypes as C

import numpy as np
import pytest

import sig_algebra_model as model
from ntcard_amd import _abi
from support import ERR_ARG

SENTINEL = 0x5A5A5A5A
U32_MAX = 2**32 - 1
A, B, CA = 0x100000, 0x200000, 0x300000  # "device" addresses that are never followed


def table(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(p) if p else None for p in ptrs])


class Outputs:
    """sentinel-filled arrays that stand in for the device outputs, and *n_out"""

    def __init__(self):
        self.h = np.full(64, SENTINEL, dtype=np.uint64)
        self.c = np.full(64, SENTINEL, dtype=np.uint32)
        self.n = C.c_uint64(SENTINEL)

    def untouched(self):
        return bool(np.all(self.h == SENTINEL)) and bool(np.all(self.c == SENTINEL)) and self.n.value == SENTINEL


def union(n_lists=2, ptrs=(A, B), cptrs=None, ns=(5, 5), out="own", out_c="own", cap=64, with_n_out=True, ptrs_null=False, n_null=False):
    """ntc_signature_union_device on pointers that are never followed -> (rc, the outputs untouched?)"""
    L = _abi.lib()
    o = Outputs()
    oh = o.h.ctypes.data if out == "own" else out
    oc = o.c.ctypes.data if out_c == "own" else out_c
    rc = L.ntc_signature_union_device(0, None, n_lists, None if ptrs_null else table(ptrs), table(cptrs) if cptrs is not None else None,
                                      None if n_null else (C.c_uint64 * max(len(ns), 1))(*ns), C.c_void_p(oh) if oh else None, C.c_void_p(oc) if oc else None, cap,
                                      C.byref(o.n) if with_n_out else None)
    return rc, o.untouched()


def select(a=A, ca=None, na=10, n_refs=1, refs=(B,), ns=(5,), mode=0, min_count=0, max_count=0, out="own", out_c="own", cap=64, with_n_out=True, refs_null=False,
           n_null=False):
    """ntc_signature_select_device likewise"""
    L = _abi.lib()
    o = Outputs()
    oh = o.h.ctypes.data if out == "own" else out
    oc = o.c.ctypes.data if out_c == "own" else out_c
    rc = L.ntc_signature_select_device(0, None, C.c_void_p(a) if a else None, C.c_void_p(ca) if ca else None, na, n_refs, None if refs_null else table(refs),
                                       None if n_null else (C.c_uint64 * max(len(ns), 1))(*ns), mode, min_count, max_count, C.c_void_p(oh) if oh else None,
                                       C.c_void_p(oc) if oc else None, cap, C.byref(o.n) if with_n_out else None)
    return rc, o.untouched()


def hist(counts=A, n=10, cov_max=1000, with_hist=True):
    L = _abi.lib()
    h = np.full(65540, SENTINEL, dtype=np.uint64)
    w = C.c_uint64(SENTINEL)
    rc = L.ntc_signature_hist_device(0, None, C.c_void_p(counts) if counts else None, n, cov_max, h.ctypes.data_as(C.c_void_p) if with_hist else None, C.byref(w))
    return rc, bool(np.all(h == SENTINEL)) and w.value == SENTINEL


def test_symbols_are_declared_and_exported():
    import ntcard_amd as nt
    for name in ("ntc_signature_union_device", "ntc_signature_select_device", "ntc_signature_hist_device"):
        assert name in _abi.ABI_SYMBOLS and hasattr(_abi.lib(), name)
    assert callable(nt.signature_union_device) and callable(nt.signature_select_device) and callable(nt.signature_hist_device)
    assert _abi.lib().ntc_abi_version() == 6


def test_union_refusals_before_the_device_is_touched():
    err = _abi.lib().ntc_last_error
    assert union(with_n_out=False) == (ERR_ARG, True) and b"n_out is null" in err()
    assert union(n_lists=0) == (ERR_ARG, True) and b"0 lists" in err()
    assert union(n_lists=1025) == (ERR_ARG, True) and b"1025 lists" in err()
    assert union(ptrs_null=True) == (ERR_ARG, True) and b"null argument" in err()
    assert union(n_null=True) == (ERR_ARG, True) and b"null argument" in err()
    assert union(ptrs=(A, 0)) == (ERR_ARG, True) and b"list 1 is null and has 5 entries" in err()
    assert union(ns=(5, 2**32)) == (ERR_ARG, True) and b"list 1 has 4294967296 entries" in err()
    assert union(ns=(2**31, 2**31)) == (ERR_ARG, True) and b"4294967296 entries in all" in err()
    # the size query is a NULL hash output with cap 0 and no count output; anything else with a NULL hash output is refused
    assert union(out=0, out_c=0, cap=1) == (ERR_ARG, True) and b"size alone" in err()
    assert union(out=0, cap=0) == (ERR_ARG, True) and b"size alone" in err()
    # an output array that overlaps an input array, by its last / first byte
    assert union(ns=(100, 5), out=A + 8 * 99, out_c=0, cap=10) == (ERR_ARG, True) and b"overlaps list 0" in err()
    assert union(ns=(5, 100), out=B - 8 * 10 + 1, out_c=0, cap=10) == (ERR_ARG, True) and b"overlaps list 1" in err()
    assert union(ns=(100, 5), out=0x900000, out_c=A + 4, cap=10) == (ERR_ARG, True) and b"overlaps list 0" in err()
    assert union(ns=(5, 100), cptrs=(0, CA), out=CA + 396, out_c=0, cap=10) == (ERR_ARG, True) and b"overlaps list 1" in err()
    assert union(ns=(5, 100), cptrs=(0, CA), out=0x900000, out_c=CA - 39, cap=10) == (ERR_ARG, True) and b"overlaps list 1" in err()


def test_select_refusals_before_the_device_is_touched():
    err = _abi.lib().ntc_last_error
    assert select(with_n_out=False) == (ERR_ARG, True) and b"n_out is null" in err()
    assert select(n_refs=1025) == (ERR_ARG, True) and b"1025 references" in err()
    assert select(refs_null=True) == (ERR_ARG, True) and b"null argument" in err()
    assert select(n_null=True) == (ERR_ARG, True) and b"null argument" in err()
    assert select(a=0) == (ERR_ARG, True) and b"A is null and has 10 entries" in err()
    assert select(na=2**32) == (ERR_ARG, True) and b"A has 4294967296 entries" in err()
    assert select(refs=(0,)) == (ERR_ARG, True) and b"reference 0 is null and has 5 entries" in err()
    assert select(n_refs=2, refs=(B, CA), ns=(5, 2**32)) == (ERR_ARG, True) and b"reference 1 has 4294967296 entries" in err()
    assert select(mode=3) == (ERR_ARG, True) and b"mode 3" in err()
    assert select(min_count=3, max_count=2) == (ERR_ARG, True) and b"min_count 3 is above max_count 2" in err()
    assert select(out=0, out_c=0, cap=1) == (ERR_ARG, True) and b"size alone" in err()
    assert select(out=0, cap=0) == (ERR_ARG, True) and b"size alone" in err()
    assert select(out=A + 8 * 9, out_c=0, cap=10) == (ERR_ARG, True) and b"overlaps A" in err()
    assert select(ca=CA, out=0x900000, out_c=CA + 36, cap=10) == (ERR_ARG, True) and b"overlaps A" in err()
    assert select(out=B - 79, out_c=0, cap=10) == (ERR_ARG, True) and b"overlaps reference 0" in err()
    assert select(n_refs=2, refs=(B, CA), ns=(5, 7), out=0x900000, out_c=CA + 8 * 6 + 7, cap=10) == (ERR_ARG, True) and b"overlaps reference 1" in err()


def test_hist_refusals_before_the_device_is_touched():
    err = _abi.lib().ntc_last_error
    assert hist(with_hist=False)[0] == ERR_ARG and b"hist_out is null" in err()
    assert hist(cov_max=0) == (ERR_ARG, True) and b"cov_max 0" in err()
    assert hist(cov_max=65536) == (ERR_ARG, True) and b"cov_max 65536" in err()
    assert hist(counts=0) == (ERR_ARG, True) and b"null and has 10 entries" in err()


def test_hist_of_nothing_needs_no_device():
    import ntcard_amd as nt
    h, w = nt.signature_hist_device(0, 0, cov_max=5)
    assert h.dtype == np.uint64 and h.tolist() == [0] * 7 and int(w) == 0
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_hist_device(0, 0, cov_max=65536)
    assert ei.value.code == ERR_ARG


# ---- the models ----
def brute_union(lists, counts):
    d = {}
    for i, h in enumerate(lists):
        for j, x in enumerate(h.tolist()):
            d[x] = d.get(x, 0) + (1 if counts is None or counts[i] is None else int(counts[i][j]))
    keys = sorted(d)
    return keys, [min(d[k], U32_MAX) for k in keys]


def brute_select(a, ca, refs, mode, lo, hi):
    sets = [set(r.tolist()) for r in refs]
    out = []
    for j, x in enumerate(a.tolist()):
        c = 1 if ca is None else int(ca[j])
        if c < lo or (hi and c > hi):
            continue
        held = [x in s for s in sets]
        if {"all": all(held), "none": not any(held), "any": any(held)}[mode]:
            out.append((x, c))
    return [x for x, _ in out], [c for _, c in out]


def brute_hist(counts, cov_max):
    h = [0] * (cov_max + 2)
    for c in counts.tolist():
        h[min(c, cov_max + 1)] += 1
    return h, sum(counts.tolist())


def test_models_against_brute_force():
    rng = np.random.default_rng(11)
    pool = np.unique(np.concatenate([rng.integers(0, 2**64, size=300, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)]))
    for trial in range(40):
        k = int(rng.integers(1, 6))
        lists = [np.sort(rng.choice(pool, size=int(rng.integers(0, 120)), replace=False)) for _ in range(k)]
        counts = [None if rng.random() < 0.4 else rng.choice(np.array([1, 2, 7, 2**31, U32_MAX], dtype=np.uint32), size=h.size) for h in lists]
        if trial % 5 == 0:
            counts = None
        h, c = model.union(lists, counts)
        assert h.dtype == np.uint64 and c.dtype == np.uint32
        assert (h.tolist(), c.tolist()) == tuple(brute_union(lists, counts))
        a, ca = lists[0], (None if counts is None else counts[0])
        lo, hi = int(rng.integers(0, 3)), int(rng.choice([0, 2, 7, U32_MAX]))
        for mode in ("all", "none", "any"):
            for refs in (lists[1:], []):
                sh, sc = model.select(a, ca, refs, mode, lo, hi)
                assert sh.dtype == np.uint64 and sc.dtype == np.uint32
                assert (sh.tolist(), sc.tolist()) == tuple(brute_select(a, ca, refs, mode, lo, hi))
        cs = rng.choice(np.array([0, 1, 1, 1, 2, 3, 9, 10, 11, 5000, U32_MAX], dtype=np.uint32), size=int(rng.integers(0, 200)))
        for cov in (1, 10, 1000):
            hh, w = model.hist(cs, cov)
            assert hh.dtype == np.uint64 and (hh.tolist(), w) == tuple(brute_hist(cs, cov))


def test_models_on_cases_worked_by_hand():
    u64, u32 = (lambda *v: np.array(v, dtype=np.uint64)), (lambda *v: np.array(v, dtype=np.uint32))
    # union: 20 is in all three lists, 0 and 2^64 - 1 are values like any other; the middle list has no counts
    h, c = model.union([u64(0, 10, 20), u64(20, 30), u64(5, 20, 2**64 - 1)], [u32(1, 2, 3), None, u32(U32_MAX, 4, 9)])
    assert h.tolist() == [0, 5, 10, 20, 30, 2**64 - 1] and c.tolist() == [1, U32_MAX, 2, 3 + 1 + 4, 1, 9]
    h, c = model.union([u64(7), u64(7), u64(7)], [u32(2**31), u32(2**31), u32(2**31)])
    assert h.tolist() == [7] and c.tolist() == [U32_MAX]  # 3 x 2^31 saturates
    h, c = model.union([u64(7), u64(7)], [u32(U32_MAX - 1), None])
    assert c.tolist() == [U32_MAX]  # lands exactly on 2^32 - 1
    h, c = model.union([u64(), u64()])
    assert h.size == 0 and c.size == 0
    # select
    a, ca = u64(10, 20, 30, 40, 50), u32(1, 2, 3, 4, 5)
    r1, r2 = u64(20, 30, 40, 99), u64(5, 30, 40, 50)
    assert [x.tolist() for x in model.select(a, ca, [r1, r2], "all")] == [[30, 40], [3, 4]]
    assert [x.tolist() for x in model.select(a, ca, [r1, r2], "none")] == [[10], [1]]
    assert [x.tolist() for x in model.select(a, ca, [r1, r2], "any")] == [[20, 30, 40, 50], [2, 3, 4, 5]]
    assert [x.tolist() for x in model.select(a, ca, [r1, r2], "any", 3, 4)] == [[30, 40], [3, 4]]  # both bounds are inclusive
    assert [x.tolist() for x in model.select(a, ca, [], "all", 2, 0)] == [[20, 30, 40, 50], [2, 3, 4, 5]]  # max_count 0: no upper bound
    assert model.select(a, ca, [], "any")[0].size == 0 and model.select(a, ca, [r1, u64()], "all")[0].size == 0  # no reference; an empty reference
    assert model.select(a, ca, [u64()], "none")[0].tolist() == a.tolist()
    assert [x.tolist() for x in model.select(a, None, [r1], "all", 1, 1)] == [[20, 30, 40], [1, 1, 1]] and model.select(a, None, [], "all", 2)[0].size == 0
    # hist
    hh, w = model.hist(u32(0, 1, 1, 3, 4, 5, U32_MAX), 3)
    assert hh.tolist() == [1, 2, 0, 1, 3] and w == 14 + U32_MAX
    hh, w = model.hist(u32(), 1)
    assert hh.tolist() == [0, 0, 0] and w == 0
