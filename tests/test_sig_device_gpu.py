"""GPU tests of the device side of signatures behind the container (include/ntcard_hip.h): ntc_signature_device and the device sort inside ntc_signature against
tests/sig_model.py, ntc_signature_compare_device and ntc_signature_matrix_device against np.intersect1d."""
import ctypes as C
import functools

import numpy as np
import pytest

import sig_model
from gpu_support import nt, submit_slots  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 14
ERR_ARG, ERR_STATE = -1, -4


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def signature_on_device(e, plane=0):
    h, c, n = e.signature_device(plane)
    assert h.dtype == torch.int64 and c.dtype == torch.int32 and h.numel() == n and c.numel() == n and h.is_cuda and c.is_cuda
    return h.cpu().numpy().view(np.uint64), c.cpu().numpy().view(np.uint32)


def same(got, want):
    return np.array_equal(got[0], want[0].astype(np.uint64)) and np.array_equal(got[1].astype(np.int64), np.asarray(want[1]).astype(np.int64))


# ---- the engine ----
def test_engine_signature_device(nt):
    want = sig_model.equal_model(32, "canonical", 7)
    assert want[0].size == 593
    rng = np.random.default_rng(21)
    extra = np.setdiff1d(np.unique(rng.integers(1, 2**64, size=70500, dtype=np.uint64)), want[0])[:70000]
    extra = extra[rng.permutation(extra.size)]
    extra_c = rng.integers(1, 1000, size=extra.size).astype(np.uint32)
    assert extra.size == 70000
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e, nt.Engine([32], r_bits=R, s_bits=7) as plain:
        submit_slots(e, sig_model.equal_reads())
        assert same(signature_on_device(e), want) and same(e.signature(), want)  # 593 pairs: the one-launch sort
        # a short cap is refused with nothing written, *n included
        h, c = dev64(np.full(593, 7)), dev32(np.full(593, 7))
        n = C.c_uint64(12345)
        L = nt._abi.lib()
        rc = L.ntc_signature_device(e._h, 0, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), 592, C.byref(n))
        assert rc == ERR_ARG and n.value == 12345 and bool((h == 7).all()) and bool((c == 7).all())
        assert L.ntc_signature_device(e._h, 1, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), 593, C.byref(n)) == ERR_ARG  # no such plane
        assert L.ntc_signature_device(e._h, 0, None, None, 593, C.byref(n)) == ERR_ARG
        assert L.ntc_signature_device(e._h, 0, C.c_void_p(h.data_ptr()), None, 593, C.byref(n)) == 0 and n.value == 593  # counts may be NULL
        assert np.array_equal(h.cpu().numpy().view(np.uint64), want[0]) and bool((c == 7).all())
        # 70 000 more keys: the table grows past 2^16 slots, the sort takes its passes
        e.signature_inject(extra, extra_c)
        order = np.argsort(np.concatenate([want[0], extra]), kind="stable")
        both = (np.concatenate([want[0], extra])[order], np.concatenate([want[1].astype(np.uint32), extra_c])[order])
        assert same(signature_on_device(e), both) and same(e.signature(), both)
        assert e.signature_stats()[0] > 2**16
        with pytest.raises(nt.NtcError) as ei:
            plain.signature_device()
        assert ei.value.code == ERR_STATE
        with pytest.raises(nt.NtcError) as ei:
            plain.signature_sort_time()
        assert ei.value.code == ERR_STATE


def test_engine_two_planes_and_sort_time(nt):
    with nt.Engine([21, 32], r_bits=R, s_bits=7, signature=True) as e:
        e.set_profiling(True)
        assert e.signature_sort_time() == 0.0
        submit_slots(e, sig_model.equal_reads())
        w21, w32 = sig_model.equal_model(21, "canonical", 7), sig_model.equal_model(32, "canonical", 7)
        assert not np.array_equal(w21[0], w32[0])
        assert same(signature_on_device(e, 0), w21) and same(signature_on_device(e, 1), w32)
        assert e.signature_sort_time() > 0.0
        e.reset()
        assert e.signature_sort_time() == 0.0
        assert signature_on_device(e, 1)[0].size == 0


# ---- compare ----
@functools.lru_cache(maxsize=None)
def pool():
    p = np.unique(np.random.default_rng(31).integers(1, 2**64 - 1, size=300000, dtype=np.uint64))
    p.setflags(write=False)
    return p


def compare_cases():
    p = pool()
    rng = np.random.default_rng(32)
    big = p[:100000]
    pick = lambda n, seed: np.sort(np.random.default_rng(seed).choice(p[:150000], size=n, replace=False))
    cases = {
        "identical": (p[:5000], p[:5000]),
        "disjoint": (p[:5000], p[5000:9000]),
        "evens_odds": (p[0:10000:2], p[1:10000:2]),
        "subset": (p[100:5000:7], p[:5000]),
        "a_empty": (p[:0], p[:1000]),
        "b_empty": (p[:1000], p[:0]),
        "both_empty": (p[:0], p[:0]),
        "one_first": (big[:1], big),
        "one_last": (big, big[-1:]),
        "one_below": (np.array([0], dtype=np.uint64), big),
        "one_above": (big, np.array([2**64 - 1], dtype=np.uint64)),
        "common_only_first": (np.concatenate([p[:1], p[1000:2000]]), np.concatenate([p[:1], p[3000:4500]])),
        "common_only_last": (np.concatenate([p[1000:2000], p[-1:]]), np.concatenate([p[3000:4500], p[-1:]])),
        "len_255_256": (pick(255, 1), pick(256, 2)),
        "len_256_257": (pick(256, 3), pick(257, 4)),
        "len_257_65537": (pick(257, 5), pick(65537, 6)),
        "len_65537_65537": (pick(65537, 7), pick(65537, 8)),
    }
    del rng
    return cases


CASES = compare_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_compare(nt, name):
    a, b = CASES[name]
    rng = np.random.default_rng(len(name))
    ca, cb = rng.integers(1, 2**32, size=a.size, dtype=np.uint64).astype(np.uint32), rng.integers(1, 2**32, size=b.size, dtype=np.uint64).astype(np.uint32)
    common, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)
    want_sum = int(np.minimum(ca[ia], cb[ib]).astype(np.uint64).sum(dtype=np.uint64)) if common.size else 0
    da, db, dca, dcb = dev64(a), dev64(b), dev32(ca), dev32(cb)
    pa, pb = (da.data_ptr() if a.size else 0), (db.data_ptr() if b.size else 0)
    got = nt.signature_compare_device(pa, dca.data_ptr() if a.size else 0, a.size, pb, dcb.data_ptr() if b.size else 0, b.size)
    if a.size and b.size:
        assert got == (common.size, want_sum)
    else:
        assert got[0] == 0 and got[1] in (0, None)
    assert nt.signature_compare_device(pa, 0, a.size, pb, 0, b.size) == (common.size, None)
    assert nt.signature_compare(a, b)[0] == common.size  # the host function on the same arrays


def test_compare_min_sum_needs_64_bits_and_is_left_alone_without_counts(nt):
    p = pool()
    a, b = p[:3000], p[1000:4000]
    ca, cb = np.full(a.size, 2**32 - 1, dtype=np.uint32), np.full(b.size, 2**32 - 2, dtype=np.uint32)
    da, db, dca, dcb = dev64(a), dev64(b), dev32(ca), dev32(cb)
    assert nt.signature_compare_device(da.data_ptr(), dca.data_ptr(), a.size, db.data_ptr(), dcb.data_ptr(), b.size) == (2000, 2000 * (2**32 - 2))
    L = nt._abi.lib()
    c, m = C.c_uint64(), C.c_uint64(777)
    v = C.c_void_p
    assert L.ntc_signature_compare_device(0, None, v(da.data_ptr()), v(dca.data_ptr()), a.size, v(db.data_ptr()), None, b.size, C.byref(c), C.byref(m)) == 0
    assert c.value == 2000 and m.value == 777
    assert L.ntc_signature_compare_device(0, None, v(da.data_ptr()), None, a.size, v(db.data_ptr()), v(dcb.data_ptr()), b.size, C.byref(c), C.byref(m)) == 0
    assert c.value == 2000 and m.value == 777
    # null arguments come before the device
    assert L.ntc_signature_compare_device(0, None, None, None, 5, v(db.data_ptr()), None, b.size, C.byref(c), None) == ERR_ARG
    assert L.ntc_signature_compare_device(0, None, v(da.data_ptr()), None, a.size, None, None, 5, C.byref(c), None) == ERR_ARG
    assert L.ntc_signature_compare_device(0, None, v(da.data_ptr()), None, a.size, v(db.data_ptr()), None, b.size, None, None) == ERR_ARG


def test_compare_refuses_lists_that_do_not_ascend(nt):
    p = pool()
    good = p[:70000]
    step = p[:70000].copy()
    step[-1] = step[-3]  # one descending step, at the last entry
    dup = p[:70000].copy()
    dup[40000] = dup[39999]  # one duplicate
    L = nt._abi.lib()
    dg, ds, dd = dev64(good), dev64(step), dev64(dup)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_compare_device(dg.data_ptr(), 0, good.size, ds.data_ptr(), 0, step.size)
    assert ei.value.code == ERR_ARG and "second list" in str(ei.value) and "entry 69999" in str(ei.value)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_compare_device(dd.data_ptr(), 0, dup.size, dg.data_ptr(), 0, good.size)
    assert ei.value.code == ERR_ARG and "first list" in str(ei.value) and "entry 40000" in str(ei.value)
    # both lists are bad: the first list and its entry are named
    two, five = p[:6].copy(), p[:8].copy()
    two[2], five[5] = two[1], five[3]
    dt, df = dev64(two), dev64(five)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_compare_device(dt.data_ptr(), 0, two.size, df.data_ptr(), 0, five.size)
    assert ei.value.code == ERR_ARG and "first list" in str(ei.value) and "entry 2" in str(ei.value) and "second list" not in str(ei.value)
    c = C.c_uint64()
    assert L.ntc_signature_compare(step.ctypes.data_as(C.c_void_p), step.size, good.ctypes.data_as(C.c_void_p), good.size, C.byref(c)) == ERR_ARG
    assert b"first list" in L.ntc_last_error() and b"entry 69999" in L.ntc_last_error()  # the host function's words


# ---- matrix ----
def check_matrix(nt, lists):
    dl = [dev64(x) for x in lists]
    got = nt.signature_matrix_device([d.data_ptr() if x.size else 0 for d, x in zip(dl, lists)], [x.size for x in lists])
    assert got.dtype == np.uint64 and got.shape == (len(lists), len(lists))
    assert np.array_equal(got, got.T) and got.diagonal().tolist() == [x.size for x in lists]
    for i in range(len(lists)):
        for j in range(i + 1, len(lists)):
            assert int(got[i, j]) == np.intersect1d(lists[i], lists[j], assume_unique=True).size, (i, j)
    return got


def test_matrix_of_one(nt):
    assert check_matrix(nt, [pool()[:777]]).tolist() == [[777]]
    assert check_matrix(nt, [pool()[:0]]).tolist() == [[0]]


def test_matrix_of_six(nt):
    p = pool()[:120000]
    rng = np.random.default_rng(41)
    draw = lambda n: np.sort(rng.choice(p, size=n, replace=False))
    five = draw(5000)
    lists = [p[:0], draw(1), draw(300), five, five.copy(), draw(70001)]
    got = check_matrix(nt, lists)
    assert not got[0].any() and not got[:, 0].any() and int(got[3, 4]) == 5000 and int(got[3, 5]) > 2000


def test_matrix_of_forty(nt):
    p = pool()[:2000]
    rng = np.random.default_rng(42)
    lists = [np.sort(rng.choice(p, size=int(n), replace=False)) for n in rng.integers(100, 301, size=40)]
    got = check_matrix(nt, lists)
    assert int(np.count_nonzero(got)) > 40 * 39 // 2  # 780 pairs, a work item each


def test_matrix_refuses_an_unsorted_list_and_bad_counts(nt):
    p = pool()
    lists = [p[:3000], p[1000:9000].copy(), p[2000:2500]]
    lists[1][5000], lists[1][5001] = lists[1][5001], lists[1][5000]
    dl = [dev64(x) for x in lists]
    L = nt._abi.lib()
    ptrs = (C.c_void_p * 3)(*[d.data_ptr() for d in dl])
    ns = (C.c_uint64 * 3)(*[x.size for x in lists])
    out = np.full((3, 3), 0x5a5a5a5a, dtype=np.uint64)
    assert L.ntc_signature_matrix_device(0, None, 3, ptrs, ns, out.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert b"list 1 " in L.ntc_last_error() and b"entry 5001" in L.ntc_last_error() and bool(np.all(out == 0x5a5a5a5a))
    # lists 0 and 2 are bad: list 0 is named
    small = [p[:6].copy(), p[2:9], p[:8].copy()]
    small[0][3], small[2][5] = small[0][2], small[2][1]
    ds = [dev64(x) for x in small]
    sp = (C.c_void_p * 3)(*[d.data_ptr() for d in ds])
    sn = (C.c_uint64 * 3)(*[x.size for x in small])
    assert L.ntc_signature_matrix_device(0, None, 3, sp, sn, out.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert b"list 0 is not strictly ascending at entry 3" in L.ntc_last_error() and bool(np.all(out == 0x5a5a5a5a))
    for bad in (0, 1025):
        assert L.ntc_signature_matrix_device(0, None, bad, ptrs, ns, out.ctypes.data_as(C.c_void_p)) == ERR_ARG and bool(np.all(out == 0x5a5a5a5a))
    assert L.ntc_signature_matrix_device(0, None, 3, None, ns, out.ctypes.data_as(C.c_void_p)) == ERR_ARG
