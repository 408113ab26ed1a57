"""Host tests of gather (include/ntcard_hip.h: ntc_signature_gather_device): the symbol, every refusal that is decided before the device is touched — so it
is NTC_ERR_ARG on a machine without a GPU too, with the outputs left alone — and the numpy model the GPU tests trust (tests/sig_gather_model.py) on a case
worked by hand."""
import ctypes as C

import numpy as np

import sig_gather_model
from ntcard_amd import _abi
from support import ERR_ARG

SENTINEL = 0x5A5A5A5A


def call(nq=10, n_refs=2, ns=(5, 5), query=0x1000, refs=(0x2000, 0x3000), rows_cap=4, with_rows=True, with_n_rows=True, refs_null=False, n_null=False):
    """ntc_signature_gather_device on pointers that are never followed -> (rc, the outputs untouched?)"""
    L = _abi.lib()
    k = max(len(refs), 1)
    ptrs = (C.c_void_p * k)(*[C.c_void_p(p) if p else None for p in refs])
    n = (C.c_uint64 * k)(*ns)
    rows = np.full(8, SENTINEL, dtype=np.dtype([("w", np.uint64, 4)]))
    n_rows, rest, rest_w = C.c_uint32(SENTINEL), C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    rc = L.ntc_signature_gather_device(0, None, C.c_void_p(query) if query else None, None, nq, n_refs, None if refs_null else ptrs, None if n_null else n, 1,
                                       rows.ctypes.data_as(C.POINTER(_abi.NtcGatherRow)) if with_rows else None, rows_cap,
                                       C.byref(n_rows) if with_n_rows else None, C.byref(rest), C.byref(rest_w))
    untouched = bool(np.all(rows["w"] == SENTINEL)) and n_rows.value == SENTINEL and rest.value == SENTINEL and rest_w.value == SENTINEL
    return rc, untouched


def test_symbol_is_declared_and_exported():
    assert "ntc_signature_gather_device" in _abi.ABI_SYMBOLS and hasattr(_abi.lib(), "ntc_signature_gather_device")
    assert C.sizeof(_abi.NtcGatherRow) == 32 and sig_gather_model.ROW_DTYPE.itemsize == 32


def test_refusals_before_the_device_is_touched():
    L = _abi.lib()
    assert call(n_refs=0) == (ERR_ARG, True) and b"0 references" in L.ntc_last_error()
    assert call(n_refs=1025) == (ERR_ARG, True) and b"1025 references" in L.ntc_last_error()
    assert call(nq=2**32) == (ERR_ARG, True) and b"2^32" in L.ntc_last_error()
    assert call(ns=(5, 2**32)) == (ERR_ARG, True) and b"reference 1 " in L.ntc_last_error()
    assert call(with_n_rows=False) == (ERR_ARG, True)
    assert call(with_rows=False) == (ERR_ARG, True)  # NULL rows with rows_cap 4
    assert call(query=0) == (ERR_ARG, True) and b"query is null" in L.ntc_last_error()  # a NULL list with a length: the query,
    assert call(refs=(0x2000, 0)) == (ERR_ARG, True) and b"reference 1 is null" in L.ntc_last_error()  # a reference
    assert call(refs_null=True) == (ERR_ARG, True) and call(n_null=True) == (ERR_ARG, True)


def test_models_membership_is_np_isin():
    rng = np.random.default_rng(7)
    p = np.unique(rng.integers(1, 2**64 - 1, size=5000, dtype=np.uint64))
    q = p[np.sort(rng.permutation(p.size)[:3000])]
    for r in (p[rng.permutation(p.size)[:700]], p[-1:], q[-1:], q[:1], p[:0], q, np.array([0, 2**64 - 1], dtype=np.uint64)):  # (r in any order)
        assert np.array_equal(sig_gather_model.positions(q, r), np.flatnonzero(np.isin(q, r)))
    assert sig_gather_model.positions(q[:0], p[:10]).size == 0


def test_model_on_a_case_worked_by_hand():
    q = np.array([10, 20, 30, 40, 50, 60, 70, 80], dtype=np.uint64)
    counts = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint32)
    a = np.array([10, 20, 30, 40, 99], dtype=np.uint64)   # 4 common
    b = np.array([5, 30, 40, 50, 60], dtype=np.uint64)    # 4 common: ties with a, a has the lower index; after a: 50, 60
    c = np.array([30, 40], dtype=np.uint64)               # inside a: never reported
    d = np.array([60, 70], dtype=np.uint64)               # after a: 60, 70 — ties with b, b has the lower index; after b: 70
    rows, rest, rest_w = sig_gather_model.gather(q, counts, [a, b, c, d])
    assert rows.tolist() == [(0, 0, 4, 4, 1 + 2 + 3 + 4), (1, 0, 4, 2, 5 + 6), (3, 0, 2, 1, 7)]
    assert (rest, rest_w) == (1, 8)  # 80
    rows, rest, rest_w = sig_gather_model.gather(q, None, [a, b, c, d], threshold=2)
    assert rows.tolist() == [(0, 0, 4, 4, 4), (1, 0, 4, 2, 2)] and (rest, rest_w) == (2, 2)
    rows, rest, rest_w = sig_gather_model.gather(q, counts, [a, b, c, d], max_rows=1)
    assert rows.tolist() == [(0, 0, 4, 4, 10)] and (rest, rest_w) == (4, 5 + 6 + 7 + 8)
    rows, rest, rest_w = sig_gather_model.gather(q, counts, [b, a], threshold=0, max_rows=0)
    assert rows.size == 0 and (rest, rest_w) == (8, 36)
    rows, rest, rest_w = sig_gather_model.gather(q, counts, [b, a, a])  # swapped: b first; a listed twice is reported once
    assert rows.tolist() == [(0, 0, 4, 4, 3 + 4 + 5 + 6), (1, 0, 4, 2, 1 + 2)] and (rest, rest_w) == (2, 15)
