"""CPU tests of the long-sequence entry points (include/ntcard_hip.h: ntc_long_plan, ntc_submit_long_device, ntc_long_stats): the plan is a pure host
function and is pinned here window by window; bad arguments are refused before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

import ntcard_amd as nt
from ntcard_amd import _abi

NEW_SYMBOLS = ["ntc_submit_long_device", "ntc_long_plan", "ntc_long_stats", "ntc_long_time"]


def test_library_exports_the_long_sequence_symbols():
    L = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in _abi.ABI_SYMBOLS and hasattr(L, name), name
    assert L.ntc_abi_version() == 6  # additive: the ABI version stays
    assert callable(nt.long_plan) and hasattr(nt.Engine, "submit_long_device") and hasattr(nt.Engine, "long_stats")


def piece_lengths(k):
    return sorted({(k + 15 + 15) // 16 * 16, 48, 1008})


@pytest.mark.parametrize("k", [12, 31, 32])
def test_long_plan_partitions_the_windows(k):
    for L in piece_lengths(k):
        assert L >= k + 15 and L % 16 == 0
        S = L - k + 1
        for n in range(0, 3 * L + 2 * S + 2):
            m, rem = nt.long_plan(k, L, n)
            assert rem == m * S
            if n < L:
                assert m == 0
            else:
                assert m >= 1 and (m - 1) * S + L <= n, (k, L, n)  # every full piece lies inside the sequence
                assert k - 1 <= n - rem <= L - 1, (k, L, n)
            starts = np.zeros(max(n - k + 1, 0), dtype=np.int64)
            for j in range(m):  # windows of piece j start at j S .. j S + L - k
                starts[j * S: j * S + L - k + 1] += 1
            if n - rem >= k:  # windows of the remainder start at rem .. n - k
                starts[rem: n - k + 1] += 1
            assert np.all(starts == 1), (k, L, n)  # 0 .. n - k, each once


def test_long_plan_rejects_bad_piece_lengths():
    L = _abi.lib()
    m, rem = C.c_uint64(), C.c_uint64()
    ok = lambda k, pl: L.ntc_long_plan(k, pl, 1000, C.byref(m), C.byref(rem))
    assert ok(32, 48) == 0 and ok(32, 65520) == 0 and ok(12, 32) == 0
    assert ok(32, 50) == -1 and b"piece_len" in L.ntc_last_error()  # not a multiple of 16
    assert ok(32, 32) == -1  # below k + 15
    assert ok(33, 47) == -1 and ok(34, 48) == -1
    assert ok(32, 65536) == -1  # above 65520
    assert ok(0, 48) == -1 and ok(0xffffffff, 48) == -1
    assert L.ntc_long_plan(32, 48, 1000, None, C.byref(rem)) == -1
    assert L.ntc_long_plan(32, 48, 1000, C.byref(m), None) == -1
    with pytest.raises(nt.NtcError):
        nt.long_plan(32, 40, 10)


def test_bad_long_submits_are_rejected_before_touching_the_device():
    """every one of these is refused for its own reason — the message says which — although there is no engine (and possibly no device) to look at"""
    L = _abi.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    offs = (C.c_uint64 * 3)(0, 100, 300)
    down = (C.c_uint64 * 3)(0, 200, 100)
    call = lambda d, o, n, pl: L.ntc_submit_long_device(None, d, o, n, pl)
    assert call(fake, None, 2, 0) == -1 and b"null offsets" in L.ntc_last_error()
    assert call(fake, offs, 2, 40) == -1 and b"piece_len" in L.ntc_last_error()  # not a multiple of 16
    assert call(fake, offs, 2, 65536) == -1 and b"piece_len" in L.ntc_last_error()  # above 65520
    assert call(fake, down, 2, 48) == -1 and b"monotone" in L.ntc_last_error()
    assert call(None, offs, 2, 48) == -1 and b"null buffer" in L.ntc_last_error()
    assert call(fake, offs, 2, 48) == -1 and b"null engine" in L.ntc_last_error()
    p, s = C.c_uint64(), C.c_uint64()
    assert L.ntc_long_stats(None, C.byref(p), C.byref(s)) == -1
    assert L.ntc_long_time(None, None, None) == -1
