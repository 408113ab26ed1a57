"""CPU tests of the cut a k list shares (include/ntcard_hip.h: ntc_submit_long_device, ntc_long_plan): the pieces are cut once, with the overlap of the
largest k, and every k of the list counts the windows that START in a piece's first S bytes.  The partition the engine relies on is pinned here window
by window, in pure Python, from ntc_long_plan(kmax, ..)."""
import ctypes as C

import numpy as np
import pytest

import ntcard_amd as nt
from ntcard_amd import _abi

PL = 48
LISTS = [(17, 32), (20, 26, 32), (12, 27)]


def boundary_lengths(kl, L):
    kmin, kmax = min(kl), max(kl)
    S = L - kmax + 1
    lens = {0, kmin - 1, kmin, kmax - 1, kmax, L - 1, L, L + S - 1, L + S}
    for m in (1, 2, 5):  # m full pieces and a remainder of kmax - 1 (the least there is), kmax, ..., L - 1 (the most) bytes
        lens |= {m * S + r for r in (kmax - 1, kmax, kmax + 1, L - 2, L - 1)}
    if L == PL:  # and every length up to three pieces and two steps
        lens |= set(range(0, 3 * L + 2 * S + 2))
    return sorted(lens)


@pytest.mark.parametrize("kl", LISTS, ids=str)
@pytest.mark.parametrize("L", [PL, 1008])
def test_one_cut_partitions_the_windows_of_every_k(kl, L):
    kmin, kmax = min(kl), max(kl)
    assert kmax - kmin <= 15 and L >= kmax + 15 and L % 16 == 0
    S = L - kmax + 1
    for n in boundary_lengths(kl, L):
        m, rem = nt.long_plan(kmax, L, n)
        assert rem == m * S and (m == 0) == (n < L)
        if m:
            assert (m - 1) * S + L <= n and kmax - 1 <= n - rem <= L - 1, (kl, L, n)  # the remainder is never shorter than kmax - 1 bytes
        for k in kl:
            # piece j as a read of L_k = L - (kmax - k) bases: its windows start at j S .. j S + L_k - k = j S + S - 1
            L_k = L - (kmax - k)
            assert L_k - k + 1 == S and 16 * (L // 16 - 1) < L_k <= L  # (spread <= 15: the trimmed read ends in the piece's last chunk)
            starts = np.zeros(max(n - k + 1, 0), dtype=np.int64)
            for j in range(m):
                starts[j * S: j * S + S] += 1
            if n - rem >= kmin and n - rem >= k:  # the remainder [m S, n) goes to row slots iff it holds a window of kmin; its windows of k start at m S .. n - k
                starts[rem: n - k + 1] += 1
            assert np.all(starts == 1), (kl, L, n, k)  # 0 .. n - k, each once


@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_a_remainder_of_kmax_minus_1_bytes_holds_windows_of_the_smaller_k_only(kl):
    kmin, kmax = min(kl), max(kl)
    S = PL - kmax + 1
    n = 5 * S + kmax - 1
    m, rem = nt.long_plan(kmax, PL, n)
    assert m == 5 and n - rem == kmax - 1
    assert n - rem >= kmin  # counted under the list (the test of one k, n - rem >= kmax, would drop it)
    assert sorted(k for k in kl if n - rem >= k) == sorted(k for k in kl if k < kmax)


@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_bad_piece_length_for_a_list_is_rejected_on_the_host(kl):
    """the piece_len rule of a list is that of its largest k: a multiple of 16 with kmax + 15 <= piece_len <= 65520 — checked by ntc_long_plan(kmax, ..)
    with no device, as for one k"""
    kmax = max(kl)
    L = _abi.lib()
    m, rem = C.c_uint64(), C.c_uint64()
    bad = (kmax + 14) // 16 * 16  # the largest multiple of 16 below kmax + 15
    assert bad < kmax + 15 and bad >= min(kl)
    assert L.ntc_long_plan(kmax, bad, 1000, C.byref(m), C.byref(rem)) == -1 and b"piece_len" in L.ntc_last_error()
    assert L.ntc_long_plan(kmax, bad + 16, 1000, C.byref(m), C.byref(rem)) == 0
    with pytest.raises(nt.NtcError) as ei:
        nt.long_plan(kmax, bad, 1000)
    assert ei.value.code == -1
    # and the submit itself refuses a malformed piece_len before it looks at an engine or a device
    offs = (C.c_uint64 * 2)(0, 1000)
    assert L.ntc_submit_long_device(None, C.c_void_p(0x1000), offs, 1, bad + 8) == -1 and b"piece_len" in L.ntc_last_error()
