"""GPU tests of ntc_signature_sort_device (include/ntcard_hip.h; ntcard_amd/csrc/ntc_sig_sort.hip): a stable sort of (uint64 key, uint32 value) pairs against
np.argsort(kind="stable").  The values are 0 .. n - 1, so the order equal keys come out in is observable.  The sizes go round the one-launch limit and the
pairs of a workgroup (both 4096), the rounds of a wave (64) and a workgroup (256 .. 1024), whole and broken tiles, and many tiles (2^20 + 1)."""
import ctypes as C

import numpy as np
import pytest
from gpu_support import nt  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_ARG = -1
ONE_LAUNCH = TILE = 4096
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 70001, 2**20 + 1]
SET_SIZES = [ONE_LAUNCH - 1, ONE_LAUNCH, ONE_LAUNCH + 1, 70001]  # TILE +- 1 are the same three


def u64(n, seed):
    return np.random.default_rng(seed).integers(0, 2**64, size=n, dtype=np.uint64)


def sig_shaped(n, seed):
    """ntComp's two patterns at s = 7 in front (sample 0: the top eight bits are 1; sample 1: the top seven are 63), random behind"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    one = (np.uint64(1) << np.uint64(56)) | (r & np.uint64(2**56 - 1))
    two = (np.uint64(63) << np.uint64(57)) | (r & np.uint64(2**57 - 1))
    return np.where(rng.integers(0, 2, size=n) == 0, one, two)


def all_but_one(n, where):
    k = np.full(n, 0x0123456789abcdef, dtype=np.uint64)
    k[where] = 0xfedcba9876543210  # differs from the rest in every digit: no pass is skipped
    return k


KEY_SETS = {
    "uniform": lambda n: u64(n, 1),
    "all_equal": lambda n: np.full(n, 0x8000000000000001, dtype=np.uint64),
    "all_but_first": lambda n: all_but_one(n, 0),
    "all_but_last": lambda n: all_but_one(n, -1),
    "top_byte_only": lambda n: (u64(n, 2) & np.uint64(0xff00000000000000)) | np.uint64(0x00123456789abcde),
    "low_byte_only": lambda n: (u64(n, 3) & np.uint64(0xff)) | np.uint64(0x7e123456789abc00),
    "sixteen_values": lambda n: u64(16, 4)[np.random.default_rng(5).integers(0, 16, size=n)],
    "ascending": lambda n: np.sort(u64(n, 6)),
    "descending": lambda n: np.unique(u64(n + 64, 7))[::-1][:n].copy(),
    "extremes": lambda n: np.concatenate([u64(n - 4, 8), np.array([0, 2**64 - 1, 0, 2**64 - 1], dtype=np.uint64)])[np.random.default_rng(9).permutation(n)],
    "signature_shaped": lambda n: sig_shaped(n, 10),
}


def check_sort(nt, keys, with_vals=True):
    n = keys.size
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.arange(n, dtype=torch.int32).cuda() if with_vals else None
    nt.signature_sort_device(dk.data_ptr() if n else 0, dv.data_ptr() if with_vals and n else 0, n)
    order = np.argsort(keys, kind="stable")
    got = dk.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, keys[order])
    if with_vals:
        assert np.array_equal(dv.cpu().numpy().view(np.uint32), order.astype(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_uniform_keys_at_every_size(nt, n):
    check_sort(nt, u64(n, 100 + n))


@pytest.mark.parametrize("n", SET_SIZES)
@pytest.mark.parametrize("name", sorted(KEY_SETS))
def test_key_sets(nt, name, n):
    keys = KEY_SETS[name](n)
    assert keys.size == n and keys.dtype == np.uint64
    if name == "descending":
        assert np.all(keys[:-1] > keys[1:])
    check_sort(nt, keys)


@pytest.mark.parametrize("n", [2, 65] + SET_SIZES)
def test_keys_only(nt, n):
    check_sort(nt, u64(n, 200 + n), with_vals=False)
    check_sort(nt, KEY_SETS["sixteen_values"](n), with_vals=False)


def test_argument_errors(nt):
    L = nt._abi.lib()
    assert L.ntc_signature_sort_device(0, None, None, None, 1) == ERR_ARG and b"null" in L.ntc_last_error()
    keys = u64(8, 11)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    dv = torch.arange(8, dtype=torch.int32).cuda()
    assert L.ntc_signature_sort_device(0, None, C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), 2**32) == ERR_ARG  # nothing is launched:
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys) and dv.cpu().tolist() == list(range(8))  # the first eight pairs are as they were
    assert L.ntc_signature_sort_device(0, None, None, None, 0) == 0
