"""CPU tests of the spaced-seed entry points (include/ntcard_hip.h: ntc_create_seeded, ntc_hash_dump_seed_device) and of
`ntcard --seed`: the symbols exist, and every malformed argument is refused before a device is looked for."""
import ctypes as C
import functools

import pytest

from ntcard_amd import _abi
from support import NTCARD, ROOT, abi_config, run_cli

ERR_ARG = -1


cfg = functools.partial(abi_config, k=None, r_bits=20)  # the seeded create: no k list


def create_seeded(seeds, c=None):
    L = _abi.lib()
    arr = (C.c_char_p * max(1, len(seeds)))(*[s if isinstance(s, bytes) else s.encode() for s in seeds])
    h = C.c_void_p()
    rc = L.ntc_create_seeded(C.byref(c if c is not None else cfg()), len(seeds), arr, C.byref(h))
    return rc, h


def test_library_exports_the_seed_entry_points():
    L = _abi.lib()
    for name in ("ntc_create_seeded", "ntc_hash_dump_seed_device"):
        assert hasattr(L, name) and name in _abi.ABI_SYMBOLS
    assert L.ntc_abi_version() == 6 and L.ntc_max_k() == 600


@pytest.mark.parametrize("seeds", [
    ["1110x111"],           # a character other than 0 / 1
    ["11102111"],
    [""],                   # empty mask
    ["0000"],               # no '1'
    ["1" * 601],            # longer than ntc_max_k()
    ["111", "000"],         # the second one is bad
    ["1"] * 33,             # more than NTC_MAX_K_LIST masks
    [],                     # none
])
def test_create_seeded_rejects_bad_masks_before_the_device(seeds):
    rc, h = create_seeded(seeds)
    assert rc == ERR_ARG and not h.value
    assert b"device" not in _abi.lib().ntc_last_error()


@pytest.mark.parametrize("c", [cfg(n_k=1), cfg(k=[12], n_k=0), cfg(gap=2), cfg(flags=1 << 20)])
def test_create_seeded_rejects_a_k_list_or_gap_in_the_config(c):
    rc, h = create_seeded(["110011"], c)
    assert rc == ERR_ARG and not h.value


def test_create_seeded_rejects_spaced_seeds_on_the_simple_kernel():
    rc, h = create_seeded(["110011"], cfg(flags=1))  # NTC_FLAG_SIMPLE_KERNEL
    assert rc == ERR_ARG and b"production kernel" in _abi.lib().ntc_last_error()


def test_create_seeded_reaches_the_device_probe_with_good_masks():
    """a well-formed call gets as far as the device probe: on a machine without a GPU that is the device error"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present (the GPU tests create seeded engines)")
    rc, h = create_seeded(["111110011111", "1" * 31, "101"])
    assert rc == -2 and not h.value


@pytest.mark.parametrize("seed", [b"11x1", b"", b"000", b"1" * 601])
def test_hash_dump_seed_rejects_bad_masks_before_the_device(seed):
    L = _abi.lib()
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint64 * 64)()
    cnt = (C.c_uint32 * 4)()
    addr = (C.addressof(buf) + 15) & ~15
    rc = L.ntc_hash_dump_seed_device(0, None, C.c_void_p(addr), 1, 8, 8, seed, 8, C.cast(out, C.c_void_p), C.cast(cnt, C.c_void_p))
    assert rc == ERR_ARG
    rc = L.ntc_hash_dump_seed_device(0, None, C.c_void_p(addr), 1, 8, 8, None, 8, C.cast(out, C.c_void_p), C.cast(cnt, C.c_void_p))
    assert rc == ERR_ARG


@pytest.mark.parametrize("args,msg", [
    (["--seed=111110011111", "-k", "12"], "cannot be combined with -k or -g"),
    (["--seed=111110011111", "-g", "2"], "cannot be combined with -k or -g"),
    (["--seed=1110N0111"], "is not a mask"),
    (["--seed=000000"], "is not a mask"),
    (["--seed=111,"], "is not a mask"),
    (["--seed=" + "1" * 601], "longer than"),
])
def test_cli_seed_argument_errors(tmp_path, args, msg):
    src = tmp_path / "r.fa"
    src.write_text(">r\nACGTACGTACGTACGTACGT\n")
    r = run_cli(NTCARD, args + ["-p", "x", str(src)], cwd=tmp_path, text=True)
    assert r.returncode == 1
    assert msg in r.stderr and "--help" in r.stderr
    assert not list(tmp_path.glob("x_*"))


def test_cli_help_lists_seed():
    r = run_cli(NTCARD, ["--help"], cwd=ROOT, text=True)
    assert r.returncode == 0 and "--seed=MASK" in r.stderr
