"""`ntbloom` and blocked filters without a GPU (ntcard_amd/csrc/ntbloom_cli.cpp): `--blocked` is refused by name where it has no meaning, before a device
is looked for, and `info` tells a blocked file by its magic and prints its header and block size there."""
import ctypes as C
import os

import numpy as np
import pytest

from ntcard_amd import _abi
from support import run, swap, without

GOOD = ["-k", "32", "-m", "4096", "-o", "out.bbf", "reads.fa"]


def write_counting(path, m=4093):
    h = _abi.NtcBloomHeader(k=32, n_hash=3, strand=0, reserved=0, m_bits=m, n_inserted=5)
    cnt = np.zeros(m, dtype=np.uint8)
    assert _abi.lib().ntc_cbloom_write(str(path).encode(), C.byref(h), cnt.ctypes.data_as(C.c_void_p)) == 0


REFUSALS = [
    (["count", "--blocked"] + GOOD, b"--blocked goes with build and solid: there is no blocked counting filter"),
    (["build", "--blocked"] + swap(GOOD, "-m", "4100"), b"-m of a blocked filter is not a multiple of 512: 4100"),
    (["build", "--blocked"] + swap(GOOD, "-m", "64"), b"-m of a blocked filter is not a multiple of 512: 64"),
    (["build", "--blocked"] + swap(GOOD, "-m", "0"), b"-m is not a number of 1 .. 2^40 - 1: 0"),
    (["build", "--blocked", "--distinct", str(10**12), "--fpr", "0.0001"] + without(GOOD, "-m"), b"ntc_bbloom_size"),
    (["build", "--blocked=yes"] + GOOD, b"unknown option: --blocked=yes"),
    (["solid", "--blocked", "--min-count", "2", "-o", "out.bbf", "in.cbf"], b"--blocked goes with input files"),
    (["solid", "--blocked", "--min-count", "2", "-o", "out.bbf", "in.cbf", "reads.fa"], b"solid with input files needs --hist FILE and --fpr P"),
    (["query", "--blocked", "f.bbf", "reads.fa"], b"unknown option: --blocked"),
    (["info", "--blocked"], b"unknown option: --blocked"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=[" ".join(a[:4]) for a, _ in REFUSALS])
def test_blocked_is_refused_by_name_where_it_has_no_meaning(args, message, tmp_path):
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    write_counting(tmp_path / "in.cbf")
    r = run(args, tmp_path)
    assert r.returncode != 0 and r.stdout == b""
    assert message in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr  # refused before a device is looked for
    assert not os.path.exists(tmp_path / "out.bbf") and not os.path.exists(tmp_path / "out.bbf.part")


def test_info_prints_a_blocked_files_header_and_block_size(tmp_path):
    """a file written by ntc_bbloom_write; the popcount lines follow only where a GPU is"""
    img = np.zeros(128, dtype=np.uint8)
    img[0], img[64] = 0x81, 0xFF  # two bits in block 0, eight in block 1
    h = _abi.NtcBloomHeader(k=21, n_hash=2, strand=2, reserved=512, m_bits=1024, n_inserted=9)
    assert _abi.lib().ntc_bbloom_write(str(tmp_path / "f.bbf").encode(), C.byref(h), img.ctypes.data_as(C.c_void_p)) == 0
    r = run(["info", "f.bbf"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert lines["k"] == "21" and lines["hashes"] == "2" and lines["strand"] == "reverse" and lines["bits"] == "1024" and lines["inserted"] == "9"
    assert lines["block"] == "512" and lines["blocks"] == "2"
    import torch
    if torch.cuda.is_available():
        assert lines["popcount"] == "10" and float(lines["occupancy"]) == pytest.approx(10 / 1024, abs=1e-6)
        assert float(lines["fpr"]) == pytest.approx(((2 / 512) ** 2 + (8 / 512) ** 2) / 2, rel=1e-4)  # per block, not (10 / 1024)^2
    else:
        assert "popcount" not in lines
    # a plain file of the same size has no block line; a blocked file with a damaged header is refused by the blocked reader's name
    h0 = _abi.NtcBloomHeader(k=21, n_hash=2, strand=2, reserved=0, m_bits=1024, n_inserted=9)
    assert _abi.lib().ntc_bloom_write(str(tmp_path / "f.bf").encode(), C.byref(h0), img.ctypes.data_as(C.c_void_p)) == 0
    r = run(["info", "f.bf"], tmp_path)
    assert r.returncode == 0 and b"block" not in r.stdout
    raw = (tmp_path / "f.bbf").read_bytes()
    (tmp_path / "bad.bbf").write_bytes(raw[:20] + b"\0\x01\0\0" + raw[24:])  # reserved = 256
    for cmd in (["info", "bad.bbf"], ["query", "bad.bbf", "f.bf"]):
        r = run(cmd, tmp_path)
        assert r.returncode != 0 and b"ntc_bbloom_read" in r.stderr and b"bad header" in r.stderr and r.stdout == b""
