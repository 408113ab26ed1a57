"""`ntbloom` without a GPU (ntcard_amd/csrc/ntbloom_cli.cpp): every malformed argument is refused with a message that names it, before a device is looked
for — so the refusals are the same on a machine without one — and `info` prints a filter file's header there."""
import ctypes as C
import os

import numpy as np
import pytest

from ntcard_amd import _abi
from support import run, swap, without

GOOD = ["-k", "32", "-m", "4096", "-o", "out.bf", "reads.fa"]


REFUSALS = [
    ([], b"no command"),
    (["make"], b"unknown command: make"),
    (["build"] + without(GOOD, "-k"), b"build needs -k"),
    (["build"] + swap(GOOD, "-k", "0"), b"-k is not a number of 1 .. ntc_max_k(): 0"),
    (["build"] + swap(GOOD, "-k", "601"), b"-k is not a number"),
    (["build"] + swap(GOOD, "-k", "3x"), b"-k is not a number"),
    (["build"] + swap(GOOD, "-k", "-3"), b"-k is not a number"),
    (["build", "-H", "0"] + GOOD, b"-H is not a number of 1 .. 32: 0"),
    (["build", "-H", "33"] + GOOD, b"-H is not a number of 1 .. 32: 33"),
    (["build"] + swap(GOOD, "-m", "0"), b"-m is not a number of 1 .. 2^40 - 1: 0"),
    (["build"] + swap(GOOD, "-m", str(1 << 40)), b"-m is not a number"),
    (["build"] + swap(GOOD, "-m", "many"), b"-m is not a number"),
    (["build"] + without(GOOD, "-m"), b"exactly one of -m BITS, --distinct N and --hist FILE"),
    (["build", "--distinct", "1000", "--fpr", "0.01"] + GOOD, b"exactly one of"),
    (["build", "--fpr", "0.01"] + GOOD, b"--fpr goes with --distinct or --hist"),
    (["build", "--distinct", "1000"] + without(GOOD, "-m"), b"need --fpr"),
    (["build", "--distinct", "0", "--fpr", "0.01"] + without(GOOD, "-m"), b"--distinct is not a positive number: 0"),
    (["build", "--distinct", "1000", "--fpr", "0"] + without(GOOD, "-m"), b"--fpr is not a number inside (0, 1): 0"),
    (["build", "--distinct", "1000", "--fpr", "1"] + without(GOOD, "-m"), b"--fpr is not a number inside (0, 1): 1"),
    (["build", "--distinct", "1000", "--fpr", "half"] + without(GOOD, "-m"), b"--fpr is not a number inside (0, 1): half"),
    (["build", "--distinct", str(10**12), "--fpr", "0.0001"] + without(GOOD, "-m"), b"2^40 bits or more"),
    (["build", "--hist", "none.hist", "--fpr", "0.01"] + without(GOOD, "-m"), b"no F0 line of a .hist file in: none.hist"),
    (["build", "--strand=sideways"] + GOOD, b"--strand is none of canonical, forward, reverse: sideways"),
    (["build", "--hpc"] + GOOD, b"unknown option: --hpc"),
    (["build"] + without(GOOD, "-o"), b"build needs -o OUT.bf"),
    (["build"] + GOOD[:-1], b"at least one input file"),
    (["build"] + GOOD[:-1] + ["-o"], b"missing value behind: -o"),
    (["query"], b"query needs F.bf and at least one input file"),
    (["query", "f.bf"], b"query needs F.bf and at least one input file"),
    (["query", "-x", "f.bf", "reads.fa"], b"unknown option: -x"),
    (["query", "none.bf", "reads.fa"], b"cannot read none.bf"),
    (["info"], b"info takes one file"),
    (["info", "a.bf", "b.bf"], b"info takes one file"),
    (["info", "none.bf"], b"cannot read none.bf"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=[" ".join(a[:4]) or "none" for a, _ in REFUSALS])
def test_malformed_arguments_are_refused_by_name(args, message, tmp_path):
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    r = run(args, tmp_path)
    assert r.returncode != 0 and r.stdout == b""
    assert message in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr  # refused before a device is looked for
    assert not os.path.exists(tmp_path / "out.bf") and not os.path.exists(tmp_path / "out.bf.part")


def test_hist_without_f0_and_files_that_are_no_filters(tmp_path):
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    (tmp_path / "bad.hist").write_bytes(b"F1\t100\nF0\tmany\n1\t5\n")
    r = run(["build", "--hist", "bad.hist", "--fpr", "0.01"] + without(GOOD, "-m"), tmp_path)
    assert r.returncode != 0 and b"no F0 line of a .hist file in: bad.hist" in r.stderr
    (tmp_path / "zero.hist").write_bytes(b"F1\t0\nF0\t0\n")
    r = run(["build", "--hist", "zero.hist", "--fpr", "0.01"] + without(GOOD, "-m"), tmp_path)
    assert r.returncode != 0 and b"F0 of the .hist file is 0" in r.stderr
    for cmd in (["info", "reads.fa"], ["query", "reads.fa", "reads.fa"]):
        r = run(cmd, tmp_path)
        assert r.returncode != 0 and b"is not a filter file" in r.stderr and r.stdout == b""


def test_info_prints_the_header(tmp_path):
    """the header of a file written by ntc_bloom_write; the popcount lines follow only where a GPU is"""
    img = np.zeros(10, dtype=np.uint8)
    img[0] = 0x81
    h = _abi.NtcBloomHeader(k=21, n_hash=4, strand=2, reserved=0, m_bits=77, n_inserted=9)
    assert _abi.lib().ntc_bloom_write(str(tmp_path / "f.bf").encode(), C.byref(h), img.ctypes.data_as(C.c_void_p)) == 0
    r = run(["info", "f.bf"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert lines["k"] == "21" and lines["hashes"] == "4" and lines["strand"] == "reverse" and lines["bits"] == "77" and lines["inserted"] == "9"
    import torch
    if torch.cuda.is_available():
        assert lines["popcount"] == "2" and float(lines["occupancy"]) == pytest.approx(2 / 77, abs=1e-6)
    else:
        assert "popcount" not in lines
