"""`ntbloom count`, `solid`, `query --min-count` and `info` on a counting filter, without a GPU (ntcard_amd/csrc/ntbloom_cli.cpp): every malformed argument
is refused with a message that names it, before a device is looked for, and `info` prints a `.cbf` file's header there."""
import ctypes as C
import os

import numpy as np
import pytest

from ntcard_amd import _abi
from support import run, swap, without

COUNT = ["-k", "32", "-m", "4096", "-o", "out.cbf", "reads.fa"]
SOLID = ["--min-count", "2", "--hist", "s.hist", "--fpr", "0.01", "-o", "out.bf", "in.cbf", "reads.fa"]


def write_filter(path, counting, m=77, k=21, h=4, strand=2, inserted=9, first=0x81):
    img = np.zeros(m if counting else (m + 7) // 8, dtype=np.uint8)
    img[0] = first
    hd = _abi.NtcBloomHeader(k=k, n_hash=h, strand=strand, reserved=0, m_bits=m, n_inserted=inserted)
    write = _abi.lib().ntc_cbloom_write if counting else _abi.lib().ntc_bloom_write
    assert write(str(path).encode(), C.byref(hd), img.ctypes.data_as(C.c_void_p)) == 0


REFUSALS = [
    (["count"] + without(COUNT, "-k"), b"count needs -k"),
    (["count"] + swap(COUNT, "-k", "0"), b"-k is not a number of 1 .. ntc_max_k(): 0"),
    (["count", "-H", "33"] + COUNT, b"-H is not a number of 1 .. 32: 33"),
    (["count"] + swap(COUNT, "-m", "0"), b"-m is not a number of 1 .. 2^40 - 1: 0"),
    (["count"] + swap(COUNT, "-m", str(1 << 40)), b"-m is not a number"),
    (["count"] + without(COUNT, "-m"), b"count needs exactly one of -m COUNTERS, --distinct N and --hist FILE"),
    (["count", "--distinct", "1000", "--fpr", "0.01"] + COUNT, b"exactly one of"),
    (["count", "--fpr", "0.01"] + COUNT, b"--fpr goes with --distinct or --hist"),
    (["count", "--distinct", "1000"] + without(COUNT, "-m"), b"need --fpr"),
    (["count", "--hist", "none.hist", "--fpr", "0.01"] + without(COUNT, "-m"), b"no F0 line of a .hist file in: none.hist"),
    (["count", "--strand=sideways"] + COUNT, b"--strand is none of canonical, forward, reverse: sideways"),
    (["count", "--min-count", "2"] + COUNT, b"unknown option: --min-count"),
    (["count"] + without(COUNT, "-o"), b"count needs -o OUT.cbf"),
    (["count"] + COUNT[:-1], b"count needs at least one input file"),
    (["solid"] + without(SOLID, "--min-count"), b"solid needs --min-count C"),
    (["solid"] + swap(SOLID, "--min-count", "0"), b"--min-count is not a number of 1 .. 255: 0"),
    (["solid"] + swap(SOLID, "--min-count", "256"), b"--min-count is not a number of 1 .. 255: 256"),
    (["solid"] + swap(SOLID, "--min-count", "two"), b"--min-count is not a number of 1 .. 255: two"),
    (["solid"] + without(SOLID, "-o"), b"solid needs -o OUT.bf"),
    (["solid", "--min-count", "2", "-o", "out.bf"], b"solid needs IN.cbf"),
    (["solid"] + without(SOLID, "--hist"), b"solid with input files needs --hist FILE and --fpr P"),
    (["solid"] + without(SOLID, "--fpr"), b"solid with input files needs --hist FILE and --fpr P"),
    (["solid"] + swap(SOLID, "--fpr", "1"), b"--fpr is not a number inside (0, 1): 1"),
    (["solid", "-H", "0"] + SOLID, b"-H is not a number of 1 .. 32: 0"),
    (["solid"] + SOLID[:-1], b"--hist, --fpr and -H go with input files"),
    (["solid", "-k", "32"] + SOLID, b"unknown option: -k"),
    (["solid"] + swap(SOLID, "-o", "out.bf")[:-2] + ["none.cbf", "reads.fa"], b"cannot read none.cbf"),
    (["solid"] + SOLID[:-2] + ["plain.bf", "reads.fa"], b"plain.bf is not a counting filter file"),
    (["solid"] + swap(SOLID, "--hist", "none.hist"), b"no F0 line of a .hist file in: none.hist"),
    (["solid"] + swap(swap(SOLID, "--hist", "short.hist"), "--min-count", "4"), b"the f_i lines of the .hist file stop below --min-count - 1: short.hist"),
    (["solid"] + swap(SOLID, "--hist", "all_once.hist"), b"F0 minus the f_i below --min-count is 0 in: all_once.hist"),
    (["solid"] + swap(SOLID, "--hist", "over.hist"), b"sum to more than its F0: over.hist"),
    (["solid"] + swap(SOLID, "--fpr", "1e-9"), b"2^40 bits or more"),
    (["query", "--min-count"], b"missing value behind: --min-count"),
    (["query", "--min-count", "0", "in.cbf", "reads.fa"], b"--min-count is not a number of 1 .. 255: 0"),
    (["query", "--min-count", "2", "plain.bf", "reads.fa"], b"--min-count goes with a counting filter (.cbf), not with: plain.bf"),
    (["query", "--min-count", "2", "in.cbf"], b"query needs F.bf and at least one input file"),
    (["query", "in.cbf", "--min-count", "2", "reads.fa"], b"unknown option: --min-count"),
    (["query", "--min-count", "2", "none.cbf", "reads.fa"], b"cannot read none.cbf"),
]


@pytest.mark.parametrize("args,message", REFUSALS, ids=[" ".join(a[:3]) + f" #{i}" for i, (a, _) in enumerate(REFUSALS)])
def test_malformed_arguments_are_refused_by_name(args, message, tmp_path):
    (tmp_path / "reads.fa").write_bytes(b">r\nACGT\n")
    write_filter(tmp_path / "in.cbf", True)
    write_filter(tmp_path / "plain.bf", False)
    (tmp_path / "s.hist").write_bytes(b"F1\t1000\nF0\t600\n1\t400\n2\t100\n3\t50\n")
    (tmp_path / "short.hist").write_bytes(b"F1\t1000\nF0\t600\n1\t400\n2\t100\n")  # lines up to f_2: enough for --min-count 3, not for 4
    (tmp_path / "all_once.hist").write_bytes(b"F1\t600\nF0\t600\n1\t600\n2\t0\n")
    (tmp_path / "over.hist").write_bytes(b"F1\t600\nF0\t600\n1\t601\n")
    if "1e-9" in args:
        (tmp_path / "s.hist").write_bytes(b"F1\t99\nF0\t%d\n1\t5\n" % 10**12)
    r = run(args, tmp_path)
    assert r.returncode != 0 and r.stdout == b""
    assert message in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr  # refused before a device is looked for
    for name in ("out.bf", "out.cbf"):
        assert not os.path.exists(tmp_path / name) and not os.path.exists(tmp_path / (name + ".part"))


def test_info_prints_the_header_of_a_counting_filter(tmp_path):
    write_filter(tmp_path / "f.cbf", True, first=255)
    r = run(["info", "f.cbf"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert lines["k"] == "21" and lines["hashes"] == "4" and lines["strand"] == "reverse" and lines["counters"] == "77" and lines["inserted"] == "9"
    assert "bits" not in lines
    import torch
    if torch.cuda.is_available():
        assert lines["nonzero"] == "1" and lines["saturated"] == "1" and float(lines["occupancy"]) == pytest.approx(1 / 77, abs=1e-6)
    else:
        assert "nonzero" not in lines
    # the magic decides: a counting filter under the name of a plain one is still a counting filter, and a damaged one is refused
    os.rename(tmp_path / "f.cbf", tmp_path / "g.bf")
    r = run(["info", "g.bf"], tmp_path)
    assert r.returncode == 0 and b"counters\t77" in r.stdout
    (tmp_path / "cut.cbf").write_bytes((tmp_path / "g.bf").read_bytes()[:-1])
    r = run(["info", "cut.cbf"], tmp_path)
    assert r.returncode != 0 and b"cut short" in r.stderr and r.stdout == b""
