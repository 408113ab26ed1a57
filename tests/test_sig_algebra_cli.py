"""Host tests of `ntsig merge | intersect | subtract | filter | hist` (ntcard_amd/csrc/ntsig_cli.cpp): what they check before a device is looked for — their
arguments, which end in a usage block of their own, and the files' headers — and that every older error path still ends in the pinned usage().  The results
themselves are tests/test_sig_algebra_cli_gpu.py's."""
import os

import numpy as np
import pytest

import ntcard_amd as nt
from support import NTSIG, run_cli
from test_sig_gather_cli import HASHES, HEADER, USAGE

COMMANDS = ("merge", "intersect", "subtract", "filter", "hist")
USAGE_ALGEBRA_HEAD = (b"Usage: ntsig merge     -o OUT.sig A.sig [B.sig ...]\n       ntsig intersect -o OUT.sig A.sig REF.sig [REF.sig ...]\n"
                      b"       ntsig subtract  -o OUT.sig A.sig REF.sig [REF.sig ...]\n       ntsig filter    [--min-count N] [--max-count N] -o OUT.sig A.sig\n"
                      b"       ntsig hist      [-c COV] F.sig\n")


def ntsig(*args):
    return run_cli(NTSIG, args, timeout=60)


@pytest.fixture
def files(tmp_path):
    nt.signature_write(tmp_path / "a.sig", HEADER, HASHES, np.ones(10, np.uint32))
    nt.signature_write(tmp_path / "b.sig", HEADER, HASHES[:5], np.ones(5, np.uint32))
    return tmp_path / "a.sig", tmp_path / "b.sig", tmp_path / "out.sig"


def test_argument_errors_print_the_new_commands_own_usage(files):
    a, b, out = files
    o = ("-o", out)
    cases = [(c,) for c in COMMANDS] + [
        ("merge", *o), ("merge", a), ("merge", "-o"), ("merge", a, "-o"), ("merge", *o, *o, a), ("merge", "--frob", *o, a), ("merge", "-c", "5", *o, a),
        ("merge", "--min-count", "2", *o, a), ("merge", *o, *([a] * 1025)),
        ("intersect", *o, a), ("intersect", a, b), ("intersect", "--max-count", "2", *o, a, b), ("intersect", *o, *([a] * 1026)),
        ("subtract", *o, a), ("subtract", a, b), ("subtract", *o, *([a] * 1026)),
        ("filter", *o), ("filter", a), ("filter", *o, a, b), ("filter", "--min-count", "x", *o, a), ("filter", "--min-count", *o, a), ("filter", "--min-count", "-1", *o, a),
        ("filter", "--min-count", "3", "--max-count", "2", *o, a), ("filter", "--min-count", "4294967296", *o, a), ("filter", "--max-count", "3x", *o, a),
        ("hist", a, b), ("hist", "-c", "0", a), ("hist", "-c", "65536", a), ("hist", "-c", "x", a), ("hist", "-c", a), ("hist", *o, a), ("hist", "--min-count", "1", a),
    ]
    for args in cases:
        r = ntsig(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr.startswith(USAGE_ALGEBRA_HEAD) and USAGE not in r.stderr, args
        assert b"nominal sampling rate" in r.stderr and not os.path.exists(out), args


def test_the_older_error_paths_still_print_the_pinned_usage(files):
    a, b, out = files
    for args in ((), ("frob",), ("union", "-o", out, a), ("info",), ("info", a, b), ("compare", a), ("matrix",), ("matrix", "--containment"), ("gather", a),
                 ("gather", "--threshold", "x", a, b)):
        r = ntsig(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr == USAGE, args


@pytest.mark.parametrize("field,other", [("k", dict(HEADER, k=24, mask="1" * 24)), ("sBits", dict(HEADER, s_bits=11)), ("strand", dict(HEADER, strand=1))])
@pytest.mark.parametrize("command", ["merge", "intersect", "subtract"])
def test_files_counted_differently_are_refused_before_a_device_is_looked_for(files, tmp_path, command, field, other):
    a, b, out = files
    nt.signature_write(tmp_path / "c.sig", other, HASHES, np.ones(10, np.uint32))
    r = ntsig(command, "-o", out, a, b, tmp_path / "c.sig")
    assert r.returncode != 0 and r.stdout == b"" and not os.path.exists(out) and not os.path.exists(str(out) + ".part")
    assert ("(%s differs)" % field).encode() in r.stderr and b"were counted differently" in r.stderr and b"device" not in r.stderr.replace(b"_device", b"")
    assert str(a).encode() in r.stderr and str(tmp_path / "c.sig").encode() in r.stderr


@pytest.mark.parametrize("command", COMMANDS)
def test_a_file_that_is_no_signature_gives_the_readers_message(files, tmp_path, command):
    a, b, out = files
    (tmp_path / "junk.sig").write_bytes(b"not a signature")
    junk = tmp_path / "junk.sig"
    args = {"merge": ("-o", out, a, junk), "intersect": ("-o", out, a, junk), "subtract": ("-o", out, junk, a), "filter": ("-o", out, junk), "hist": (junk,)}[command]
    r = ntsig(command, *args)
    assert r.returncode != 0 and r.stdout == b"" and b"not a signature file" in r.stderr and not os.path.exists(out)
    r = ntsig(command, *[tmp_path / "missing.sig" if x is junk else x for x in args])
    assert r.returncode != 0 and r.stdout == b"" and b"cannot read" in r.stderr and not os.path.exists(out)
