"""Host tests of `ntsig matrix` (ntcard_amd/csrc/ntsig_cli.cpp): what it checks before a device is looked for — its arguments, the files' headers, the
reader's refusals.  The matrix itself is tests/test_sig_matrix_cli_gpu.py's."""

import numpy as np
import pytest

import ntcard_amd as nt
from support import NTSIG, run_cli

HEADER = dict(k=32, gap=0, strand=0, hpc=0, s_bits=7, mask="1" * 32)
HASHES = np.arange(1, 11, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 8)


def ntsig(*args):
    return run_cli(NTSIG, args, timeout=60)


def test_matrix_without_a_file_is_a_usage_error():
    for args in (("matrix",), ("matrix", "--containment")):
        r = ntsig(*args)
        assert r.returncode != 0 and r.stdout == b""
        assert b"Usage: ntsig info" in r.stderr and b"ntsig matrix [--containment] A.sig B.sig ..." in r.stderr


@pytest.mark.parametrize("field,other", [("k", dict(HEADER, k=24, mask="1" * 24)), ("sBits", dict(HEADER, s_bits=11))])
@pytest.mark.parametrize("flag", [(), ("--containment",)])
def test_matrix_refuses_files_counted_differently(tmp_path, field, other, flag):
    nt.signature_write(tmp_path / "a.sig", HEADER, HASHES, np.ones(10, np.uint32))
    nt.signature_write(tmp_path / "b.sig", HEADER, HASHES[:5], np.ones(5, np.uint32))
    nt.signature_write(tmp_path / "c.sig", other, HASHES, np.ones(10, np.uint32))
    r = ntsig("matrix", *flag, tmp_path / "a.sig", tmp_path / "b.sig", tmp_path / "c.sig")
    assert r.returncode != 0 and r.stdout == b""
    assert ("(%s differs)" % field).encode() in r.stderr and b"were counted differently" in r.stderr
    assert str(tmp_path / "a.sig").encode() in r.stderr and str(tmp_path / "c.sig").encode() in r.stderr


def test_matrix_gives_the_readers_message_for_a_file_that_is_no_signature(tmp_path):
    nt.signature_write(tmp_path / "a.sig", HEADER, HASHES, np.ones(10, np.uint32))
    (tmp_path / "junk.sig").write_bytes(b"not a signature")
    r = ntsig("matrix", tmp_path / "a.sig", tmp_path / "junk.sig")
    assert r.returncode != 0 and r.stdout == b"" and b"not a signature file" in r.stderr
    r = ntsig("matrix", tmp_path / "a.sig", tmp_path / "missing.sig")
    assert r.returncode != 0 and r.stdout == b"" and b"cannot read" in r.stderr
