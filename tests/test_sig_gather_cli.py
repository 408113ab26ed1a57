"""Host tests of `ntsig gather` (ntcard_amd/csrc/ntsig_cli.cpp): what it checks before a device is looked for — its arguments and the files' headers.  The
decomposition itself is tests/test_sig_gather_cli_gpu.py's."""
import numpy as np
import pytest

import ntcard_amd as nt
from support import NTSIG, run_cli

HEADER = dict(k=32, gap=0, strand=0, hpc=0, s_bits=7, mask="1" * 32)
HASHES = np.arange(1, 11, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 8)
USAGE = (b"Usage: ntsig info F.sig\n       ntsig compare A.sig B.sig\n       ntsig matrix [--containment] A.sig B.sig ...\n"
         b"       ntsig gather [--threshold N] QUERY.sig REF.sig ...\n")


def ntsig(*args):
    return run_cli(NTSIG, args, timeout=60)


def test_gather_without_a_reference_is_a_usage_error(tmp_path):
    nt.signature_write(tmp_path / "q.sig", HEADER, HASHES, np.ones(10, np.uint32))
    q = tmp_path / "q.sig"
    for args in (("gather",), ("gather", q), ("gather", "--threshold"), ("gather", "--threshold", "3"), ("gather", "--threshold", "3", q),
                 ("gather", "--threshold", "x", q, q), ("gather", "--threshold", "-1", q, q), ("gather", "--threshold", "3x", q, q)):
        r = ntsig(*args)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr == USAGE, args


@pytest.mark.parametrize("field,other", [("k", dict(HEADER, k=24, mask="1" * 24)), ("sBits", dict(HEADER, s_bits=11))])
@pytest.mark.parametrize("flag", [(), ("--threshold", "2")])
def test_gather_refuses_a_reference_counted_differently(tmp_path, field, other, flag):
    """(refuse() names the header's s_bits as it prints it everywhere: sBits)"""
    nt.signature_write(tmp_path / "q.sig", HEADER, HASHES, np.ones(10, np.uint32))
    nt.signature_write(tmp_path / "a.sig", HEADER, HASHES[:5], np.ones(5, np.uint32))
    nt.signature_write(tmp_path / "b.sig", other, HASHES, np.ones(10, np.uint32))
    r = ntsig("gather", *flag, tmp_path / "q.sig", tmp_path / "a.sig", tmp_path / "b.sig")
    assert r.returncode != 0 and r.stdout == b""
    assert ("(%s differs)" % field).encode() in r.stderr and b"were counted differently" in r.stderr
    assert str(tmp_path / "q.sig").encode() in r.stderr and str(tmp_path / "b.sig").encode() in r.stderr


def test_gather_gives_the_readers_message_for_a_file_that_is_no_signature(tmp_path):
    nt.signature_write(tmp_path / "q.sig", HEADER, HASHES, np.ones(10, np.uint32))
    (tmp_path / "junk.sig").write_bytes(b"not a signature")
    r = ntsig("gather", tmp_path / "q.sig", tmp_path / "junk.sig")
    assert r.returncode != 0 and r.stdout == b"" and b"not a signature file" in r.stderr
