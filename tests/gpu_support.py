"""What the GPU tests share: the `nt` fixture, uploads, and the long-sequence route (include/ntcard_hip.h: ntc_submit_long_device).  tests/support.py holds
what needs no device.  A test module imports the fixture by name: `from gpu_support import nt  # noqa: F401`."""
import functools

import numpy as np
import pytest

from support import offsets_of, to_slots

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def nt():
    assert torch.cuda.is_available(), "GPU tests need a HIP device (run on the MI355X box)"
    import ntcard_amd
    return ntcard_amd


def dev(a):
    """numpy array -> device tensor"""
    return torch.from_numpy(a).cuda()


def on_device(seqs_or_buf, offs=None, lead=3):
    """sequences (a list of bytes; or the sequences [offs[i], offs[i + 1]) of a uint8 array) behind one another in one device buffer, `lead` bytes in
    front (start offsets of any alignment) and one behind, all '#' -> (tensor, host offsets)"""
    if offs is None:
        host = np.frombuffer(b"#" * lead + b"".join(seqs_or_buf) + b"#", dtype=np.uint8).copy()
        offs = offsets_of(seqs_or_buf, lead)
    else:
        host = np.concatenate([np.full(lead, ord("#"), dtype=np.uint8), seqs_or_buf, np.full(1, ord("#"), dtype=np.uint8)])
        offs = (offs + np.uint64(lead)).astype(np.uint64)
    d = dev(host)
    assert d.data_ptr() % 4 == 0
    return d, offs


@functools.lru_cache(maxsize=None)
def device_slots(reads, L, stride):
    """reads (a tuple) of L bases in row slots on the device, uploaded once -> (tensor, n, L, stride)"""
    assert all(len(r) == L for r in reads)
    return dev(to_slots(reads, stride)), len(reads), L, stride


def submit_slots(e, reads, L=150, stride=152):
    d, n, L, stride = device_slots(tuple(reads), L, stride)
    e.submit_device(d.data_ptr(), n, L, stride)


def planned(nt, lens, kmax, pl):
    """what ntc_long_stats must report for sequences of these lengths: (full pieces, sequences with one)"""
    m = [nt.long_plan(kmax, pl, int(n))[0] for n in lens]
    return sum(m), sum(1 for x in m if x)


def count_long(nt, d, offs, klist, piece_len, gap=0, flags=0, submits=1, r_bits=14, s_bits=7):
    """-> (t_Counter, F1, long_stats) of an engine that takes the device buffer through ntc_submit_long_device"""
    with nt.Engine(list(klist), gap=gap, r_bits=r_bits, s_bits=s_bits, flags=flags) as e:
        for _ in range(submits):
            e.submit_long_device(d.data_ptr(), offs, piece_len)
        tc, _, f1 = e.finish(counters=True)
        return tc, f1, e.long_stats()
