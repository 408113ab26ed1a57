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


def upload(a, stream=None, into=None):
    """numpy array (or a pinned host tensor) -> device tensor by a copy ON `stream` (a torch.cuda.Stream; None: the current one) that the host does not wait
    for: whatever reads the tensor must be ordered behind that stream.  into: an existing device tensor to overwrite instead of a new one.
    -> (tensor, the pinned host tensor the copy reads: keep it until the stream has passed).  tests/test_engine_seq_gpu.py (test_shared_helpers) pins it
    and tests/devview.py's DevArray, which need a device."""
    pinned = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    assert pinned.is_pinned()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        t = into if into is not None else torch.empty(pinned.shape, dtype=pinned.dtype, device="cuda")
        t.copy_(pinned, non_blocking=True)
    return t, pinned


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
