"""GPU tests of gather above its caps (ntcard_amd/csrc/ntc_sig_gather.hip, ntc_sig_lists.hip; DESIGN.md §4, the table of grid caps).  The count, clear, rest and ascent kernels
cap their grids and walk the rest in a grid-stride loop, the search runs at most 2^18 work items per launch and the pick walks the references 256 at a
time: each case here is the smallest that takes such a loop into a second turn, asserts the size that makes it do so before it touches the device, and is
compared with tests/sig_gather_model.py."""
import functools

import numpy as np
import pytest

import sig_gather_model
from gpu_support import nt  # noqa: F401
from support import ERR_ARG
from test_sig_gather_gpu import checked, on_device

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHUNK = 4096                      # entries (search) or hits (count) per work item
SEARCH_ITEMS = 2**18              # search work items per launch
COUNT_BLOCKS = 1024               # gather_count_kernel: work items per turn
CLEAR_STRIDE = 1024 * 256         # gather_clear_kernel, gather_rest_kernel: hits / query entries per turn
ASCENT_STRIDE = 1024 * 256        # sig_ascent_kernel (SigLists): the first turn covers the entries 1 .. ASCENT_STRIDE
PICK_THREADS = 256                # gather_pick_kernel: references per turn
MAX_REFS = 1024


@functools.lru_cache(maxsize=None)
def big_pool():
    p = np.unique(np.random.default_rng(91).integers(1, 2**64 - 1, size=2_400_000, dtype=np.uint64))
    assert p.size == 2_400_000
    p.setflags(write=False)
    return p


def test_count_kernel_takes_a_second_turn(nt):
    p = big_pool()
    q = p[:6000]
    counts = np.arange(1, q.size + 1, dtype=np.uint32)
    small = [q[4097 + i: 4098 + i] for i in range(MAX_REFS - 1)]
    refs = small + [q[:CHUNK + 1]]
    items = sum(-(-r.size // CHUNK) for r in refs)  # every entry of every reference is a hit
    assert len(refs) == MAX_REFS and items == COUNT_BLOCKS + 1  # the last reference's second item — one hit — is the second turn of workgroup 0
    rows, rest, _ = checked(nt, q, counts, refs, max_rows=5)
    assert rows["ref"].tolist() == [1023, 0, 1, 2, 3] and rows["unique"].tolist() == [CHUNK + 1, 1, 1, 1, 1] and rest == q.size - CHUNK - 5
    assert int(rows["unique_weight"][0]) == (CHUNK + 1) * (CHUNK + 2) // 2


def test_clear_and_rest_kernels_take_a_second_turn(nt):
    p = big_pool()
    q = p[:300_000]
    counts = np.random.default_rng(92).integers(1, 2**32, size=q.size, dtype=np.uint64).astype(np.uint32)
    first = q[10_000: 10_000 + CLEAR_STRIDE + 2]
    refs = [q[272_100:272_200], first, first.copy(), q[5000:10_050]]
    assert first.size > CLEAR_STRIDE and q.size > CLEAR_STRIDE and q.size - first.size < CLEAR_STRIDE
    # every hit of `first` has to be cleared: its copy then counts nothing and is never reported, and reference 0 keeps 54 of its 100 entries
    rows, rest, rest_w = checked(nt, q, counts, refs)
    assert rows["ref"].tolist() == [1, 3, 0] and rows["unique"].tolist() == [first.size, 5000, 54] and rest == q.size - first.size - 5054
    assert rest_w == int(counts.astype(np.uint64).sum(dtype=np.uint64)) - int(rows["unique_weight"].sum(dtype=np.uint64)) > 2**40


@pytest.mark.parametrize("which", ["query", "reference"])
def test_ascent_beyond_the_first_turn(nt, which):
    p = big_pool()
    at = ASCENT_STRIDE + 1  # the first entry of the second turn
    bad = p[:ASCENT_STRIDE + 10].copy()
    bad[at] = bad[at - 2]
    assert bad.size > at > ASCENT_STRIDE and np.flatnonzero(bad[:-1] >= bad[1:]).tolist() == [at - 1]
    good = p[1000:3000]
    q, refs = (bad, [good, good[:50]]) if which == "query" else (good, [good[:50], bad])
    keep, pq, _, ptrs, ns = on_device(q, None, refs)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_gather_device(pq, 0, q.size, ptrs, ns)
    assert ei.value.code == ERR_ARG and ("the query is" if which == "query" else "reference 1 is") in str(ei.value) and f"entry {at} " in str(ei.value)
    del keep


def test_search_takes_a_second_launch(nt):
    """1024 references of 257 work items each: two arrays, listed 1020 and 4 times, so that the device holds 25 MB and the model looks two lists up"""
    p = big_pool()
    n = 256 * CHUNK + 1
    q = p[1_200_000: 1_200_000 + n + 5000]
    a = np.concatenate([p[:n - 3000], q[-6000:-3000]])  # the hits are a list's LAST entries: 3000 common,
    b = np.concatenate([p[:n - 4000], q[-4000:]])       # 4000 common, 1000 of them a's
    refs = [a] * 1020 + [b] * 4
    items = sum(-(-min(r.size, q.size) // CHUNK) for r in refs)
    assert a.size == b.size == n and q.size >= n and bool(np.all(a[:-1] < a[1:])) and bool(np.all(b[:-1] < b[1:]))
    # the second launch: the last 253 work items of the first b, its hits among them, and the other three b
    assert len(refs) == MAX_REFS and SEARCH_ITEMS < items == MAX_REFS * 257 and items - SEARCH_ITEMS == 4 * 256 and 1020 * 257 + 4 == SEARCH_ITEMS
    keep, pq, _, ptrs, ns = on_device(q, None, refs)
    got = nt.signature_gather_device(pq, 0, q.size, ptrs, ns)
    del keep
    rows, rest, _ = got
    assert sig_gather_model.same(got, sig_gather_model.gather(q, None, refs))
    assert rows.tolist() == [(1020, 0, 4000, 4000, 4000), (0, 0, 3000, 2000, 2000)] and rest == q.size - 6000


def test_pick_walks_the_references_in_two_turns(nt):
    p = big_pool()
    sizes = [10 + (i % 7) for i in range(300)]
    sizes[299], sizes[2], sizes[290], sizes[256] = 40, 30, 30, 30
    offs = np.concatenate([[0], np.cumsum(sizes)])
    refs = [p[int(x): int(y)] for x, y in zip(offs[:-1], offs[1:])]
    q = p[:int(offs[-1]) + 9]
    assert len(refs) > PICK_THREADS and max(sizes[:PICK_THREADS]) == 30 < sizes[299]
    rows, rest, _ = checked(nt, q, None, refs, threshold=16)
    assert rows["ref"].tolist()[:4] == [299, 2, 256, 290] and rows["unique"].tolist()[:5] == [40, 30, 30, 30, 16] and rows["ref"][4] == 6
    assert rows.size == 4 + sum(1 for s in sizes if s == 16) and rest == q.size - int(rows["unique"].sum())
