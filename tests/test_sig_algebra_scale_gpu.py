"""GPU tests of the set algebra's kernels above their grid caps (ntcard_amd/csrc/ntc_sig_algebra.hip; DESIGN.md §4 "Grid caps").  Every kernel there caps its
grid and walks the rest in a grid-stride loop, and the compaction's scan walks the tile counts 256 tiles per turn: each case here is the smallest that takes
one of these loops into its second turn, asserts its size against the cap (and the cap against the source) before it touches the device, and compares with
tests/sig_algebra_model.py."""
import functools

import numpy as np
import pytest

import sig_algebra_model as model
from gpu_support import nt  # noqa: F401
from test_sig_algebra_gpu import T, dev32, library_constant, ptr, run_select, run_union, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SCAN_TURN = 256 * T          # compact_scan_kernel: entries under the tiles of one turn
SELECT_STRIDE = 3072 * 256   # select_flag_kernel: entries of A per turn
COMPACT_STRIDE = 512 * T     # compact_count_kernel, compact_scatter_kernel: entries per turn
GATHER_STRIDE = 1024 * 256   # union_gather_kernel: entries of a list per turn
HEAD_STRIDE = 1024 * 256     # union_head_kernel: pairs per turn
HIST_STRIDE = 1024 * 256     # sig_hist_kernel: counts per turn


def test_the_strides_here_are_the_librarys():
    c = library_constant
    assert (SCAN_TURN, SELECT_STRIDE, COMPACT_STRIDE) == (c("kCompactScanTiles") * c("kCompactTile"), c("kSelectBlocks") * 256, c("kCompactBlocks") * c("kCompactTile"))
    assert (GATHER_STRIDE, HEAD_STRIDE, HIST_STRIDE) == (c("kUnionGatherBlocks") * 256, c("kUnionHeadBlocks") * 256, c("kHistBlocks") * 256)
    assert HIST_STRIDE < SCAN_TURN < SELECT_STRIDE < COMPACT_STRIDE  # so every loop below has a size that takes it, and no later one, into a second turn


@functools.lru_cache(maxsize=None)
def many():
    """1 100 000 distinct hashes of [0, 2^64), ascending, 0 and 2^64 - 1 among them, with counts of 1 .. 5 (most of them 1)"""
    rng = np.random.default_rng(91)
    h = np.unique(np.concatenate([rng.integers(0, 2**64, size=1_100_100, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)]))
    h = np.sort(np.concatenate([h[:1], rng.choice(h[1:-1], size=1_099_998, replace=False), h[-1:]]))
    c = np.minimum(rng.geometric(0.7, size=h.size), 5).astype(np.uint32)
    c[-1] = 1
    h.setflags(write=False)
    c.setflags(write=False)
    return h, c


@pytest.mark.parametrize("na,loops", [(SCAN_TURN + 1, "scan"), (SELECT_STRIDE + 1, "scan, flags"), (COMPACT_STRIDE + 1, "scan, flags, count and scatter")])
def test_select_second_turns(nt, na, loops):
    assert na - 1 in (SCAN_TURN, SELECT_STRIDE, COMPACT_STRIDE)
    assert (na > SCAN_TURN, na > SELECT_STRIDE, na > COMPACT_STRIDE) == ("scan" in loops, "flags" in loops, "count" in loops)
    assert (na + T - 1) // T in (257, 385, 513)  # tiles: one more than a turn of the scan (256) and of the count and scatter kernels (512) takes
    h, c = many()
    a, ca = h[-na:], c[-na:]  # (the last entries: the last tile holds one entry, 2^64 - 1, and it is kept)
    ref = h[(h.size - 1) % 3::3]  # every third hash, the last one among them
    want = model.select(a, ca, [ref], "all", 1, 2)
    assert want[0][-1] == 2**64 - 1 and na // 4 < want[0].size < na // 3 and a[-1] in ref and ca[-1] <= 2
    assert same(run_select(nt, a, ca, [ref], "all", 1, 2), want)
    want = model.select(a, ca, [ref], "none")
    assert 2 * na // 3 - 1 <= want[0].size <= 2 * na // 3 + 1
    assert same(run_select(nt, a, ca, [ref], "none"), want)


def test_union_head_second_turn(nt):
    h, c = many()
    n = HEAD_STRIDE // 2 + 1
    lists, counts = [h[:n], h[n // 2:n // 2 + n]], [c[:n], None]
    assert 2 * n == HEAD_STRIDE + 2 and n <= GATHER_STRIDE and 2 * n <= SCAN_TURN  # the heads' second turn alone: every list is one turn of the gather
    want = model.union(lists, counts)
    assert want[0].size == n // 2 + n
    assert same(run_union(nt, lists, counts), want)


def test_union_gather_second_turn(nt):
    h, c = many()
    n = GATHER_STRIDE + 1
    lists, counts = [h[5:5 + n], h[:10], h[n:n + 20]], [c[5:5 + n], None, c[n:n + 20]]
    assert lists[0].size > GATHER_STRIDE and sum(x.size for x in lists) <= SCAN_TURN  # the long list's entry GATHER_STRIDE is a second turn's
    want = model.union(lists, counts)
    assert want[0].size == n + 5 + 15
    assert same(run_union(nt, lists, counts), want)
    assert same(run_union(nt, lists[:1], counts[:1]), (lists[0], counts[0]))  # one list: the checked copy is the same kernel


def test_union_scan_and_compaction_second_turns(nt):
    h, c = many()
    n = COMPACT_STRIDE // 2 + 1
    lists, counts = [h[:n], h[n - 1000:2 * n - 1000]], [None, c[n - 1000:2 * n - 1000]]
    assert 2 * n == COMPACT_STRIDE + 2 and 2 * n <= h.size + 1000  # 513 tiles of sorted pairs
    want = model.union(lists, counts)
    assert want[0].size == 2 * n - 1000
    assert same(run_union(nt, lists, counts), want)


def test_hist_second_turn(nt):
    h, c = many()
    n = HIST_STRIDE + 1
    counts = c[:n].copy()
    counts[-1] = 4_000_000_000  # the one entry of the second turn
    want = model.hist(counts, 3)
    assert want[0][1] > n // 2 and want[0][4] > 1 and int(want[0].sum()) == n
    d = dev32(counts)
    got = nt.signature_hist_device(ptr(d), n, cov_max=3)
    assert np.array_equal(got[0], want[0]) and int(got[1]) == want[1]
