"""GPU tests of the set algebra and the spectrum of signatures (include/ntcard_hip.h: ntc_signature_union_device, ntc_signature_select_device,
ntc_signature_hist_device; ntcard_amd/csrc/ntc_sig_algebra.hip) against the numpy models of tests/sig_algebra_model.py — np.unique + np.add.at, np.isin,
np.bincount —, never against the code under test.  Hashes are drawn with a fixed seed from [0, 2^64), 0 and 2^64 - 1 among them.  The sizes above the grid
caps are tests/test_sig_algebra_scale_gpu.py's."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import sig_algebra_model as model
import sig_model
from gpu_support import nt, submit_slots  # noqa: F401
from support import ERR_ARG, ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = 2048             # the compaction tile: entries per workgroup and turn of the count and scatter kernels (kCompactTile)
HIST_LDS_BINS = 1024  # the counts below it are binned in LDS (kHistLdsBins)
SORT_ONE_LAUNCH = 4096  # sig_sort_one_launch(): up to here the union's sort is one launch
U32_MAX = 2**32 - 1
SENTINEL = 0x5A5A5A5A
MODES = ("all", "none", "any")


def library_constant(name):
    """a constexpr uint32_t of ntc_sig_algebra.hip, as the source states it"""
    with open(os.path.join(ROOT, "ntcard_amd", "csrc", "ntc_sig_algebra.hip")) as f:
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, f.read()).group(1))


def test_the_constants_here_are_the_librarys():
    assert library_constant("kCompactTile") == T and library_constant("kHistLdsBins") == HIST_LDS_BINS
    with open(os.path.join(ROOT, "ntcard_amd", "csrc", "ntc_sig_sort.hip")) as f:
        assert re.search(r"kSortTile = kSortWaves \* kSortWaveItems;\s+// 4096 pairs", f.read()) and SORT_ONE_LAUNCH == 4096


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda()


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def host(h, c, n):
    assert h.dtype == torch.int64 and c.dtype == torch.int32 and h.numel() == n and c.numel() == n
    return h.cpu().numpy().view(np.uint64), c.cpu().numpy().view(np.uint32)


def same(got, want):
    return (got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and np.array_equal(got[0], np.asarray(want[0], dtype=np.uint64)) and
            np.array_equal(got[1].astype(np.uint64), np.asarray(want[1]).astype(np.uint64)))


@functools.lru_cache(maxsize=None)
def pool():
    """40 000-odd distinct hashes of [0, 2^64), ascending, with 0 and 2^64 - 1"""
    rng = np.random.default_rng(71)
    p = np.unique(np.concatenate([rng.integers(0, 2**64, size=40_000, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)]))
    assert p[0] == 0 and p[-1] == 2**64 - 1 and p.size > 39_000
    p.setflags(write=False)
    return p


def sample(rng, n, of=None):
    """n of the pool's hashes (or of `of`), ascending"""
    src = pool() if of is None else of
    return np.sort(rng.choice(src, size=n, replace=False))


def run_select(nt, a, ca, refs, mode="all", lo=0, hi=0):
    da, dca = dev64(a), (dev32(ca) if ca is not None else None)
    drefs = [dev64(r) for r in refs]
    return host(*nt.signature_select_device(ptr(da), ptr(dca), a.size, [ptr(d) for d in drefs], [r.size for r in refs], mode=mode, min_count=lo, max_count=hi))


def run_union(nt, lists, counts=None):
    dl = [dev64(h) for h in lists]
    dc = None if counts is None else [dev32(c) if c is not None else None for c in counts]
    return host(*nt.signature_union_device([ptr(d) for d in dl], None if dc is None else [ptr(d) for d in dc], [h.size for h in lists]))


def table(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(p) if p else None for p in ptrs])


class Out:
    """sentinel-filled device outputs of `room` entries and *n_out"""

    def __init__(self, room):
        self.h, self.c = dev64(np.full(max(room, 1), SENTINEL)), dev32(np.full(max(room, 1), SENTINEL))
        self.n = C.c_uint64(SENTINEL)

    def untouched(self):
        return bool((self.h == SENTINEL).all()) and bool((self.c == SENTINEL).all()) and self.n.value == SENTINEL

    def pairs(self):
        n = self.n.value
        return self.h[:n].cpu().numpy().view(np.uint64), self.c[:n].cpu().numpy().view(np.uint32)


def raw_union(nt, lists, counts, out, cap, with_counts=True, query=False):
    dl = [dev64(h) for h in lists]
    dc = [dev32(c) if c is not None else None for c in counts] if counts is not None else None
    ns = (C.c_uint64 * len(lists))(*[h.size for h in lists])
    rc = nt._abi.lib().ntc_signature_union_device(0, None, len(lists), table([ptr(d) for d in dl]), table([ptr(d) for d in dc]) if dc is not None else None, ns,
                                                  None if query else C.c_void_p(out.h.data_ptr()), C.c_void_p(out.c.data_ptr()) if with_counts and not query else None,
                                                  cap, C.byref(out.n))
    return rc, nt._abi.lib().ntc_last_error()


def raw_select(nt, a, ca, refs, mode, out, cap, with_counts=True, query=False, lo=0, hi=0):
    da, dca = dev64(a), (dev32(ca) if ca is not None else None)
    drefs = [dev64(r) for r in refs]
    ns = (C.c_uint64 * max(len(refs), 1))(*[r.size for r in refs])
    rc = nt._abi.lib().ntc_signature_select_device(0, None, C.c_void_p(ptr(da)) if ptr(da) else None, C.c_void_p(ptr(dca)) if ptr(dca) else None, a.size, len(refs),
                                                   table([ptr(d) for d in drefs]) if refs else None, ns if refs else None, MODES.index(mode), lo, hi,
                                                   None if query else C.c_void_p(out.h.data_ptr()), C.c_void_p(out.c.data_ptr()) if with_counts and not query else None,
                                                   cap, C.byref(out.n))
    return rc, nt._abi.lib().ntc_last_error()


# ---- the compaction, through select without references: the count bounds 3 .. 7 are the flags ----
PATTERNS = {
    "all": lambda n, rng: np.ones(n, bool),
    "none": lambda n, rng: np.zeros(n, bool),
    "alternating": lambda n, rng: np.arange(n) % 2 == 1,
    "only_the_last": lambda n, rng: np.arange(n) == n - 1,
    "first_of_every_tile": lambda n, rng: np.arange(n) % T == 0,
    "random_half": lambda n, rng: rng.random(n) < 0.5,
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_compaction_keeps_the_flagged_entries_in_order(nt, pattern):
    rng = np.random.default_rng(72)
    for na in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        a = sample(rng, na, pool()[1:-1])
        a[:1], a[1:][-1:] = np.uint64(0), np.uint64(2**64 - 1)  # 0 first and, from two entries on, 2^64 - 1 last
        keep = PATTERNS[pattern](na, rng)
        ca = np.where(keep, rng.integers(3, 8, size=na), np.where(np.arange(na) % 3 == 0, U32_MAX, rng.integers(0, 3, size=na))).astype(np.uint32)
        ca[np.flatnonzero(~keep)[1::2]] = 8  # dropped on both sides of the bounds
        want = model.select(a, ca, [], "all", 3, 7)
        assert np.array_equal(want[0], a[keep]) and np.array_equal(want[1], ca[keep]), (pattern, na)
        for mode in ("all", "none"):  # (without references both keep what passes the count test)
            assert same(run_select(nt, a, ca, [], mode, 3, 7), want), (pattern, na, mode)


# ---- select ----
@functools.lru_cache(maxsize=None)
def select_case():
    """A: 5000 entries (three tiles, the last one partial) with counts; a pool of 9000 that holds it"""
    rng = np.random.default_rng(73)
    wide = sample(rng, 9000)
    a = np.sort(np.concatenate([rng.choice(wide[1:-1], size=4998, replace=False), wide[:1], wide[-1:]]))
    ca = rng.integers(1, 50, size=a.size).astype(np.uint32)
    for x in (wide, a, ca):
        x.setflags(write=False)
    assert a.size == 5000 and 2 * T < a.size < 3 * T
    return wide, a, ca


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_refs", [1, 2, 3])
def test_select_against_a_few_references(nt, mode, n_refs):
    wide, a, ca = select_case()
    rng = np.random.default_rng(74 + n_refs)
    refs = [sample(rng, int(s), wide) for s in (6000, 300, 8000)[:n_refs]]
    want = model.select(a, ca, refs, mode)
    assert 0 < want[0].size < a.size
    assert same(run_select(nt, a, ca, refs, mode), want)
    assert same(run_select(nt, a, ca, refs, mode, 10, 30), model.select(a, ca, refs, mode, 10, 30))


@pytest.mark.parametrize("mode", MODES)
def test_select_against_1024_references(nt, mode):
    wide, a, ca = select_case()
    rng = np.random.default_rng(78)
    shared = a[[0, 2500, 4999]]  # what every reference holds: A's first and last entry among them
    refs = [np.unique(np.concatenate([shared, rng.choice(wide, size=4)])) for _ in range(1024)]
    want = model.select(a, ca, refs, mode)
    assert want[0].size == {"all": 3}.get(mode, want[0].size) and 3 < model.select(a, ca, refs, "any")[0].size < a.size
    assert same(run_select(nt, a, ca, refs, mode), want)


@pytest.mark.parametrize("mode", MODES)
def test_select_identical_disjoint_and_outlying_references(nt, mode):
    wide, a, ca = select_case()
    inner, ca = a[20:-20], ca[19:-19]  # (room for hashes outside A below and above; ca[1:-1] below are inner's counts)
    others = np.setdiff1d(wide, a)
    below, above = others[others < inner[0]], others[others > inner[-1]]
    assert below.size and above.size and others.size > 3000
    everything = (inner, ca[1:-1])
    nothing = (inner[:0], ca[:0])
    for refs, kept in (([inner.copy()], "all"), ([others], "none"), ([below], "none"), ([above], "none"), ([below, above], "none"), ([inner.copy(), inner.copy()], "all")):
        want = model.select(inner, ca[1:-1], refs, mode)
        assert same(want, everything if (mode == "none") == (kept == "none") else nothing), (mode, kept)
        assert same(run_select(nt, inner, ca[1:-1], refs, mode), want), (mode, kept)


@pytest.mark.parametrize("mode", MODES)
def test_select_with_an_empty_reference_and_with_none(nt, mode):
    wide, a, ca = select_case()
    empty = a[:0]
    for refs in ([empty], [a[::2], empty], [empty, a[::2]], []):  # (an empty reference goes in as a NULL pointer)
        want = model.select(a, ca, refs, mode)
        assert same(run_select(nt, a, ca, refs, mode), want), (mode, len(refs))
    assert model.select(a, ca, [empty], mode)[0].size == (a.size if mode == "none" else 0)
    assert model.select(a, ca, [], mode)[0].size == (0 if mode == "any" else a.size)
    assert model.select(a, ca, [a[::2], empty], mode)[0].size == {"all": 0, "none": a.size // 2, "any": a.size // 2}[mode]
    assert same(run_select(nt, empty, None, [a], mode), (empty, ca[:0]))  # an empty A


def test_select_count_bounds_without_counts(nt):
    wide, a, ca = select_case()
    ones = np.ones(a.size, np.uint32)
    assert same(run_select(nt, a, None, [], "all", 1, 1), (a, ones)) and same(run_select(nt, a, None, [], "all", 0, 0), (a, ones))
    assert same(run_select(nt, a, None, [], "all", 1, 0), (a, ones)) and same(run_select(nt, a, None, [], "all", 0, U32_MAX), (a, ones))
    assert same(run_select(nt, a, None, [], "all", 2, 0), (a[:0], ones[:0])) and same(run_select(nt, a, None, [a], "all", 2, 0), (a[:0], ones[:0]))
    assert same(run_select(nt, a, None, [a[::3]], "all", 1, 1), (a[::3], ones[::3]))
    # with counts both bounds are inclusive
    lo, hi = 7, 23
    want = model.select(a, ca, [], "all", lo, hi)
    assert (want[1] == lo).any() and (want[1] == hi).any() and (ca == lo - 1).any() and (ca == hi + 1).any()
    assert same(run_select(nt, a, ca, [], "all", lo, hi), want)
    assert same(run_select(nt, a, ca, [], "all", hi, hi), model.select(a, ca, [], "all", hi, hi))


def test_select_output_protocol(nt):
    wide, a, ca = select_case()
    refs = [a[::2]]
    want = model.select(a, ca, refs, "all")
    size = want[0].size
    out = Out(a.size)
    rc, _ = raw_select(nt, a, ca, refs, "all", out, 0, query=True)  # the size alone
    assert rc == 0 and out.n.value == size and bool((out.h == SENTINEL).all()) and bool((out.c == SENTINEL).all())
    out = Out(a.size)
    rc, msg = raw_select(nt, a, ca, refs, "all", out, size - 1)  # one short
    assert rc == ERR_ARG and out.untouched() and (b"%d entries" % size) in msg, msg
    out = Out(a.size)
    rc, _ = raw_select(nt, a, ca, refs, "all", out, size)  # exact
    assert rc == 0 and same(out.pairs(), want) and bool((out.h[size:] == SENTINEL).all()) and bool((out.c[size:] == SENTINEL).all())
    out = Out(a.size)
    rc, _ = raw_select(nt, a, ca, refs, "all", out, a.size, with_counts=False)  # hashes only
    assert rc == 0 and np.array_equal(out.pairs()[0], want[0]) and bool((out.c == SENTINEL).all())


# ---- union ----
@pytest.mark.parametrize("n_lists", [1, 2, 3, 1024])
def test_union_of_lists_with_and_without_counts(nt, n_lists):
    rng = np.random.default_rng(80 + n_lists)
    size = 3000 if n_lists <= 3 else 12
    lists = [sample(rng, size + i % 5) for i in range(n_lists)]
    lists[0] = np.unique(np.concatenate([lists[0], pool()[:1], pool()[-1:]]))
    counts = [None if i % 3 == 1 else rng.integers(1, 1000, size=h.size).astype(np.uint32) for i, h in enumerate(lists)]
    want = model.union(lists, counts)
    total = sum(h.size for h in lists)
    assert want[0][0] == 0 and want[0][-1] == 2**64 - 1 and (n_lists == 1 or (want[0].size < total and total > SORT_ONE_LAUNCH))
    assert same(run_union(nt, lists, counts), want)
    assert same(run_union(nt, lists, None), model.union(lists, None))
    assert same(run_union(nt, lists, [None] * n_lists), model.union(lists, None))


@pytest.mark.parametrize("total", [SORT_ONE_LAUNCH, SORT_ONE_LAUNCH + 1])
def test_union_at_the_one_launch_sort_and_one_above(nt, total):
    rng = np.random.default_rng(85)
    lists = [sample(rng, 2000), sample(rng, 1500), sample(rng, total - 3500)]
    counts = [rng.integers(1, 9, size=h.size).astype(np.uint32) for h in lists]
    assert sum(h.size for h in lists) == total
    want = model.union(lists, counts)
    assert want[0].size < total  # some hashes are shared
    assert same(run_union(nt, lists, counts), want)


def test_union_identical_disjoint_and_empty_lists(nt):
    rng = np.random.default_rng(86)
    h = sample(rng, 5000)
    c = rng.integers(1, 100, size=h.size).astype(np.uint32)
    assert same(run_union(nt, [h, h.copy(), h.copy()], [c, c, None]), (h, 2 * c.astype(np.uint64) + 1))
    parts = [h[0::3], h[1::3], h[2::3]]  # disjoint: the union is their interleaving
    assert same(run_union(nt, parts, [c[0::3], c[1::3], c[2::3]]), (h, c))
    empty = h[:0]
    assert same(run_union(nt, [empty, empty, empty], None), (empty, c[:0])) and same(run_union(nt, [empty], None), (empty, c[:0]))
    assert same(run_union(nt, [empty, h, empty], [None, c, None]), (h, c)) and same(run_union(nt, [h], [c]), (h, c))
    assert same(run_union(nt, [h], None), (h, np.ones(h.size, np.uint32)))


def test_union_run_of_1024_across_a_tile_boundary(nt):
    """one hash held by all 1024 lists; list 0 holds `below` smaller ones, so the run's head is entry `below` of the sorted pairs and its run reaches into the
    next tile of the run-head pass"""
    rng = np.random.default_rng(87)
    below = T - 500
    p = pool()
    shared = p[30_000]
    lists = [np.concatenate([sample(rng, below, p[1:30_000]), [shared]])] + [np.array([shared], dtype=np.uint64) for _ in range(1023)]
    lists[1023] = np.array([shared, p[-1]], dtype=np.uint64)
    counts = [None if i % 2 else np.full(h.size, 3, np.uint32) for i, h in enumerate(lists)]
    assert below < T < below + 1024 and sum(h.size for h in lists) == below + 1024 + 1
    want = model.union(lists, counts)
    assert want[0].size == below + 2 and want[0][below] == shared and want[1][below] == 512 * 3 + 512
    assert same(run_union(nt, lists, counts), want)


def test_union_saturates_at_u32_max(nt):
    u64, u32 = (lambda *v: np.array(v, dtype=np.uint64)), (lambda *v: np.array(v, dtype=np.uint32))
    h = u64(5, 7, 9)
    assert same(run_union(nt, [h, h], [u32(U32_MAX, 1, 2), None]), (h, u32(U32_MAX, 2, 3)))                       # (2^32 - 1) + 1
    assert same(run_union(nt, [h, h, h], [u32(2**31, 1, 1)] * 3), (h, u32(U32_MAX, 3, 3)))                        # 3 x 2^31
    assert same(run_union(nt, [h, h], [u32(2**31, 1, 1)] * 2), (h, u32(U32_MAX, 2, 2)))                           # 2^32: one above
    assert same(run_union(nt, [h, h, u64(7)], [u32(2**31, 2**31, 1), u32(2**31 - 1, 2**31 - 2, 1), u32(1)]), (h, u32(U32_MAX, U32_MAX, 2)))  # exactly 2^32 - 1
    assert same(run_union(nt, [h, h, h], [u32(U32_MAX, U32_MAX, 0)] * 3), (h, u32(U32_MAX, U32_MAX, 0)))


def test_union_output_protocol(nt):
    rng = np.random.default_rng(88)
    lists = [sample(rng, 3000), sample(rng, 2500)]
    counts = [rng.integers(1, 9, size=3000).astype(np.uint32), None]
    want = model.union(lists, counts)
    size = want[0].size
    assert size < 5500
    out = Out(5500)
    rc, _ = raw_union(nt, lists, counts, out, 0, query=True)
    assert rc == 0 and out.n.value == size and bool((out.h == SENTINEL).all()) and bool((out.c == SENTINEL).all())
    out = Out(5500)
    rc, msg = raw_union(nt, lists, counts, out, size - 1)
    assert rc == ERR_ARG and out.untouched() and (b"%d entries" % size) in msg, msg
    out = Out(5500)
    rc, _ = raw_union(nt, lists, counts, out, size)
    assert rc == 0 and same(out.pairs(), want) and bool((out.h[size:] == SENTINEL).all()) and bool((out.c[size:] == SENTINEL).all())
    out = Out(5500)
    rc, _ = raw_union(nt, lists, counts, out, 5500, with_counts=False)
    assert rc == 0 and np.array_equal(out.pairs()[0], want[0]) and bool((out.c == SENTINEL).all())
    # one list: the checked copy follows the same protocol
    out = Out(3000)
    rc, msg = raw_union(nt, lists[:1], counts[:1], out, 2999)
    assert rc == ERR_ARG and out.untouched() and b"3000 entries" in msg
    rc, _ = raw_union(nt, lists[:1], counts[:1], out, 0, query=True)
    assert rc == 0 and out.n.value == 3000 and bool((out.h == SENTINEL).all())


def broken(h, at, how):
    """h with entry `at` repeated (h[at] = h[at - 1]) or out of order (swapped with its predecessor): the first bad entry is `at`"""
    b = h.copy()
    if how == "repeated":
        b[at] = b[at - 1]
    else:
        b[at - 1], b[at] = h[at], h[at - 1]
    return b


@pytest.mark.parametrize("how", ["repeated", "unsorted"])
def test_inputs_that_do_not_ascend_are_named(nt, how):
    rng = np.random.default_rng(89)
    good = [sample(rng, 3000), sample(rng, 10), sample(rng, 2600)]
    for which, at in ((0, 1777), (2, 2599)):
        lists = list(good)
        lists[which] = broken(good[which], at, how)
        out = Out(6000)
        rc, msg = raw_union(nt, lists, None, out, 6000)
        assert rc == ERR_ARG and out.untouched() and (b"list %d is not strictly ascending at entry %d" % (which, at)) in msg, msg
        rc, msg = raw_union(nt, lists, None, out, 0, query=True)
        assert rc == ERR_ARG and out.untouched()
    out = Out(3000)
    rc, msg = raw_union(nt, [broken(good[0], 1, how)], None, out, 3000)  # one list: the copy is a checked one
    assert rc == ERR_ARG and out.untouched() and b"list 0 is not strictly ascending at entry 1" in msg, msg
    for mode in MODES:
        out = Out(3000)
        rc, msg = raw_select(nt, good[0], None, [good[1], broken(good[2], 5, how)], mode, out, 3000)
        assert rc == ERR_ARG and out.untouched() and b"reference 1 is not strictly ascending at entry 5" in msg, msg
        rc, msg = raw_select(nt, broken(good[0], 2999, how), None, [good[1]], mode, out, 3000)
        assert rc == ERR_ARG and out.untouched() and b"A is not strictly ascending at entry 2999" in msg, msg


# ---- hist ----
def run_hist(nt, counts, cov_max):
    d = dev32(counts)
    h, w = nt.signature_hist_device(ptr(d), counts.size, cov_max=cov_max)
    assert h.dtype == np.uint64 and h.size == cov_max + 2
    return h, int(w)


@pytest.mark.parametrize("cov_max", [1, 1000, 65535])
def test_hist_against_bincount(nt, cov_max):
    rng = np.random.default_rng(90)
    edge = np.array([0, 1, cov_max, cov_max + 1, U32_MAX, HIST_LDS_BINS - 1, HIST_LDS_BINS, HIST_LDS_BINS + 1, 65535, 65536], dtype=np.uint32)
    counts = np.concatenate([edge, edge[:5], rng.integers(0, 70_000, size=3000).astype(np.uint32), rng.integers(0, 4, size=3000).astype(np.uint32)])
    want = model.hist(counts, cov_max)
    assert want[0][cov_max + 1] >= 2 and want[0][0] >= 2 and want[1] == int(counts.astype(np.uint64).sum()) > 2 * U32_MAX
    got = run_hist(nt, counts, cov_max)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    for v in edge.tolist():  # each edge value alone
        one = np.array([v], dtype=np.uint32)
        got, want = run_hist(nt, one, cov_max), model.hist(one, cov_max)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] == v and int(got[0][min(v, cov_max + 1)]) == 1, v


def test_hist_of_nothing_and_of_ones(nt):
    h, w = run_hist(nt, np.zeros(0, np.uint32), 1000)
    assert not h.any() and w == 0
    h, w = run_hist(nt, np.ones(100_000, np.uint32), 1000)
    assert int(h[1]) == 100_000 and int(h.sum()) == 100_000 and w == 100_000


def test_hist_on_either_side_of_the_last_lds_bin(nt):
    counts = np.repeat(np.array([HIST_LDS_BINS - 1, HIST_LDS_BINS], dtype=np.uint32), [777, 333])
    for cov_max in (HIST_LDS_BINS - 2, HIST_LDS_BINS - 1, HIST_LDS_BINS, 2000):
        got, want = run_hist(nt, counts, cov_max), model.hist(counts, cov_max)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    h = run_hist(nt, counts, 2000)[0]
    assert int(h[HIST_LDS_BINS - 1]) == 777 and int(h[HIST_LDS_BINS]) == 333


# ---- end to end on counted reads ----
def test_union_select_and_hist_of_counted_reads(nt):
    reads = sig_model.equal_reads()
    half = len(reads) // 2
    want = sig_model.equal_model(32, "canonical", 7)
    first = sig_model.model(reads[:half], 32, "canonical", 7)
    assert want[0].size == 593 and 0 < first[0].size < 593

    def on_device(e):
        h, c, n = e.signature_device()
        return h.clone(), c.clone(), n

    with nt.Engine([32], r_bits=14, s_bits=7, signature=True) as e1, nt.Engine([32], r_bits=14, s_bits=7, signature=True) as e2, \
            nt.Engine([32], r_bits=14, s_bits=7, signature=True) as whole:
        submit_slots(e1, reads[:half])
        submit_slots(e2, reads[half:])
        submit_slots(whole, reads)
        h1, c1, n1 = on_device(e1)
        h2, c2, n2 = on_device(e2)
        hw, cw, nw = on_device(whole)
    assert same(host(hw, cw, nw), want) and same(host(h1, c1, n1), first)
    uh, uc, un = nt.signature_union_device([h1.data_ptr(), h2.data_ptr()], [c1.data_ptr(), c2.data_ptr()], [n1, n2])
    assert un == 593 and same(host(uh, uc, un), want) and same(host(uh, uc, un), host(hw, cw, nw))
    hist, weight = nt.signature_hist_device(uc.data_ptr(), un, cov_max=1000)
    total = int(np.asarray(want[1]).astype(np.uint64).sum())
    assert int(weight) == total and int((np.arange(1002, dtype=np.uint64) * hist).sum()) == total and int(hist[1001]) == 0 and int(hist.sum()) == 593
    in_first = np.isin(want[0], first[0])
    sh, sc, sn = nt.signature_select_device(uh.data_ptr(), uc.data_ptr(), un, [h1.data_ptr()], [n1], mode="all")
    assert same(host(sh, sc, sn), (first[0], np.asarray(want[1])[in_first])) and np.array_equal(want[0][in_first], first[0])
    sh, sc, sn = nt.signature_select_device(uh.data_ptr(), uc.data_ptr(), un, [h1.data_ptr()], [n1], mode="none")
    assert same(host(sh, sc, sn), (want[0][~in_first], np.asarray(want[1])[~in_first])) and sn == 593 - n1
