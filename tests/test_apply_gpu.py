"""The sketch update (ntc_apply.hip: split_kernel / split_packed_kernel -> count_kernel, the direct-atomic fall-backs, log_atomics_kernel) on CHOSEN key sets.

Every other GPU test reaches the update through a hash kernel, so the keys it sees are ntHash output: uniform, or a few hot counters.  Here
`ntc_log_replace_device` makes an array of counter indices the pending log and the engine's own update counts exactly those; the reference is
`np.unique(keys, return_counts=True)` — exact, no hashing.  The key sets are built from the geometry (which digit, slice and word slot a key falls in)
and never from what a kernel returned; every expected value is numpy's count of the injected keys.

`Geo` restates `plan_log` (ntc_plan.hip) for ONE purpose: to aim the key sets (which bits are a pass's digit, how many keys overflow a run).  No
assertion on a kernel's output depends on it — a wrong restatement could only make a key set miss the branch it aims at, never make a wrong sketch pass.
What of it can be seen from outside is checked: the log takes `room` keys and refuses `room + 1` (test_refusals).
"""
import numpy as np
import pytest

import orc
from devview import DevArray
from gpu_support import nt  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

J_SPARSE = (1, 2, 3, 4, 7)
HOT_N = (1, 65534, 65535, 65536, 65537, 3 * 65535 + 1)


def _ceil_log2(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


class Geo:
    """where a key of this engine goes: key = [b1 | b2 | slice_bits] (plan_log), and how much a run holds"""

    def __init__(self, klist, r_bits, log_entries):
        assert log_entries >= 1 << 14 and log_entries & (log_entries - 1) == 0
        self.klist, self.r_bits, self.log_entries = list(klist), r_bits, log_entries
        self.counters = len(klist) * (2 << r_bits)
        self.key_bits = _ceil_log2(self.counters)
        self.slice_bits = min(15, self.key_bits)
        pb = self.key_bits - self.slice_bits
        self.b1 = pb if pb <= 8 else (pb + 1) // 2
        self.b2 = pb - self.b1
        self.n_slices = (self.counters + (1 << self.slice_bits) - 1) >> self.slice_bits
        self.region_cap = min(32768, max(256, log_entries // 8192))
        self.regions = log_entries // self.region_cap
        self.all_regions = self.regions + max(1, min(1024, self.regions // 8))
        self.room = self.all_regions * self.region_cap  # what ntc_log_replace_device takes: log_entries fit, 2 * log_entries do not
        self.g1 = min(self.regions, 256)
        self.share1 = (self.all_regions + self.g1 - 1) // self.g1 * self.region_cap  # the most keys one pass-1 workgroup reads
        self.cap1 = ((self.share1 >> self.b1) * 5 // 4 + 64 + 7) & ~7
        self.packed = self.b2 != 0 and self.key_bits - self.b1 <= 21
        self.cap1_keys = 3 * (self.cap1 // 2) if self.packed else self.cap1  # a packed run: cap1 / 2 words of three keys
        share2 = ((self.room >> self.b1) * 5 // 4) // 4 + 1
        self.cap2 = ((share2 >> self.b2) * 13 // 10 + 64 + 7) & ~7
        self.low_bits = self.key_bits - self.b1  # what pass 1 leaves of a key
        self.n_digits1 = (self.counters + (1 << self.low_bits) - 1) >> self.low_bits  # pass-1 digits that hold counters

    def shape(self):
        return (self.key_bits, self.b1, self.b2, self.packed)

    def slice_width(self, s):
        return min(1 << self.slice_bits, self.counters - (s << self.slice_bits))

    def valid(self, keys):
        """reject what lies beyond the sketch (a counter space that is not a power of two leaves the top of the key space unbacked)"""
        keys = np.asarray(keys, dtype=np.uint64)
        return keys[keys < self.counters].astype(np.uint32)


# (klist, r_bits, log_entries, (key_bits, b1, b2, packed between the passes)) — the class is what plan_log derives; test_geometry_classes holds Geo to it
GEOMETRIES = [
    pytest.param([32], 8, 1 << 14, (9, 0, 0, False), id="r8-no-partition-slice9"),            # no partition, slice_bits = 9 < 15: count_kernel on the raw log, 512 threads
    pytest.param([32], 14, 1 << 16, (15, 0, 0, False), id="r14-no-partition-slice15"),        # no partition, one slice of 2^15
    pytest.param([32], 15, 1 << 18, (16, 1, 0, False), id="r15-one-pass-1bit"),               # one pass of 1 bit, uint16 runs
    pytest.param([32], 22, 1 << 18, (23, 8, 0, False), id="r22-one-pass-8bit"),               # one pass of 8 bits
    pytest.param([20, 24, 32], 13, 1 << 16, (16, 1, 0, False), id="3k-r13-one-pass"),         # 3 x 2^14 counters: the second slice is half backed
    pytest.param([16, 20, 24, 28, 32], 16, 1 << 18, (20, 5, 0, False), id="5k-r16-one-pass"),  # 5 x 2^17 counters: 20 of 32 digits
    pytest.param([14, 16, 20, 24, 28, 30, 32], 16, 1 << 16, (20, 5, 0, False), id="7k-r16-one-pass"),  # 7 x 2^17 counters: 28 of 32 digits
    pytest.param([32], 23, 1 << 18, (24, 5, 4, True), id="r23-two-packed-5+4"),               # two passes, 19 bits left: packed words
    pytest.param([20, 24, 32], 22, 1 << 18, (25, 5, 5, True), id="3k-r22-two-packed-5+5"),    # packed, 3 x 2^23 counters: 24 of 32 digits
    pytest.param([32], 27, 1 << 20, (28, 7, 6, True), id="r27-two-packed-7+6"),               # the headline configuration: exactly 21 bits left
    pytest.param([32], 28, 1 << 18, (29, 7, 7, False), id="r28-two-unpacked-7+7"),            # 22 bits left: uint32 runs between the passes
    pytest.param([24, 32], 27, 1 << 16, (29, 7, 7, False), id="2k-r27-two-unpacked-7+7"),
    pytest.param([32], 30, 1 << 20, (31, 8, 8, False), id="r30-two-unpacked-8+8"),            # 2^31 counters, 65536 slices
]
TWO_PASS = [p for p in GEOMETRIES if p.values[3][2] != 0]


def _modes(nt):
    """partition passes for every log, and the engine's own choice (logs this small: log_atomics_kernel)"""
    return (nt.FLAG_ALWAYS_LOG | nt.FLAG_PARTITION_ALWAYS, 0)


class Sketch:
    """one engine, the keys injected into it since its last reset, and the check of its counters against numpy's count of them"""

    def __init__(self, nt, geo, flags):
        self.nt, self.geo = nt, geo
        self.e = nt.Engine(geo.klist, r_bits=geo.r_bits, s_bits=7, flags=flags, log_entries=geo.log_entries)
        self.keys, self.extra, self._keep = [], {}, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.e.close()

    def inject(self, keys):
        """keys -> the pending log (no apply)"""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        assert keys.ndim == 1 and keys.size <= self.geo.room
        assert keys.size == 0 or int(keys.max()) < self.geo.counters, "a key beyond the sketch would be written out of bounds"
        if keys.size:
            d = torch.from_numpy(keys.view(np.int32)).cuda()
            self._keep.append(d)
            self.e.log_replace(d.data_ptr(), keys.size)
        else:
            self.e.log_replace(None, 0)
        return keys

    def apply(self, keys):
        self.keys.append(self.inject(keys))
        self.e.flush()

    def reset(self):
        self.e.reset()
        self.keys, self.extra = [], {}

    def view(self):
        sk, ncnt, f1 = self.e.device_state()
        torch.cuda.synchronize()
        assert ncnt == self.geo.counters
        return torch.as_tensor(DevArray(sk, ncnt), device="cuda"), torch.as_tensor(DevArray(f1, 2 * len(self.geo.klist)), device="cuda")

    def check(self, what=""):
        """got[u] == c for the distinct keys u, and the sum of all counters == the number of keys: counters are non-negative, so every other one is zero"""
        got, f1 = self.view()
        allk = np.concatenate(self.keys + [np.repeat(np.uint32(k), n) for k, n in self.extra.items()] + [np.zeros(0, np.uint32)])
        u, c = np.unique(allk, return_counts=True)
        have = got[torch.from_numpy(u.astype(np.int64)).cuda()].cpu().numpy().astype(np.int64)
        bad = np.flatnonzero(have != c)
        assert bad.size == 0, (what, "counters differ", bad.size, [(int(u[i]), int(have[i]), int(c[i])) for i in bad[:8]])
        total = int(got.sum(dtype=torch.int64))
        assert total == allk.size, (what, "counts outside the injected keys", total, allk.size)
        assert not bool(f1.any()), (what, "F1 touched")
        self._keep.clear()
        if self.geo.counters <= 1 << 22:  # the uint16 view the rest of the suite uses
            tc, ph, hf1 = self.e.finish(counters=True)
            want = (np.bincount(allk, minlength=self.geo.counters) & 0xffff).astype(np.uint16).reshape(tc.shape)
            assert np.array_equal(tc, want), what
            for ki in range(len(self.geo.klist)):
                assert np.array_equal(ph[ki], orc.value_hist(want[ki], self.geo.r_bits)), (what, ki)
            assert not hf1.any(), what


# -- key sets (all from the geometry and a seeded generator) -------------------------------------------------------------------------------------------
def uniform(geo, rng, n):
    return rng.integers(0, geo.counters, size=n, dtype=np.uint64).astype(np.uint32)


def in_slice(geo, rng, s, n):
    """n keys of slice s, low bits random (folded into what of the slice is backed by counters)"""
    assert 0 <= s < geo.n_slices
    return ((s << geo.slice_bits) + rng.integers(0, geo.slice_width(s), size=n, dtype=np.uint64)).astype(np.uint32)


def slices_of_interest(geo):
    return sorted({0, geo.n_slices // 2, geo.n_slices - 1})


def hot_targets(geo):
    """counter 0, the last valid counter, and an even and an odd counter on each side of a slice boundary — no two of them (or of their pairs key ^ 1) in
    one LDS dword"""
    b = (geo.n_slices // 2) << geo.slice_bits if geo.n_slices > 1 else geo.counters // 2  # (a single slice: its middle)
    t = [0, geo.counters - 1, b - 4, b - 1, b, b + 3]
    assert len({k >> 1 for k in t}) == len(t) and all(0 <= k < geo.counters and (k ^ 1) < geo.counters for k in t)
    return t


def hot_round(geo, rot):
    """target i is hit HOT_N[(i + rot) % 6] times and its pair key ^ 1 once; the hits of a target lie together, so whole waves hold one key"""
    parts = []
    for i, k in enumerate(hot_targets(geo)):
        parts.append(np.full(HOT_N[(i + rot) % len(HOT_N)], k, dtype=np.uint32))
        parts.append(np.array([k ^ 1], dtype=np.uint32))
    return np.concatenate(parts)


def sparse_slices(geo, rng, j):
    """every slice gets exactly j keys (as many slices as the log holds), in random order: a region — one round of a partition workgroup — then gives most
    digits 0 .. 4 keys: packed words of one, two and three keys and their padding"""
    ns = min(geo.n_slices, geo.log_entries // j)
    first = geo.n_slices - ns  # (the last slices: the last one may be partly backed)
    s = np.repeat(np.arange(first, first + ns, dtype=np.uint64), j)
    width = np.where(s == geo.n_slices - 1, geo.slice_width(geo.n_slices - 1), 1 << geo.slice_bits).astype(np.uint64)
    keys = ((s << np.uint64(geo.slice_bits)) + rng.integers(0, 1 << 62, size=s.size, dtype=np.uint64) % width).astype(np.uint32)
    return keys[rng.permutation(keys.size)]


def digit_groups(geo, j):
    """one region (one round of a pass-1 workgroup): as many pass-1 digits as fit get exactly j keys each, the rest of the region goes to the digits in
    turn one key at a time — digits of exactly j and j + 1 keys in a round"""
    m = min(geo.n_digits1, geo.region_cap // j)
    d = np.concatenate([np.repeat(np.arange(m, dtype=np.uint64), j), np.arange(geo.region_cap - m * j, dtype=np.uint64) % np.uint64(m)])
    assert d.size == geo.region_cap
    low = (np.arange(d.size, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << geo.low_bits) - 1)
    return geo.valid((d << np.uint64(geo.low_bits)) | low)


def slot_patterns(geo):
    """keys whose bits below the pass-1 digit are all ones, all zeros and 0x155555, in groups of one, two and three per digit and rotated, so that each lands
    in each slot of a packed word (the third slot ends at bit 62, next to the flag)"""
    mask = (1 << geo.low_bits) - 1
    pats = [mask, 0, 0x155555 & mask]
    keys = []
    for rep in range(9):
        for d in range(geo.n_digits1):
            ln, rot = 1 + (d + rep) % 3, (d // 3 + rep) % 3
            keys += [(d << geo.low_bits) | pats[(rot + q) % 3] for q in range(ln)]
    return geo.valid(keys)[: geo.room]


def skewed(geo, rng, n):
    hot = rng.integers(0, geo.counters, size=16, dtype=np.uint64)
    keys = np.concatenate([hot[rng.integers(0, 16, size=n // 2)], rng.integers(0, geo.counters, size=n - n // 2, dtype=np.uint64)]).astype(np.uint32)
    return keys[rng.permutation(n)]


# -- tests ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_geometry_classes(klist, r_bits, log_entries, shape):
    """the cases are the classes they are named for (key_bits, pass-1 bits, pass-2 bits, packed words between the passes)"""
    geo = Geo(klist, r_bits, log_entries)
    assert geo.shape() == shape
    assert geo.log_entries <= geo.room < 2 * geo.log_entries


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_uniform_sorted_and_skewed_keys(nt, klist, r_bits, log_entries, shape):
    """key sets 1, 7, 9 and the state rules: a new engine's first apply writes into the zeroed sketch, the second adds; after reset() an apply counts alone.
    The counters are read (ntc_device_state) only AFTER the applies under test: an engine that has handed the address out never writes"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits * 100 + len(klist))
    n = geo.log_entries  # a log filled to the last entry of its regions
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            s.apply(uniform(geo, rng, n))                    # apply 1: writes
            s.apply(np.sort(uniform(geo, rng, n)))           # apply 2: adds; sorted ascending: every region, so every round of a workgroup, holds one digit
            s.check(("1+2", flags))
            s.reset()
            s.apply(np.sort(uniform(geo, rng, n))[::-1])     # apply 3, behind a reset: counts of this apply alone
            s.check(("3", flags))
            s.apply(skewed(geo, rng, n))                     # half the keys on 16 hot counters
            s.check(("3+skew", flags))
        with Sketch(nt, geo, flags) as s:                    # behind a reset WITHOUT the address handed out: the apply writes again
            s.apply(skewed(geo, rng, n))
            s.reset()
            s.apply(uniform(geo, rng, geo.room))             # every region full, the fix-up kernel's own regions behind the hash kernels' too
            s.check(("room", flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_one_counter_hit_around_65535_times(nt, klist, r_bits, log_entries, shape):
    """key set 2: a counter hit 1, 65534, 65535, 65536, 65537 and 3 x 65535 + 1 times while its pair in the same LDS dword (key ^ 1) is hit once — count_kernel
    takes at most 65535 keys per pass so that no 16-bit field carries into its neighbour, and a wave of equal keys adds popcount << 16 at once.  Six applies
    rotate the six counts over the six targets.  (A log of 2^19 entries for every geometry: a round has 458 755 keys.  With the shallow geometries
    — no partition, 1 bit — all hits of a target reach count_kernel; the deeper the partition, the more of them overflow their runs and are added by the
    fall-back atomics: the sum must be exact either way.)"""
    geo = Geo(klist, r_bits, 1 << 19)
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            for rot in range(len(HOT_N)):
                s.apply(hot_round(geo, rot))
            s.check(("hot", flags))
        with Sketch(nt, geo, flags) as s:  # the first apply alone (it writes: a slice's second pass must add to its first)
            s.apply(hot_round(geo, 3))
            s.check(("hot first", flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_all_keys_in_one_slice_overflow_the_runs(nt, klist, r_bits, log_entries, shape):
    """key set 3, and the device-side dirty word: all keys in the first, a middle and the last valid slice, as the FIRST apply of a new engine.  With every
    region full (`room` keys) a pass-1 workgroup reads up to share1 keys and all of them have one digit, so its run of cap1_keys overflows as soon as
    share1 > cap1_keys — cap1 is (share1 >> b1) * 5 / 4 + 64: true for every partitioned geometry here (asserted).  What pass 1 kept, g1 / 4 runs per pass-2
    workgroup, again has one digit and overflows cap2 (asserted).  The overflow is added with atomics BEFORE the count pass: that pass must then add, not
    write; and the packed second pass rebuilds the counter index from 21 bits | hi."""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 7)
    if geo.b1:
        assert geo.share1 > geo.cap1_keys
    if geo.b2:
        assert (geo.g1 // 4) * min(geo.cap1_keys, geo.region_cap) > geo.cap2
    for flags in _modes(nt):
        for sl in slices_of_interest(geo):
            with Sketch(nt, geo, flags) as s:
                s.apply(in_slice(geo, rng, sl, geo.room))
                s.apply(uniform(geo, rng, 5000))
                s.check(("slice", sl, flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", TWO_PASS)
def test_one_digit_of_one_pass_all_digits_of_the_other(nt, klist, r_bits, log_entries, shape):
    """key set 4: all keys in one pass-1 digit (the first, a middle, the last valid one) and spread evenly over the pass-2 digits — pass 1 overflows, pass 2
    does not —, and the reverse: pass 1 keeps everything, every pass-2 workgroup gets one digit and overflows (room / digits keys per pass-1 digit, a quarter
    per workgroup, against cap2: asserted)"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 11)
    nd1 = geo.n_digits1
    i = np.arange(geo.room, dtype=np.uint64)
    low = rng.integers(0, 1 << geo.slice_bits, size=geo.room, dtype=np.uint64)
    assert (geo.room // nd1) // 4 > geo.cap2
    for flags in _modes(nt):
        for d1 in sorted({0, nd1 // 2, nd1 - 1}):
            with Sketch(nt, geo, flags) as s:
                s.apply(geo.valid((np.uint64(d1) << np.uint64(geo.low_bits)) | ((i % np.uint64(1 << geo.b2)) << np.uint64(geo.slice_bits)) | low))
                s.check(("one pass-1 digit", d1, flags))
        for d2 in sorted({0, (1 << geo.b2) - 1}):
            with Sketch(nt, geo, flags) as s:
                s.apply(geo.valid(((i % np.uint64(nd1)) << np.uint64(geo.low_bits)) | (np.uint64(d2) << np.uint64(geo.slice_bits)) | low))
                s.check(("one pass-2 digit", d2, flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_sparse_digits_and_word_slots(nt, klist, r_bits, log_entries, shape):
    """key sets 5 and 6: every slice gets exactly j keys, and every pass-1 digit exactly j (or j + 1) keys in a round, j = 1, 2, 3, 4, 7 — the packed word's
    "fewer than three" flag at bit 63, its "one, not two" flag at bit 42 and the padding to whole words; leftover bits all ones / all zeros / 0x155555 in
    each of the three slots"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 13)
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            for j in J_SPARSE:
                s.apply(sparse_slices(geo, rng, j))
            s.check(("sparse slices", flags))
            s.reset()
            for j in J_SPARSE:
                s.apply(np.tile(digit_groups(geo, j), 3))
            s.apply(slot_patterns(geo))
            s.check(("digit groups", flags))
        with Sketch(nt, geo, flags) as s:  # as a first apply
            s.apply(slot_patterns(geo))
            s.apply(digit_groups(geo, 1))
            s.check(("slots first", flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_log_sizes(nt, klist, r_bits, log_entries, shape):
    """key set 8: 0 keys (the sketch must not change), 1, 2, 3, a region one short / full / one over, 8191 / 8192 / 8193 (a round of a partition workgroup),
    exactly log_entries; each a sketch update of its own on one engine"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 17)
    rc = geo.region_cap
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            s.apply(np.zeros(0, np.uint32))
            s.apply(uniform(geo, rng, 1))
            s.apply(np.zeros(0, np.uint32))
            for n in (2, 3, rc - 1, rc, rc + 1, 8191, 8192, 8193, geo.log_entries):
                s.apply(uniform(geo, rng, n))
            s.check(("sizes", flags))
            s.apply(np.zeros(0, np.uint32))
            s.check(("sizes + empty", flags))
        for n in (1, 3, rc + 1):  # as the one and only apply
            with Sketch(nt, geo, flags) as s:
                s.apply(uniform(geo, rng, n))
                s.check(("size alone", n, flags))


@pytest.mark.parametrize("klist,r_bits,log_entries,shape", GEOMETRIES)
def test_an_apply_adds_to_what_the_caller_wrote(nt, klist, r_bits, log_entries, shape):
    """ntc_device_state has handed the counters' address out and the caller has added to a counter through it: an apply without a reset() adds to that value
    — also behind a reset(), since the caller may write at any time"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 19)
    mark = geo.counters - 3
    n = min(20000, geo.log_entries // 2)
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            got, _ = s.view()
            got[mark] += 7
            torch.cuda.synchronize()
            s.extra[mark] = 7
            s.apply(np.concatenate([uniform(geo, rng, n), np.full(5, mark, np.uint32), in_slice(geo, rng, geo.n_slices - 1, 3000)]))
            s.check(("caller's value", flags))
            s.reset()
            got[mark] += 9
            torch.cuda.synchronize()
            s.extra[mark] = 9
            s.apply(np.concatenate([uniform(geo, rng, n), np.full(2, mark ^ 1, np.uint32)]))
            s.check(("caller's value behind a reset", flags))


EXPORTS = [([20, 24, 32], 13, 1 << 16, (1, 2, 3, 6, 64)), ([32], 15, 1 << 14, (1, 2, 64)), ([32], 23, 1 << 18, (1, 2, 64))]


@pytest.mark.parametrize("klist,r_bits,log_entries,parts", EXPORTS)
def test_export_of_injected_keys(nt, klist, r_bits, log_entries, parts):
    """ntc_log_export_device over injected keys: per part exactly numpy's multiset for keys // (counters / n_parts) — keys on both sides of every range
    boundary, empty parts —; the log stays pending and a following flush counts the same keys; after that apply an export is refused"""
    geo = Geo(klist, r_bits, log_entries)
    rng = np.random.default_rng(r_bits + 23)
    edges = sorted({p * (geo.counters // n) + o for n in parts for p in range(n + 1) for o in (-2, -1, 0, 1)})
    edges = [k for k in edges if 0 <= k < geo.counters]
    sets = {
        "edges": np.concatenate([np.repeat(np.array(edges, dtype=np.uint32), 3), uniform(geo, rng, geo.log_entries // 2)]),
        "lower half": uniform(geo, rng, geo.log_entries) % np.uint32(geo.counters // 2),                                  # the upper parts are empty
        "one part of 64": np.uint32(geo.counters // 64 * 5) + uniform(geo, rng, 3000) % np.uint32(geo.counters // 64),     # 63 of 64 parts are empty
        "full": uniform(geo, rng, geo.room),
    }
    for name, keys in sets.items():
        keys = rng.permutation(keys.astype(np.uint32))
        with Sketch(nt, geo, 0) as s:
            s.keys.append(s.inject(keys))
            for n in parts:
                per = geo.counters // n
                owner = keys.astype(np.int64) // per
                want = np.bincount(owner, minlength=n)
                counts = s.e.log_export(n)
                assert counts == [int(x) for x in want], (name, n)
                offs = np.concatenate([[0], np.cumsum(want)]).astype(np.int64)
                buf = torch.full((keys.size + 1,), -1, dtype=torch.int32, device="cuda")
                assert s.e.log_export(n, buf.data_ptr(), offs[:-1]) == counts
                torch.cuda.synchronize()
                out = buf.cpu().numpy().view(np.uint32)
                assert out[keys.size] == 0xffffffff, "written behind the last part"
                for p in range(n):
                    assert np.array_equal(np.sort(out[offs[p]:offs[p + 1]]), np.sort(keys[owner == p])), (name, n, p)
            s.e.flush()  # still pending: the engine's own update counts the same keys
            s.check(("export", name))
            s.inject(keys[:100])
            with pytest.raises(nt.NtcError):  # the sketch holds counts now
                s.e.log_export(parts[0])
            s.keys.append(keys[:100])
            s.e.flush()
            s.check(("export refused, log intact", name))


def test_refusals(nt):
    """no device work is started by a refused call: the engine counts what it was given before and after"""
    geo = Geo([32], 16, 1 << 14)
    rng = np.random.default_rng(29)
    big = torch.zeros(2 * geo.log_entries, dtype=torch.int32, device="cuda")
    for flags in _modes(nt):
        with Sketch(nt, geo, flags) as s:
            s.keys.append(s.inject(uniform(geo, rng, 1000)))
            with pytest.raises(nt.NtcError):
                s.e.log_replace(big.data_ptr(), 2 * geo.log_entries)
            with pytest.raises(nt.NtcError):
                s.e.log_replace(big.data_ptr(), geo.room + 1)
            s.e.flush()                           # the pending log is what it was
            s.apply(uniform(geo, rng, geo.room))  # what Geo calls the room is the room
            s.check(("refused", flags))
    with nt.Engine([32], r_bits=16, s_bits=7, flags=nt.FLAG_DIRECT_ATOMICS) as e:  # no log
        with pytest.raises(nt.NtcError):
            e.log_replace(big.data_ptr(), 100)
        with pytest.raises(nt.NtcError):
            e.log_export(2)
        tc, ph, f1 = e.finish(counters=True)
        assert not tc.any() and not f1.any()
