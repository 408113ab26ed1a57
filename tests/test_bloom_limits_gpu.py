"""GPU tests of the Bloom family's limits and loops (ntcard_amd/csrc/ntc_bloom_walk.hpp, ntc_bloom.hip, ntc_cbloom.hip, ntc_bbloom.hip;
ntcard_amd/bloom.py) that the tests of each feature do not reach:
  the walk at k = 128 .. 600 (kMaxK), where a lane's outgoing base lies dozens of lanes' runs behind the incoming one and one block holds many sequences
      shorter than k;
  the SECOND sweep of the grid-stride loops (stride_grid caps a launch at 4096 workgroups of 256 lanes: 2^20 items per sweep) of insert_hashes_kernel and
      query_hashes_kernel over each view, bloom_or_kernel, cbloom_add_kernel, cbloom_threshold_kernel and bbloom_hist_kernel;
  every call on a caller's stream that is not the default one, its input arriving late on that stream;
  filters of every kind at 0, 4, 8 and 12 bytes behind a 16-byte boundary between guard bytes, the dword path of cbloom_threshold_kernel among them;
  inputs without a window: no sequence, empty sequences only, a whole input shorter than k.
Every comparison is exact and against tests/bloom_model.py, cbloom_model.py and bbloom_model.py.  Inputs and helpers are those of tests/test_bloom_gpu.py,
test_cbloom_gpu.py and test_bbloom_gpu.py.

Not tested: the remainder by m for m between 2^33 + 9 and 2^40 — a filter of that size cannot be allocated on a machine that others share, and a
restatement of bloom_mod in Python would test the restatement."""
import functools
import random

import numpy as np
import pytest

import bbloom_model as bb
import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401  (nt: the fixture)
from test_bbloom_gpu import GUARD, guarded, guards_are_zero
from test_bbloom_gpu import adversarial as block_adversarial
from test_bloom_gpu import B, STRANDS, adversarial, mixed_seqs, padding_is_zero, put
from test_cbloom_gpu import layouts, pad_is_zero, put_at

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H = 3
M = (1 << 20) + 7          # the plain filter of the walk tests
# the small filter that is queried, with one hash and with two: half of a layout fills it to 98 % with one hash (false positives and misses) and all but
# wholly with two (misses are few, in one layout none)
M_QUERY, H_QUERY = 4093, (1, 2)
M_COUNT = 4099              # the counting filter of the walk tests
M_SOLID, H_SOLID = (1 << 16) + 3, 2  # the plain filter a solid insert fills: another size and hash count than the counting filter's
BLOCKED = ((64, 3), (1, 8))  # (blocks, hashes) of the blocked filters of the walk tests


# ---- 1: the walk at large k ----
ALL_K, PLAIN_K = (128, 256, 600), (255, 257, 599)
OTHER = {128: "forward", 255: "reverse", 256: "reverse", 257: "forward", 599: "forward"}  # the strand beside the canonical one where not all three run
LAYOUTS = ("boundary-1", "boundary+0", "N@B+k-2", "N@2B+k-1")
LEADS = (0, 7)  # the address of the first base modulo 16; put_at's offsets[0] is 16


def strands_of(k):
    return STRANDS if k == 600 else ["canonical", OTHER[k]]


def half_of(seqs, k):
    """what the QUERIED filter holds: every second sequence — of a layout that is one sequence, its first 1500 windows — so that the query of all sequences
    meets k-mers the filter never saw"""
    return tuple(seqs[::2]) if len(seqs) > 1 else (seqs[0][: 1500 + k - 1],)


def hits_and_misses(hit, allv, known_values):
    """whether, in the MODEL, k-mers that were never inserted are found (false positives) and are not found (misses), and every inserted one is found"""
    known = np.isin(allv, known_values)
    return bool((hit & ~known).any() and (~hit).any() and hit[known].all())


@functools.lru_cache(maxsize=4)
def plain_walk_model(k, name, strand):
    seqs, st = layouts(k)[name], sm.STRANDS[strand]
    half = half_of(seqs, k)
    want, n_win = bm.build(list(seqs), k, st, H, M)
    assert n_win > 2 * B
    asked = {}
    for n_hash in H_QUERY:
        img, _ = bm.build(list(half), k, st, n_hash, M_QUERY)
        asked[n_hash] = (img,) + bm.query(img, list(seqs), k, st, n_hash, M_QUERY)
    allv = cm.all_values(seqs, k, st)
    hit = bm.bits_set(asked[1][0], bm.positions(allv, 1, k, M_QUERY)).all(axis=1)
    assert hits_and_misses(hit, allv, cm.all_values(half, k, st)), (k, name, strand)
    return want, n_win, asked


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("k", ALL_K + PLAIN_K)
def test_plain_walk_at_large_k(nt, k, name):
    seqs = layouts(k)[name]
    half = half_of(seqs, k)
    for strand in strands_of(k):
        want, n_win, asked = plain_walk_model(k, name, strand)
        for lead in LEADS:
            d, offs = put_at(seqs, lead)
            assert int(offs[0]) != 0
            f = nt.BloomFilter(M, H, k, strand)
            assert f.insert(d, offs) == n_win, (strand, lead)
            assert np.array_equal(f.bytes(), want) and padding_is_zero(f), (strand, lead)
            dh, oh = put_at(half, lead)
            for n_hash, (img, mw, mh) in asked.items():
                g = nt.BloomFilter(M_QUERY, n_hash, k, strand)
                g.insert(dh, oh)
                assert np.array_equal(g.bytes(), img), (strand, lead, n_hash)
                w, h = g.query(d, offs)
                assert np.array_equal(w, mw) and np.array_equal(h, mh), (strand, lead, n_hash)


@functools.lru_cache(maxsize=4)
def counting_walk_model(k, name, strand):
    """-> (counters, windows, profile, {min_count: (windows, hits)}, mid, the values that pass mid): mid is the MEDIAN count of the input's windows in the
    model, a threshold with windows below it, at it and above it — at 1 and 2 every window of this input passes"""
    seqs, st = layouts(k)[name], sm.STRANDS[strand]
    cnt, n_win = cm.counters(seqs, k, st, H, M_COUNT)
    c = cm.counts(cnt, cm.all_values(seqs, k, st), H, k)
    mid = int(np.median(c))
    assert 2 < mid < 255 and (c < mid).any() and (c == mid).any() and (c > mid).any(), (k, name, strand)
    queries = {mc: cm.query(cnt, seqs, k, st, H, mc) for mc in (1, 2, mid)}
    solid = cm.solid_values(cnt, seqs, k, st, H, mid)
    assert 0 < solid.size < n_win and int(queries[mid][1].sum()) == solid.size
    return cnt, n_win, cm.profile(cnt, seqs, k, st, H), queries, mid, solid


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("k", ALL_K)
def test_counting_walk_at_large_k(nt, k, name):
    seqs = layouts(k)[name]
    for strand in strands_of(k):
        cnt, n_win, prof, queries, mid, solid = counting_walk_model(k, name, strand)
        solid_img = bm.image_of(bm.positions(solid, H_SOLID, k, M_SOLID), M_SOLID)
        for lead in LEADS:
            d, offs = put_at(seqs, lead)
            f = nt.CountingBloomFilter(M_COUNT, H, k, strand)
            assert f.insert(d, offs) == n_win, (strand, lead)
            assert np.array_equal(f.counters(), cnt) and pad_is_zero(f), (strand, lead)
            assert np.array_equal(f.profile(d, offs), prof), (strand, lead)
            for mc, (mw, mh) in queries.items():
                w, h = f.query(d, offs, mc)
                assert np.array_equal(w, mw) and np.array_equal(h, mh), (strand, lead, mc)
            into = nt.BloomFilter(M_SOLID, H_SOLID, k, strand)
            assert f.solid(d, offs, mid, into) == solid.size, (strand, lead)
            assert np.array_equal(into.bytes(), solid_img) and padding_is_zero(into), (strand, lead)


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("k", ALL_K)
def test_blocked_walk_at_large_k(nt, k, name):
    seqs = layouts(k)[name]
    half = half_of(seqs, k)
    for strand in strands_of(k):
        st = sm.STRANDS[strand]
        cnt, n_win, _, _, mid, solid = counting_walk_model(k, name, strand)
        allv, halfv = cm.all_values(seqs, k, st), cm.all_values(half, k, st)
        for lead in LEADS:
            d, offs = put_at(seqs, lead)
            cbf = nt.CountingBloomFilter(M_COUNT, H, k, strand)
            assert cbf.insert(d, offs) == n_win and np.array_equal(cbf.counters(), cnt)
            for n_blocks, n_hash in BLOCKED:
                m = 512 * n_blocks
                f, whole = guarded(nt, m, n_hash, k, strand)
                assert f.insert(d, offs) == n_win, (strand, lead, n_blocks)
                assert np.array_equal(f.bytes(), bb.image_of(allv, n_hash, k, m)) and guards_are_zero(f, whole), (strand, lead, n_blocks)
                img = bb.image_of(halfv, n_hash, k, m)
                if n_blocks == 64:
                    assert hits_and_misses(bb.test_values(img, allv, n_hash, k, m), allv, halfv)
                g, gw = guarded(nt, m, n_hash, k, strand)
                assert g.insert(*put_at(half, lead)) == halfv.size and np.array_equal(g.bytes(), img), (strand, lead, n_blocks)
                w, h = g.query(d, offs)
                mw, mh = bb.query(img, seqs, k, st, n_hash, m)
                assert np.array_equal(w, mw) and np.array_equal(h, mh) and guards_are_zero(g, gw), (strand, lead, n_blocks)
                s, sw = guarded(nt, m, n_hash, k, strand)
                assert s.insert_solid(cbf, d, offs, mid) == solid.size, (strand, lead, n_blocks)
                assert np.array_equal(s.bytes(), bb.image_of(solid, n_hash, k, m)) and guards_are_zero(s, sw), (strand, lead, n_blocks)


# ---- 2: the second sweep of the grid-stride loops ----
SWEEP = 1 << 20            # 4096 workgroups of 256 lanes: item SWEEP is the first of a lane's second turn
N_VALUES = SWEEP + 4097


@functools.lru_cache(maxsize=None)
def stride_values():
    """-> (inserted, asked): 2^20 + 4097 values each; the last 4096 inserted ones are one value, so the second sweep is not all-distinct"""
    rng = np.random.default_rng(20)
    h0 = rng.integers(0, 2**64, size=N_VALUES, dtype=np.uint64)
    h0[-4096:] = h0[-4096]
    return h0, rng.integers(0, 2**64, size=N_VALUES, dtype=np.uint64)


def both_answers(flags):
    """the model's answers of the second sweep are not all alike"""
    return bool(flags[SWEEP:].any() and not flags[SWEEP:].all())


def test_plain_hashes_beyond_one_sweep(nt):
    h0, fresh = stride_values()
    m, k = (1 << 23) + 9, 32
    first = bm.image_of(bm.positions(h0[:SWEEP], H, k, m), m)
    want = bm.image_of(bm.positions(h0[SWEEP:], H, k, m), m, into=first.copy())
    assert not np.array_equal(want, first)  # the second sweep sets bits of its own
    flags = bm.bits_set(want, bm.positions(fresh, H, k, m)).all(axis=1)
    assert both_answers(flags)
    f = nt.BloomFilter(m, H, k)
    f.insert_hashes(h0)
    assert np.array_equal(f.bytes(), want) and padding_is_zero(f) and f.n_inserted == N_VALUES
    assert np.array_equal(f.query_hashes(fresh), flags)
    assert f.query_hashes(h0).all()


def test_counting_hashes_beyond_one_sweep(nt):
    h0, fresh = stride_values()
    m, k = (1 << 22) + 5, 32
    first = cm.counters_of(h0[:SWEEP], H, k, m)
    want = cm.counters_of(h0[SWEEP:], H, k, m, into=first)
    assert int((want != first).sum()) >= 4 and (want == 255).any()  # the one value of the second sweep, 4096 times, saturates its counters
    counts = cm.counts(want, fresh, H, k)
    assert both_answers(counts != 0) and (counts[SWEEP:] >= 2).any()
    f = nt.CountingBloomFilter(m, H, k)
    f.insert_hashes(h0)
    assert np.array_equal(f.counters(), want) and pad_is_zero(f)
    assert np.array_equal(f.counts_of_hashes(fresh), counts)
    assert np.array_equal(f.counts_of_hashes(h0), cm.counts(want, h0, H, k))


def test_blocked_hashes_beyond_one_sweep(nt):
    h0, fresh = stride_values()
    m, k = 512 * ((1 << 13) + 3), 32
    first = bb.image_of(h0[:SWEEP], H, k, m)
    want = bb.image_of(h0[SWEEP:], H, k, m, into=first.copy())
    assert not np.array_equal(want, first)
    flags = bb.test_values(want, fresh, H, k, m)
    assert both_answers(flags)
    f, whole = guarded(nt, m, H, k)
    f.insert_hashes(h0)
    assert np.array_equal(f.bytes(), want) and guards_are_zero(f, whole)
    assert np.array_equal(f.query_hashes(fresh), flags)
    assert f.query_hashes(h0).all()


def fill(f, image):
    """the filter's bytes from a host image (what load() does)"""
    f.filter[: image.size] = torch.from_numpy(image).cuda()


def test_or_beyond_one_sweep(nt):
    """m_bits = 2^25 + 1031: 1 048 609 dwords, the last one partial; dwords of the source that are zero (skipped) and that are not, in both sweeps"""
    m, k = (1 << 25) + 1031, 32
    n = bm.n_bytes(m)
    assert (n + 3) // 4 == SWEEP + 33 and m % 32 != 0
    rng = np.random.default_rng(21)
    a, b = rng.integers(0, 256, size=(2, n), dtype=np.uint8)
    skip = np.repeat(rng.integers(0, 2, size=(n + 3) // 4, dtype=np.uint8), 4)[:n] == 0
    b[skip] = 0
    a[-1], b[-1] = 0x44, 0x82  # the last byte holds 7 positions: no bit from m_bits on
    assert m % 8 == 7 and not (a[-1] | b[-1]) & 1
    both = a | b
    tail = slice(4 * SWEEP, n)
    assert not np.array_equal(both[tail], a[tail]) and skip[tail].any() and not skip[tail].all()
    f, g = nt.BloomFilter(m, H, k), nt.BloomFilter(m, H, k)
    fill(f, a)
    fill(g, b)
    f.merge(g)
    assert np.array_equal(f.bytes(), both) and padding_is_zero(f)
    assert np.array_equal(g.bytes(), b)


def test_add_beyond_one_sweep(nt):
    """m = 2^22 + 5: the second sweep is the last two dwords — a counter at 255, a pair whose sum saturates, a zero of the source beside counters that are
    not, and a source dword that is all zeros (skipped)"""
    m, k = (1 << 22) + 5, 32
    rng = np.random.default_rng(22)
    palette = np.array([0, 0, 0, 1, 1, 2, 3, 17, 100, 128, 200, 254, 255], dtype=np.uint8)
    a, b = palette[rng.integers(0, palette.size, size=(2, m))]
    a[4 * SWEEP:] = [255, 200, 7, 9, 5]
    b[4 * SWEEP:] = [3, 100, 0, 1, 0]
    want = cm.merge(a, b)
    assert want[4 * SWEEP:].tolist() == [255, 255, 7, 10, 5] and (want[: 4 * SWEEP] == 255).any()
    f, g = nt.CountingBloomFilter(m, H, k), nt.CountingBloomFilter(m, H, k)
    fill(f, a)
    fill(g, b)
    f.merge(g)
    assert np.array_equal(f.counters(), want) and pad_is_zero(f)
    assert np.array_equal(g.counters(), b)


@functools.lru_cache(maxsize=None)
def threshold_counters():
    """2^25 + 33 counters: five eighths are zero; the 33 of the second sweep (filter dwords 2^20 and 2^20 + 1) hold every class of value"""
    m = (1 << 25) + 33
    rng = np.random.default_rng(23)
    palette = np.array([0] * 10 + [1, 1, 2, 3, 254, 255], dtype=np.uint8)
    cnt = palette[rng.integers(0, palette.size, size=m, dtype=np.uint8)]
    cnt[1 << 25:] = ([0, 1, 2, 3, 254, 255, 1, 0] * 5)[:33]
    return cnt


@pytest.mark.parametrize("min_count", [1, 2, 255])
def test_threshold_beyond_one_sweep(nt, min_count):
    cnt = threshold_counters()
    m = cnt.size
    assert bm.n_bytes(m) == 4 * SWEEP + 5
    want = cm.threshold(cnt, min_count)
    tail = np.unpackbits(want[4 * SWEEP:])[:33]  # the positions of the second sweep
    assert tail.any() and not tail.all()
    f = nt.CountingBloomFilter(m, H, 32)
    fill(f, cnt)
    g = f.threshold(min_count)
    assert np.array_equal(g.bytes(), want) and padding_is_zero(g)


def test_block_histogram_beyond_one_sweep(nt):
    """2^20 + 3 blocks, bin for bin: a quarter of them empty, the others filled around 256, 128 and 64 bits; in the second sweep a full block, one of 511
    bits and one of 1"""
    n_blocks = SWEEP + 3
    rng = np.random.default_rng(24)
    img = rng.integers(0, 256, size=(n_blocks, 64), dtype=np.uint8)
    thin = rng.integers(0, 4, size=n_blocks, dtype=np.uint8)  # 0: the block is empty; 1 .. 3: random bytes under thin - 1 random masks
    for t in (2, 3):
        sel = thin >= t
        img[sel] &= rng.integers(0, 256, size=(int(sel.sum()), 64), dtype=np.uint8)
    img[thin == 0] = 0
    img[-3] = 0xFF
    img[-2] = 0xFF
    img[-2, 0] = 0x7F
    img[-1] = 0
    img[-1, 63] = 0x01
    img = img.reshape(-1)
    want = bb.block_hist(img)
    assert int(want[512]) == 1 and int(want[511]) == 1 and int(want[0]) > n_blocks // 5 and int((want != 0).sum()) > 100 and int(want.sum()) == n_blocks
    f = nt.BlockedBloomFilter(512 * n_blocks, H, 32)
    fill(f, img)
    assert np.array_equal(f.block_hist(), want)


# ---- 3: the caller's stream ----
class Late:
    """Device tensors whose content arrives LATE on a side stream.  late(dst, real, stale) queues on the current stream, without waiting for anything:
    dst <- stale, a sort of 2^24 values (milliseconds), dst <- real.  A library call issued right behind it is ordered behind the copy only if ALL of its
    work — kernels, memsets, copies — is on the caller's stream; work on any other stream reads the stale content or an unfinished filter, and the
    comparison with the model fails.  A library that keeps to the stream can never fail it."""

    def __init__(self):
        self.ballast = torch.randint(0, 1 << 30, (1 << 24,), dtype=torch.int32, device="cuda")
        self.side = torch.cuda.Stream()
        assert self.side.cuda_stream != torch.cuda.default_stream().cuda_stream

    def __enter__(self):
        self.side.wait_stream(torch.cuda.current_stream())  # what the test prepared on the default stream is there; the host does not wait
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        assert torch.cuda.current_stream() == self.side
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        self.side.synchronize()
        return False

    def __call__(self, dst, real, stale):
        assert torch.cuda.current_stream() == self.side and dst.shape == real.shape
        dst.fill_(stale)
        torch.sort(self.ballast)
        dst.copy_(real)
        return dst


@functools.lru_cache(maxsize=None)
def stream_input():
    """-> (sequences, every second one, values asked for): about 60 sequences over four blocks, k = 32"""
    seqs = mixed_seqs(32, seed=41, n=60)
    rng = np.random.default_rng(41)
    asked = np.concatenate([cm.all_values(seqs[::2], 32, sm.CANONICAL)[:3000], rng.integers(0, 2**64, size=3000, dtype=np.uint64)])
    assert sum(map(len, seqs)) > 3 * B
    return seqs, seqs[::2], asked


def staged(seqs):
    """-> (the real bases on the device, a tensor of the same size full of N, host offsets)"""
    real, offs = put(seqs, lead=3)
    return real, torch.full_like(real, ord("N")), offs


def device_hashes(h0):
    """-> (the values on the device as int64, a tensor of the same size full of zeros)"""
    real = dev(np.ascontiguousarray(h0).view(np.int64))
    return real, torch.zeros_like(real)


def test_plain_filter_on_a_side_stream(nt):
    k, m, st = 32, (1 << 16) + 5, sm.CANONICAL
    seqs, half, asked = stream_input()
    img_all, n_all = bm.build(list(seqs), k, st, H, m)
    img_half, n_half = bm.build(list(half), k, st, H, m)
    mw, mh = bm.query(img_half, list(seqs), k, st, H, m)
    flags = bm.bits_set(img_half, bm.positions(asked, H, k, m)).all(axis=1)
    assert 0 < int(mh.sum()) < int(mw.sum()) and flags.any() and not flags.all()
    real_all, d_all, o_all = staged(seqs)
    real_half, d_half, o_half = staged(half)
    real_h, d_h = device_hashes(cm.all_values(half, k, st))
    real_q, d_q = device_hashes(asked)
    real_img = dev(np.concatenate([img_all, np.zeros(-img_all.size % 4, dtype=np.uint8)]))
    with Late() as late:
        f = nt.BloomFilter(m, H, k)
        late(d_half, real_half, ord("N"))
        assert f.insert(d_half, o_half) == n_half
        assert np.array_equal(f.bytes(), img_half)
        late(d_all, real_all, ord("N"))
        w, h = f.query(d_all, o_all)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        g = nt.BloomFilter(m, H, k)
        late(d_h, real_h, 0)
        g.insert_hashes(d_h)
        assert np.array_equal(g.bytes(), img_half)
        late(d_q, real_q, 0)
        assert np.array_equal(g.query_hashes(d_q), flags)
        other = nt.BloomFilter(m, H, k)
        late(other.filter, real_img, 0)
        g.merge(other)
        assert np.array_equal(g.bytes(), img_all)
        late(other.filter, real_img, 0)
        assert other.popcount() == bm.popcount(img_all)


def test_counting_filter_on_a_side_stream(nt):
    k, m, st = 32, 4099, sm.CANONICAL
    seqs, half, asked = stream_input()
    twice = tuple(seqs) + tuple(half)  # every second sequence twice: true counts of 2
    cnt, n_win = cm.counters(twice, k, st, H, m)
    c = cm.counts(cnt, cm.all_values(twice, k, st), H, k)
    mid = int(np.median(c))
    assert (c < mid).any() and (c == mid).any() and (c > mid).any()
    mw, mh = cm.query(cnt, twice, k, st, H, mid)
    solid = cm.solid_values(cnt, twice, k, st, H, mid)
    half_cnt, n_half = cm.counters(half, k, st, H, m)
    real, d, offs = staged(twice)
    real_h, d_h = device_hashes(cm.all_values(half, k, st))
    real_q, d_q = device_hashes(asked)
    real_cnt = dev(np.concatenate([cnt, np.zeros(-cnt.size % 4, dtype=np.uint8)]))
    with Late() as late:
        f = nt.CountingBloomFilter(m, H, k)
        late(d, real, ord("N"))
        assert f.insert(d, offs) == n_win
        assert np.array_equal(f.counters(), cnt)
        late(d, real, ord("N"))
        w, h = f.query(d, offs, mid)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        late(d, real, ord("N"))
        assert np.array_equal(f.profile(d, offs), cm.profile(cnt, twice, k, st, H))
        g = nt.CountingBloomFilter(m, H, k)
        late(d_h, real_h, 0)
        g.insert_hashes(d_h)
        assert np.array_equal(g.counters(), half_cnt)
        late(d_q, real_q, 0)
        assert np.array_equal(g.counts_of_hashes(d_q), cm.counts(half_cnt, asked, H, k))
        other = nt.CountingBloomFilter(m, H, k)
        late(other.filter, real_cnt, 0)
        g.merge(other)
        assert np.array_equal(g.counters(), cm.merge(half_cnt, cnt))
        late(other.filter, real_cnt, 0)
        assert np.array_equal(other.hist(), cm.hist(cnt))
        late(other.filter, real_cnt, 0)
        assert np.array_equal(other.threshold(mid).bytes(), cm.threshold(cnt, mid))
        into = nt.BloomFilter(M_SOLID, H_SOLID, k)
        late(d, real, ord("N"))
        assert f.solid(d, offs, mid, into) == solid.size
        assert np.array_equal(into.bytes(), bm.image_of(bm.positions(solid, H_SOLID, k, M_SOLID), M_SOLID))
        blocked = nt.BlockedBloomFilter(64 * 512, H, k)
        late(d, real, ord("N"))
        assert blocked.insert_solid(f, d, offs, mid) == solid.size
        assert np.array_equal(blocked.bytes(), bb.image_of(solid, H, k, 64 * 512))


def test_blocked_filter_on_a_side_stream(nt):
    k, m, st = 32, 64 * 512, sm.CANONICAL
    seqs, half, asked = stream_input()
    img_all, n_all = bb.build(list(seqs), k, st, H, m)
    img_half, n_half = bb.build(list(half), k, st, H, m)
    mw, mh = bb.query(img_half, list(seqs), k, st, H, m)
    flags = bb.test_values(img_half, asked, H, k, m)
    assert 0 < int(mh.sum()) < int(mw.sum()) and flags.any() and not flags.all()
    real_all, d_all, o_all = staged(seqs)
    real_half, d_half, o_half = staged(half)
    real_h, d_h = device_hashes(cm.all_values(half, k, st))
    real_q, d_q = device_hashes(asked)
    real_img = dev(img_all)
    with Late() as late:
        f = nt.BlockedBloomFilter(m, H, k)
        late(d_half, real_half, ord("N"))
        assert f.insert(d_half, o_half) == n_half
        assert np.array_equal(f.bytes(), img_half)
        late(d_all, real_all, ord("N"))
        w, h = f.query(d_all, o_all)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        g = nt.BlockedBloomFilter(m, H, k)
        late(d_h, real_h, 0)
        g.insert_hashes(d_h)
        assert np.array_equal(g.bytes(), img_half)
        late(d_q, real_q, 0)
        assert np.array_equal(g.query_hashes(d_q), flags)
        other = nt.BlockedBloomFilter(m, H, k)
        late(other.filter, real_img, 0)
        g.merge(other)
        assert np.array_equal(g.bytes(), img_all)
        late(other.filter, real_img, 0)
        assert other.popcount() == bm.popcount(img_all)
        late(other.filter, real_img, 0)
        assert np.array_equal(other.block_hist(), bb.block_hist(img_all))


# ---- 4: alignment and guard bytes ----
SHIFTS = (0, 4, 8, 12)


def in_guards(f, shift):
    """test_bbloom_gpu.guarded's pattern for a plain or a counting filter, whose tensor is padded to whole dwords: the tensor's bytes inside a larger zeroed
    one, GUARD + shift bytes from its start -> (filter, the whole tensor).  guards_are_zero then looks at every byte but the filter's n_bytes: the padding of
    the last dword — which the kernels may write, as zeros — and the guards"""
    n = f.filter.numel()
    whole = torch.zeros(GUARD + shift + n + GUARD, dtype=torch.uint8, device="cuda")
    f.filter = whole[GUARD + shift: GUARD + shift + n]
    assert f.filter.data_ptr() % 16 == shift and n % 4 == 0 and n - f.n_bytes < 4
    return f, whole


@functools.lru_cache(maxsize=None)
def guard_input():
    """-> sequences over two blocks, a third of them twice, k = 32: true counts of 1 and of 2"""
    seqs = mixed_seqs(32, seed=51, n=30)
    return seqs + seqs[5:15]


@pytest.mark.parametrize("m", [9, 33, 4099, (1 << 16) + 1])
@pytest.mark.parametrize("shift", SHIFTS)
def test_plain_filter_between_guards(nt, shift, m):
    k, st = 32, sm.CANONICAL
    assert m % 32 != 0  # a partial last dword
    seqs = guard_input()
    d, offs = put(seqs, lead=shift + 1)
    want, n_win = bm.build(list(seqs), k, st, H, m)
    f, whole = in_guards(nt.BloomFilter(m, H, k), shift)
    assert f.insert(d, offs) == n_win and np.array_equal(f.bytes(), want) and guards_are_zero(f, whole)
    h0 = adversarial(m, random.Random(m + shift))
    g, gw = in_guards(nt.BloomFilter(m, H, k), (shift + 4) % 16)
    g.insert_hashes(h0)
    img = bm.image_of(bm.positions(h0, H, k, m), m)
    assert np.array_equal(g.bytes(), img) and guards_are_zero(g, gw)
    assert np.array_equal(g.query_hashes(h0[:100]), np.ones(100, dtype=bool))
    g.merge(f)
    assert np.array_equal(g.bytes(), img | want) and guards_are_zero(g, gw) and guards_are_zero(f, whole)
    assert g.popcount() == bm.popcount(img | want)  # (the popcount refuses an image with a bit behind m_bits)


def threshold_into(f, min_count, shift):
    """ntc_cbloom_threshold_device of the counting filter f into a plain filter between guards, `shift` bytes behind a 16-byte boundary -> (filter, whole)"""
    from ntcard_amd import _abi
    import ntcard_amd
    g, whole = in_guards(ntcard_amd.BloomFilter(f.m_bits, f.n_hash, f.k), shift)
    _abi.check(_abi.lib().ntc_cbloom_threshold_device(0, None, f.filter.data_ptr(), f.m_bits, min_count, g.filter.data_ptr()))
    return g, whole


@pytest.mark.parametrize("m", [9, 33, 4099])
@pytest.mark.parametrize("shift", SHIFTS)
def test_counting_filter_between_guards(nt, shift, m):
    """off a 16-byte boundary cbloom_threshold_kernel reads its 32 counters dword by dword; the last filter dword of these m has fewer than 8 counter
    dwords (m = 9: 3 of 8; m = 33 and 4099: 1 of 8), at shift 0 and 8 too, where the 16-byte loads would reach behind the array"""
    k, st = 32, sm.CANONICAL
    seqs = guard_input()
    d, offs = put(seqs, lead=shift + 1)
    rng = np.random.default_rng(m + shift)
    h0 = rng.integers(0, 2**64, size=max(8, m), dtype=np.uint64)
    want = cm.counters_of(h0, H, k, m)
    f, whole = in_guards(nt.CountingBloomFilter(m, H, k), shift)
    f.insert_hashes(h0)
    assert np.array_equal(f.counters(), want) and guards_are_zero(f, whole) and int(want.max()) < 255
    assert np.array_equal(f.counts_of_hashes(h0), cm.counts(want, h0, H, k))
    assert 2 <= int(want.max()) and int(want.min()) < int(want.max())
    for c in sorted({1, 2, int(want.max())}):
        g, gw = threshold_into(f, c, 4)
        assert np.array_equal(g.bytes(), cm.threshold(want, c)) and guards_are_zero(g, gw), c
        assert guards_are_zero(f, whole)
    other, ow = in_guards(nt.CountingBloomFilter(m, H, k), (shift + 4) % 16)
    cnt, n_win = cm.counters(seqs, k, st, H, m)
    assert other.insert(d, offs) == n_win and np.array_equal(other.counters(), cnt) and guards_are_zero(other, ow)
    f.merge(other)
    both = cm.merge(want, cnt)
    assert np.array_equal(f.counters(), both) and guards_are_zero(f, whole) and guards_are_zero(other, ow)
    g, gw = threshold_into(f, 255, 4)
    assert np.array_equal(g.bytes(), cm.threshold(both, 255)) and guards_are_zero(g, gw)
    assert int(f.hist().sum()) == m  # (hist refuses an array with a byte behind its m counters)


@pytest.mark.parametrize("shift", SHIFTS)
def test_solid_inserts_between_guards(nt, shift):
    """counters, the plain and the blocked destination each between guards; at min_count = 2 windows of count 1, of count 2 and above all occur"""
    k, st, m = 32, sm.CANONICAL, (1 << 16) + 3
    seqs = guard_input()
    d, offs = put(seqs, lead=shift + 1)
    cnt, n_win = cm.counters(seqs, k, st, H, m)
    c = cm.counts(cnt, cm.all_values(seqs, k, st), H, k)
    assert (c == 1).any() and (c == 2).any() and (c > 2).any()
    solid = cm.solid_values(cnt, seqs, k, st, H, 2)
    assert 0 < solid.size < n_win
    f, whole = in_guards(nt.CountingBloomFilter(m, H, k), shift)
    assert f.insert(d, offs) == n_win and np.array_equal(f.counters(), cnt)
    into, iw = in_guards(nt.BloomFilter(4099, H_SOLID, k), (shift + 4) % 16)
    assert f.solid(d, offs, 2, into) == solid.size
    assert np.array_equal(into.bytes(), bm.image_of(bm.positions(solid, H_SOLID, k, 4099), 4099)) and guards_are_zero(into, iw)
    b, bw = guarded(nt, 8 * 512, H, k, shift=(shift + 8) % 16)
    assert b.insert_solid(f, d, offs, 2) == solid.size
    assert np.array_equal(b.bytes(), bb.image_of(solid, H, k, 8 * 512)) and guards_are_zero(b, bw)
    assert np.array_equal(f.counters(), cnt) and guards_are_zero(f, whole)  # the counting filter is only read


@pytest.mark.parametrize("shift", SHIFTS)
def test_blocked_filter_between_guards(nt, shift):
    """test_bbloom_gpu.py places its filters at shift 0 and 4: here the walk, the given values and the merge at all four"""
    k, st, m = 32, sm.CANONICAL, 67 * 512
    seqs = guard_input()
    d, offs = put(seqs, lead=shift + 1)
    want, n_win = bb.build(list(seqs), k, st, H, m)
    f, whole = guarded(nt, m, H, k, shift=shift)
    assert f.insert(d, offs) == n_win and np.array_equal(f.bytes(), want) and guards_are_zero(f, whole)
    h0 = block_adversarial(67, random.Random(shift))[:300]
    g, gw = guarded(nt, m, H, k, shift=(shift + 4) % 16)
    g.insert_hashes(h0)
    img = bb.image_of(h0, H, k, m)
    assert np.array_equal(g.bytes(), img) and guards_are_zero(g, gw)
    g.merge(f)
    assert np.array_equal(g.bytes(), img | want) and not np.array_equal(img | want, img) and guards_are_zero(g, gw) and guards_are_zero(f, whole)
    assert np.array_equal(g.block_hist(), bb.block_hist(img | want))


# ---- 5: inputs without a window ----
NO_WINDOW = {
    "no sequence": (),
    "empty sequences": (b"", b"", b"", b""),
    "shorter than k": (b"ACGTACGTAC", b"", b"ACGTTGCAACGTAGGCTAAC"),  # 30 bases in all, k = 32
}


def prefilled(nt, kind, m, k, strand):
    """a filter of the kind with 200 values in it -> (filter, the whole device array before the call under test)"""
    f = getattr(nt, kind)(m, H, k, strand)
    f.insert_hashes(np.random.default_rng(7).integers(0, 2**64, size=200, dtype=np.uint64))
    return f, f.filter.cpu().numpy().copy()


@pytest.mark.parametrize("strand", ["canonical", "forward"])
@pytest.mark.parametrize("case", list(NO_WINDOW))
def test_inputs_without_a_window(nt, case, strand):
    k, seqs = 32, NO_WINDOW[case]
    assert sum(map(len, seqs)) < k
    d, offs = put(seqs, lead=5)
    assert offs.size == len(seqs) + 1 and int(offs[0]) == 5
    zeros = np.zeros(len(seqs), dtype=np.uint32)
    counting, cnt_before = prefilled(nt, "CountingBloomFilter", 4099, k, strand)
    for kind, m in (("BloomFilter", 4099), ("CountingBloomFilter", 4099), ("BlockedBloomFilter", 4096)):
        f, before = prefilled(nt, kind, m, k, strand)
        assert before.any()
        assert f.insert(d, offs) == 0 and f.n_inserted == 200, kind
        w, h = f.query(d, offs)
        assert w.dtype == np.uint32 and h.dtype == np.uint32 and np.array_equal(w, zeros) and np.array_equal(h, zeros), kind
        if kind == "BloomFilter":
            assert counting.solid(d, offs, 1, f) == 0
        elif kind == "BlockedBloomFilter":
            assert f.insert_solid(counting, d, offs, 1) == 0
        else:
            w, h = f.query(d, offs, 255)
            assert np.array_equal(w, zeros) and np.array_equal(h, zeros)
            prof = f.profile(d, offs)
            assert prof.dtype == np.uint8 and np.array_equal(prof, np.zeros(sum(map(len, seqs)), dtype=np.uint8))
        assert np.array_equal(f.filter.cpu().numpy(), before) and f.n_inserted == 200, kind
    assert np.array_equal(counting.filter.cpu().numpy(), cnt_before)


# ---- 6: the randomised sweep ----
def test_randomised_cases_small():
    """the short run of tools/fuzz_bloom.py (random kinds, actions, k up to 600, strands, sizes, alignments and layouts; tests/test_fuzz_bloom_host.py
    asserts what that run draws)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import fuzz_bloom
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_bloom.py"), *map(str, fuzz_bloom.SHORT_RUN)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:]
