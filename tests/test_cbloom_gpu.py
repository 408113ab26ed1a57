"""GPU tests of the counting Bloom filters (include/ntcard_hip.h: ntc_cbloom_*_device, ntc_bloom_insert_solid_device; ntcard_amd/bloom.py): the counters
an insert leaves are BYTE for byte those of tests/cbloom_model.py — one increment per position and window, min(., 255) — whatever the contention on a
dword, at and beyond saturation, across the seams of the block grid and at every alignment; query, profile, threshold, the solid insert, add and hist
give what the model gives.  Every comparison is exact.  Inputs and helpers are tests/test_bloom_gpu.py's."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401  (nt: the fixture)
from support import offsets_of
from test_bloom_gpu import B, STRANDS, adversarial, mixed_seqs, padding_is_zero, put, rand_seq, seam_layouts

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H = 3
ERR_STATE = -4


@functools.lru_cache(maxsize=None)
def values(seqs, k, strand=sm.CANONICAL):
    return cm.all_values(seqs, k, strand)


def model(seqs, k, strand, n_hash, m, into=None):
    v = values(tuple(seqs), k, strand)
    return cm.counters_of(v, n_hash, k, m, into), int(v.size)


def pad_is_zero(f):
    return not f.filter[f.m_bits:].cpu().numpy().any()


def random_windows(seed, n_windows, k=32):
    """one clean sequence of n_windows windows"""
    return (rand_seq(random.Random(seed), n_windows + k - 1),)


@functools.lru_cache(maxsize=None)
def saturation_input():
    """more than 12,000 equal windows over four workgroups, and about 300 windows of random sequence behind them"""
    return (b"A" * (3 * B + 100),) + random_windows(7, 300)


# ---- 1 ----
@pytest.mark.parametrize("strand", STRANDS)
@pytest.mark.parametrize("k", [1, 31, 32, 33, 65])
def test_counters_are_the_models_byte_for_byte(nt, k, strand):
    seqs = mixed_seqs(k)
    assert sum(map(len, seqs)) > 2 * B + k
    d, offs = put(seqs)
    for m in (4099, 1 << 14):
        want, n_win = model(seqs, k, sm.STRANDS[strand], H, m)
        f = nt.CountingBloomFilter(m, H, k, strand)
        assert f.insert(d, offs) == n_win and n_win > 0
        assert np.array_equal(f.counters(), want), (k, strand, m)
        assert pad_is_zero(f) and f.n_inserted == n_win


# ---- 2 ----
def test_no_increment_is_lost_under_dword_contention(nt):
    k = 32
    seqs = random_windows(3, 6000)
    d, offs = put(seqs)
    want, n_win = model(seqs, k, sm.CANONICAL, H, 1024)
    assert n_win == 6000 and 8 <= int(want.max()) < 255  # about 18 increments per counter, four counters per dword: every increment is visible
    f = nt.CountingBloomFilter(1024, H, k)
    assert f.insert(d, offs) == n_win
    assert np.array_equal(f.counters(), want)
    assert int(f.counters().astype(np.int64).sum()) == H * n_win


@pytest.mark.parametrize("m", [5, 7, 9, 33])
def test_small_filters_every_byte_of_a_dword(nt, m):
    """the bytes of one dword, two positions of one k-mer that coincide, the last partial dword"""
    k = 32
    seqs = random_windows(40 + m, 200)
    d, offs = put(seqs)
    want, n_win = model(seqs, k, sm.CANONICAL, H, m)
    assert int(want.max()) < 255 and int(want.astype(np.int64).sum()) == H * n_win
    pos = bm.positions(values(seqs, k), H, k, m)
    assert (pos[:, 0] == pos[:, 1]).any() or (pos[:, 1] == pos[:, 2]).any()  # coincident positions of one k-mer occur
    f = nt.CountingBloomFilter(m, H, k)
    assert f.insert(d, offs) == n_win
    assert np.array_equal(f.counters(), want) and pad_is_zero(f)


# ---- 3 ----
def test_saturation_is_exact_and_does_not_spill(nt):
    k, m = 32, 64
    seqs = saturation_input()
    d, offs = put(seqs)
    want, n_win = model(seqs, k, sm.CANONICAL, H, m)
    assert n_win > 12000 + 290
    dwords = want.reshape(-1, 4)
    mixed = [(row == 255).any() and (row < 255).any() for row in dwords]
    assert (want == 255).any() and any(mixed)  # a saturated counter with a neighbour below 255 in its dword
    f = nt.CountingBloomFilter(m, H, k)
    assert f.insert(d, offs) == n_win
    assert np.array_equal(f.counters(), want) and pad_is_zero(f)
    again, _ = model(seqs, k, sm.CANONICAL, H, m, into=want)
    assert (again[want == 255] == 255).all() and (again >= want).all() and not np.array_equal(again, want)
    assert f.insert(d, offs) == n_win
    assert np.array_equal(f.counters(), again) and pad_is_zero(f)


# ---- 4 ----
@functools.lru_cache(maxsize=None)
def layouts(k):
    return {name: tuple(seqs) for name, seqs in seam_layouts(k, random.Random(k)).items()}


def put_at(seqs, lead, first=16):
    """the source's first byte at `lead` behind a 16-byte boundary, offsets[0] = first"""
    host = np.frombuffer(b"#" * (lead + first) + b"".join(seqs) + b"#", dtype=np.uint8).copy()
    d = dev(host)[lead:]
    assert d.data_ptr() % 16 == lead
    return d, offsets_of(list(seqs), first)


@pytest.mark.parametrize("lead", [0, 1, 3, 15])
@pytest.mark.parametrize("k", [32, 127])
def test_block_seams_and_alignment(nt, k, lead):
    m = 4099
    for name, seqs in layouts(k).items():
        d, offs = put_at(seqs, lead)
        assert int(offs[0]) != 0
        want, n_win = model(seqs, k, sm.CANONICAL, H, m)
        f = nt.CountingBloomFilter(m, H, k)
        assert f.insert(d, offs) == n_win, name
        assert np.array_equal(f.counters(), want), name
        assert np.array_equal(f.profile(d, offs), cm.profile(want, seqs, k, sm.CANONICAL, H)), name


# ---- 5 ----
def profile_into(nt, f, d, offs, n, shift, guard=64):
    """ntc_cbloom_profile_device into a buffer of the fill pattern 0xAB, the output `shift` bytes behind its (aligned) start -> (the n bytes, the rest)"""
    from ntcard_amd import _abi
    buf = torch.full((shift + n + guard,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    _abi.check(_abi.lib().ntc_cbloom_profile_device(0, None, f.filter.data_ptr(), f.m_bits, f.n_hash, f.k, 0, d.data_ptr(), offs.ctypes.data_as(C.c_void_p), offs.size - 1,
                                                    buf.data_ptr() + shift))
    host = buf.cpu().numpy()
    return host[shift: shift + n], np.concatenate([host[:shift], host[shift + n:]])


@pytest.mark.parametrize("k", [1, 32, 65])
def test_profile_is_the_models(nt, k):
    m = 4099
    seqs = mixed_seqs(k)
    d, offs = put(seqs, lead=5)
    want, _ = model(seqs, k, sm.CANONICAL, H, m)
    f = nt.CountingBloomFilter(m, H, k)
    f.insert(d, offs)
    prof = cm.profile(want, seqs, k, sm.CANONICAL, H)
    n = sum(map(len, seqs))
    assert prof.size == n and (prof != 0).any()
    at = np.concatenate([cm.window_starts(s, k) for s in seqs])
    assert not prof[~at].any() and (k == 1 or (~at).sum() > (k - 1) * 200)  # zeros at every sequence's end, around non-bases, in short sequences
    assert np.array_equal(f.profile(d, offs), prof)
    for shift in (0, 1, 4, 7):  # the output at every alignment class: 16-byte, dword and byte stores
        got, rest = profile_into(nt, f, d, offs, n, shift)
        assert np.array_equal(got, prof), shift
        assert (rest == 0xAB).all(), shift


@pytest.mark.parametrize("n", [B + 21, B + 1, 2 * B + 31, 5, 31, 32, 33, B + 31, B + 32])
def test_profile_writes_the_tail_no_window_starts_in(nt, n):
    """the last block holds fewer than k positions and n is no multiple of 16: its lanes have no window and still own bytes below n; n < k: all zeros"""
    k, m = 32, 4099
    seqs = (rand_seq(random.Random(n), n),)
    d, offs = put(seqs)
    f = nt.CountingBloomFilter(m, H, k)
    want, n_win = model(seqs, k, sm.CANONICAL, H, m)
    assert f.insert(d, offs) == n_win == max(n - k + 1, 0)
    prof = cm.profile(want, seqs, k, sm.CANONICAL, H)
    assert not prof[max(n - k + 1, 0):].any()
    for shift in (0, 3):
        got, rest = profile_into(nt, f, d, offs, n, shift)
        assert np.array_equal(got, prof) and (rest == 0xAB).all(), shift


# ---- 6 ----
def test_query_counts_what_the_model_counts(nt):
    k, m = 32, 8191
    ins = mixed_seqs(k, seed=31, n=6) + mixed_seqs(k, seed=31, n=6)[:8] + mixed_seqs(k, seed=33, n=3)  # some sequences twice: true counts of 2
    rest = mixed_seqs(k, seed=32, n=150)
    d, offs = put(ins)
    dq, oq = put(rest, lead=3)
    for strand in STRANDS:
        s = sm.STRANDS[strand]
        want, _ = model(ins, k, s, H, m)
        f = nt.CountingBloomFilter(m, H, k, strand)
        f.insert(d, offs)
        assert np.array_equal(f.counters(), want)
        inserted = set(values(tuple(ins), k, s).tolist())
        for c in (1, 2, 3, 255):
            w, h = f.query(d, offs, c)
            mw, mh = cm.query(want, ins, k, s, H, c)
            assert np.array_equal(w, mw) and np.array_equal(h, mh), (strand, c)
            if c == 1:
                assert np.array_equal(h, w)  # what was inserted is found
            w, h = f.query(dq, oq, c)
            mw, mh = cm.query(want, rest, k, s, H, c)
            assert np.array_equal(w, mw) and np.array_equal(h, mh), (strand, c)
            assert w.dtype == np.uint32 and w.shape == (len(rest),)
            if c <= 3:  # false ">= c" answers: k-mers that were never inserted and read a count >= c
                v = values(tuple(rest), k, s)
                fresh = v[~np.isin(v, np.fromiter(inserted, dtype=np.uint64))]
                assert 0 < int((cm.counts(want, fresh, H, k) >= c).sum()) < fresh.size, (strand, c)
            else:
                assert int(mh.sum()) == 0
    with pytest.raises(ValueError):
        f.query(d, offs, 0)
    with pytest.raises(ValueError):
        f.query(d, offs, 256)


def test_query_of_many_short_sequences(nt):
    """thousands of sequences of a few bases in one block: more than a workgroup's table of sums in LDS holds"""
    k, m = 2, 64
    prng = random.Random(6)
    seqs = tuple(rand_seq(prng, prng.choice([0, 1, 2, 2, 3, 3, 4]), pn=0.1) for _ in range(3 * B))
    assert len(seqs) > 3 * 1024 and sum(map(len, seqs)) < 3 * len(seqs)
    d, offs = put(seqs)
    f = nt.CountingBloomFilter(m, 2, k)
    ins = (b"ACGTTGCA", b"AC", b"AC", b"CA")
    di, oi = put(ins)
    f.insert(di, oi)
    want, _ = model(ins, k, sm.CANONICAL, 2, m)
    assert np.array_equal(f.counters(), want)
    for c in (1, 2, 3):
        w, h = f.query(d, offs, c)
        mw, mh = cm.query(want, seqs, k, sm.CANONICAL, 2, c)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        assert 0 < int(mh.sum()) < int(mw.sum())


# ---- 7 ----
@functools.lru_cache(maxsize=None)
def threshold_input():
    return saturation_input() + mixed_seqs(32)[:80] + mixed_seqs(32)[:30]


@pytest.mark.parametrize("m", [9, 4099, 1 << 20])
def test_threshold(nt, m):
    k = 32
    seqs = threshold_input()
    d, offs = put(seqs)
    want, n_win = model(seqs, k, sm.CANONICAL, H, m)
    f = nt.CountingBloomFilter(m, H, k)
    assert f.insert(d, offs) == n_win and np.array_equal(f.counters(), want)
    plain = nt.BloomFilter(m, H, k)
    plain.insert(d, offs)
    one = f.threshold(1)
    assert (one.m_bits, one.n_hash, one.k, one.strand) == (m, H, k, "canonical")
    assert np.array_equal(one.filter.cpu().numpy(), plain.filter.cpu().numpy())  # the padding too
    v = values(seqs, k)
    uniq, true = np.unique(v, return_counts=True)
    rest = mixed_seqs(k, seed=32, n=60)
    dq, oq = put(rest, lead=3)
    for c in (2, 255):
        g = f.threshold(c)
        img = cm.threshold(want, c)
        assert np.array_equal(g.bytes(), img), c
        assert padding_is_zero(g) and g.popcount() == bm.popcount(img)  # ntc_bloom_popcount_device accepts it
        assert (want >= c).any()
        w, h = g.query(dq, oq)
        mw, mh = bm.query(img, rest, k, sm.CANONICAL, H, m)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        often = uniq[true >= c]
        assert often.size > 0 and g.query_hashes(often).all()  # no k-mer of true count >= c misses
    with pytest.raises(ValueError):
        f.threshold(0)


# ---- 8 ----
def test_solid_insert(nt):
    k, m = 32, 4099
    seqs = threshold_input()
    d, offs = put(seqs)
    want, n_win = model(seqs, k, sm.CANONICAL, H, m)
    f = nt.CountingBloomFilter(m, H, k)
    f.insert(d, offs)
    mb, h2 = (1 << 16) + 3, 2  # another size and hash count than the counting filter's
    for c in (1, 2, 20, 255):
        passing = cm.solid_values(want, seqs, k, sm.CANONICAL, H, c)
        into = nt.BloomFilter(mb, h2, k)
        assert f.solid(d, offs, c, into) == passing.size and into.n_inserted == passing.size, c
        assert np.array_equal(into.bytes(), bm.image_of(bm.positions(passing, h2, k, mb), mb)), c
        assert padding_is_zero(into)
        if c == 1:
            plain = nt.BloomFilter(mb, h2, k)
            assert plain.insert(d, offs) == passing.size == n_win and np.array_equal(plain.bytes(), into.bytes())
        else:
            assert 0 < passing.size < n_win
    with pytest.raises(ValueError):
        f.solid(d, offs, 2, nt.BloomFilter(mb, h2, 31))


# ---- 9 ----
@pytest.mark.parametrize("m", [2**32 - 5, 2**32 + 15])
def test_hashes_with_exact_remainders(nt, m):
    """the adversarial values of test_bloom_gpu.test_remainder_is_exact, positions taken with Python integers"""
    k = 32
    rng = random.Random(m)
    h0 = adversarial(m, rng)
    h0 = np.concatenate([h0, h0[:100]])  # some values twice
    multi = bm.multihash(h0, H, k)
    pos = np.array([[int(x) % m for x in row] for row in multi.tolist()], dtype=np.int64)
    locs, incs = np.unique(pos.ravel(), return_counts=True)
    assert incs.max() < 255
    f = nt.CountingBloomFilter(m, H, k)
    f.insert_hashes(h0)
    got = f.filter[torch.from_numpy(locs).cuda()].cpu().numpy()
    assert np.array_equal(got, incs.astype(np.uint8))  # every counter the model touches
    hist = f.hist()
    want_hist = np.bincount(incs, minlength=256).astype(np.uint64)
    want_hist[0] = m - locs.size
    assert np.array_equal(hist, want_hist)  # and no other
    by_loc = dict(zip(locs.tolist(), incs.tolist()))
    want_counts = np.array([min(by_loc[p] for p in row) for row in pos.tolist()], dtype=np.uint8)
    assert np.array_equal(f.counts_of_hashes(h0), want_counts) and (want_counts >= 2).any()
    other = np.array([rng.getrandbits(64) for _ in range(512)], dtype=np.uint64)
    assert not f.counts_of_hashes(other).any()  # (about 12.8 k counters of 2^32 are set and the values are fixed: none of them is hit three times)
    assert f.counts_of_hashes(np.zeros(0, dtype=np.uint64)).size == 0


def test_hashes_on_a_small_filter(nt):
    m, k = 33, 32
    rng = random.Random(9)
    h0 = np.array([rng.getrandbits(64) for _ in range(500)], dtype=np.uint64)
    f = nt.CountingBloomFilter(m, H, k)
    f.insert_hashes(h0)
    want = cm.counters_of(h0, H, k, m)
    assert np.array_equal(f.counters(), want) and pad_is_zero(f) and int(want.max()) < 255
    f.insert_hashes(np.repeat(h0[:3], 200))
    want = cm.counters_of(np.repeat(h0[:3], 200), H, k, m, into=want)
    assert np.array_equal(f.counters(), want) and (want == 255).any() and (want < 255).any()
    other = np.array([rng.getrandbits(64) for _ in range(300)], dtype=np.uint64)
    assert np.array_equal(f.counts_of_hashes(other), cm.counts(want, other, H, k))


# ---- 10 ----
def test_add_hist_and_the_round_trip(nt, tmp_path):
    k, m = 32, 64
    seqs = saturation_input()
    long_a = seqs[0]
    shard_a, shard_b = (long_a[: len(long_a) // 2], seqs[1][:150]), (long_a[len(long_a) // 2:], seqs[1][150:])
    fa, fb = nt.CountingBloomFilter(m, H, k), nt.CountingBloomFilter(m, H, k)
    da, oa = put(shard_a)
    db, ob = put(shard_b)
    na, nb = fa.insert(da, oa), fb.insert(db, ob)
    wa, _ = model(shard_a, k, sm.CANONICAL, H, m)
    wb, _ = model(shard_b, k, sm.CANONICAL, H, m)
    assert np.array_equal(fa.counters(), wa) and np.array_equal(fb.counters(), wb)
    both = cm.merge(wa, wb)
    assert (both == 255).any() and (both < 255).any()
    fa.merge(fb)
    assert np.array_equal(fa.counters(), both) and np.array_equal(fb.counters(), wb) and pad_is_zero(fa)
    assert fa.n_inserted == na + nb
    # two counters below 255 whose sum is not: saturation in the add itself
    parts = ((b"A" * (k - 1 + 130),), (b"A" * (k - 1 + 140),))
    fs = []
    for part in parts:
        fs.append(nt.CountingBloomFilter(m, H, k))
        fs[-1].insert(*put(part))
    w0, w1 = model(parts[0], k, sm.CANONICAL, H, m)[0], model(parts[1], k, sm.CANONICAL, H, m)[0]
    assert int(w0.max()) < 255 and int(w1.max()) < 255 and (cm.merge(w0, w1) == 255).any()
    fs[0].merge(fs[1])
    assert np.array_equal(fs[0].counters(), cm.merge(w0, w1))
    with pytest.raises(ValueError):
        fa.merge(nt.CountingBloomFilter(m, H, 31))
    # hist, and the rates read from it
    hist = fa.hist()
    assert hist.dtype == np.uint64 and np.array_equal(hist, cm.hist(both)) and int(hist.sum()) == m
    assert fa.fpr(2) == (int((both >= 2).sum()) / m) ** H
    big = nt.CountingBloomFilter((1 << 20) + 1, H, k)
    d, offs = put(seqs)
    big.insert(d, offs)
    wbig, _ = model(seqs, k, sm.CANONICAL, H, (1 << 20) + 1)
    assert np.array_equal(big.hist(), cm.hist(wbig))
    # save / load
    path = tmp_path / "a.cbf"
    fa.save(path)
    raw = path.read_bytes()
    assert raw[:8] == b"NTCCB1\0\0" and raw[40:] == both.tobytes()
    back = nt.CountingBloomFilter.load(path)
    assert (back.m_bits, back.n_hash, back.k, back.strand, back.n_inserted) == (m, H, k, "canonical", na + nb)
    assert np.array_equal(back.counters(), both) and np.array_equal(back.hist(), hist)
    # a byte behind m is no part of the filter: hist refuses such an array
    odd = nt.CountingBloomFilter(33, H, k)
    odd.insert(d, offs)
    assert int(odd.hist().sum()) == 33
    odd.filter[odd.filter.numel() - 1] = 1
    with pytest.raises(nt.NtcError) as e:
        odd.hist()
    assert e.value.code == ERR_STATE and "behind" in str(e.value)
