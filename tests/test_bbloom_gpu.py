"""GPU tests of the blocked Bloom filters (include/ntcard_hip.h: ntc_bbloom_*_device; ntcard_amd/bloom.py: BlockedBloomFilter): the filter is BYTE for
byte the image of tests/bbloom_model.py — block = h_0 mod n_blocks, four 9-bit positions from the top of each multi-hash value, the reference's bit rule
— for given values and for the walk over reads, up to bit indices beyond 2^32; inserts are idempotent and commute with the plain filter's OR, whose
popcount counts a blocked image too; the block histogram and the solid insert are the model's; nothing outside the filter's bytes is written."""
import functools
import random

import numpy as np
import pytest

import bbloom_model as bb
import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401  (nt: the fixture)
from support import offsets_of, rand_seq

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 4096  # NTC_BLOOM_BLOCK: the window starts of one workgroup
STRANDS = ["canonical", "forward", "reverse"]
GUARD = 256  # bytes in front of and behind a guarded filter


def guarded(nt, m_bits, n_hash, k, strand="canonical", shift=0):
    """a BlockedBloomFilter whose bytes lie inside a larger zeroed tensor, GUARD + shift bytes from its start (shift 4: 4-byte but not 16-byte aligned)
    -> (filter, the whole tensor)"""
    f = nt.BlockedBloomFilter(m_bits, n_hash, k, strand)
    whole = torch.zeros(GUARD + shift + f.n_bytes + GUARD, dtype=torch.uint8, device="cuda")
    f.filter = whole[GUARD + shift: GUARD + shift + f.n_bytes]
    assert f.filter.data_ptr() % 16 == shift
    return f, whole


def guards_are_zero(f, whole):
    raw = whole.cpu().numpy()
    lo = f.filter.data_ptr() - whole.data_ptr()
    return not raw[:lo].any() and not raw[lo + f.n_bytes:].any()


def put(seqs, lead=0, first=0):
    """the sequences behind one another on the device, `lead` bytes in front of a 16-byte boundary and `first` more in front of the first sequence
    -> (tensor whose address is `lead` behind a 16-byte boundary, host offsets that start at `first`)"""
    host = np.frombuffer(b"#" * (lead + first) + b"".join(seqs) + b"#", dtype=np.uint8).copy()
    d = dev(host)[lead:]
    assert d.data_ptr() % 16 == lead
    return d, offsets_of(list(seqs), first)


def test_constants(nt):
    assert nt.BLOOM_BLOCK == B and nt.BBLOOM_BLOCK_BITS == bb.BLOCK == 512


# ---- the hash tools ----
def adversarial(n_blocks, rng):
    """tests/test_bloom_gpu.py's values for the remainder, by n_blocks: 0, 2^64 - 1, the values around n_blocks and around every one of the last 64
    multiples of n_blocks below 2^64, and 5000 random ones"""
    top = (2**64 - 1) // n_blocks
    vals = [0, 1, n_blocks - 1, n_blocks, n_blocks + 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]
    for i in range(64):
        vals += [(top - i) * n_blocks - 1, (top - i) * n_blocks, (top - i) * n_blocks + 1]
    vals += [rng.getrandbits(64) for _ in range(5000)]
    return np.array([v & (2**64 - 1) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("n_hash", [1, 3, 4, 5, 8, 9, 32])
@pytest.mark.parametrize("n_blocks", [1, 3, 8, 1000])
def test_hash_tools_give_the_models_image_and_flags(nt, n_blocks, n_hash):
    m = 512 * n_blocks
    rng = random.Random(1000 * n_blocks + n_hash)
    h0 = adversarial(n_blocks, rng)
    other = np.array([rng.getrandbits(64) for _ in range(2048)], dtype=np.uint64)
    one = np.full(4096, rng.getrandbits(64), dtype=np.uint64)  # every lane contends for the same dwords
    for k in (12, 32, 600):
        want = bb.image_of(h0, n_hash, k, m)
        f, whole = guarded(nt, m, n_hash, k)
        f.insert_hashes(h0)
        assert np.array_equal(f.bytes(), want), (k, "image")
        assert f.query_hashes(h0).all()
        assert np.array_equal(f.query_hashes(other), bb.test_values(want, other, n_hash, k, m)), (k, "flags")
        f.insert_hashes(one)
        want = bb.image_of(one[:1], n_hash, k, m, into=want)
        assert np.array_equal(f.bytes(), want), (k, "one value 4096 times")
        assert guards_are_zero(f, whole) and f.n_inserted == h0.size + one.size
        g, gw = guarded(nt, m, n_hash, k)
        g.insert_hashes(one)  # into an empty filter: all 4096 lanes find the bits clear
        assert np.array_equal(g.bytes(), bb.image_of(one[:1], n_hash, k, m)) and guards_are_zero(g, gw)
        assert np.array_equal(g.query_hashes(other), bb.test_values(g.bytes(), other, n_hash, k, m))
    if n_blocks == 1000:  # at this size the filter is sparse enough for both answers to occur
        flags = bb.test_values(want, other, n_hash, 600, m)
        assert not flags.all()
    assert nt.BlockedBloomFilter(m, n_hash, 32).query_hashes(np.zeros(0, dtype=np.uint64)).size == 0


def test_bit_indices_beyond_32_bits(nt):
    """2^32 + 3 * 512 bits (512 MiB), n_blocks = 2^23 + 3: values whose blocks are the first, 2^23 - 2, 2^23 - 1 and the last three — 2^23, 2^23 + 1,
    2^23 + 2, whose bits lie at 2^32 and beyond.  Those six blocks are compared with the model byte for byte, the rest through the popcount."""
    m = 2**32 + 3 * 512
    n_blocks, n_hash, k = m // 512, 8, 32
    blocks = [0, 2**23 - 2, 2**23 - 1, 2**23, 2**23 + 1, 2**23 + 2]
    assert blocks[-1] == n_blocks - 1
    rng = random.Random(23)
    vals = []
    for b in blocks:
        for _ in range(40):
            q = rng.randrange(0, (2**64 - 1 - b) // n_blocks + 1)  # any value of that block
            vals.append(q * n_blocks + b)
    vals += [(2**64 - 1) // n_blocks * n_blocks - 1]  # the last whole multiple below 2^64, less one: the last block
    h0 = np.array(vals, dtype=np.uint64)
    pos = bb.positions(h0, n_hash, k, m)
    assert sorted(set((pos[:, 0] // np.uint64(512)).tolist())) == blocks and int(pos.max()) >= 2**32 + 2 * 512
    f = nt.BlockedBloomFilter(m, n_hash, k)
    f.insert_hashes(h0)
    assert f.popcount() == np.unique(pos).size
    for b in blocks:
        got = f.filter[64 * b: 64 * b + 64].cpu().numpy()
        mine = pos[(pos[:, 0] // np.uint64(512)) == np.uint64(b)] - np.uint64(512 * b)
        assert np.array_equal(got, bm.image_of(mine, 512)), b
    assert f.query_hashes(h0).all()
    other = np.array([q * n_blocks + b for b in blocks for q in (5, 6, 7)], dtype=np.uint64)  # the same blocks, other positions
    want = np.array([np.isin(bb.positions(other[i:i + 1], n_hash, k, m), pos).all() for i in range(other.size)])
    assert np.array_equal(f.query_hashes(other), want) and not want.all()
    hist = f.block_hist()
    assert int(hist.sum()) == n_blocks and int(hist[0]) == n_blocks - len(blocks)
    del f


# ---- the walk ----
@functools.lru_cache(maxsize=None)
def walk_reads(k):
    """more than 3 * 4096 windows: runs of N, empty sequences, sequences shorter than k, one sequence over three blocks of window starts, and a sequence
    that starts exactly on the seam at B window starts"""
    rng = random.Random(500 + k)
    with_n = bytearray(rand_seq(rng, B - 100))
    with_n[700:700 + 2 * k + 5] = b"N" * (2 * k + 5)
    with_n[1500:1501] = b"n"
    seqs = [bytes(with_n), rand_seq(rng, 100)]  # the next sequence starts at byte B
    assert sum(map(len, seqs)) == B
    seqs += [rand_seq(rng, 2 * B + 300, pn=0.001), b"", b"", rand_seq(rng, max(k - 1, 0)), rand_seq(rng, k), rand_seq(rng, k + 1)]
    seqs += [rand_seq(rng, rng.randint(100, 400), pn=rng.choice([0.0, 0.01])) for _ in range(40)]
    seqs += [b"", rand_seq(rng, 1), rand_seq(rng, 333)]
    return tuple(seqs)


@pytest.mark.parametrize("strand", STRANDS)
@pytest.mark.parametrize("k", [1, 32, 127])
def test_walk_inserts_and_queries_what_the_model_does(nt, k, strand):
    seqs = walk_reads(k)
    st = sm.STRANDS[strand]
    vals = bm.h0_values(list(seqs), k, st)
    assert sum(v.size for v in vals) >= 3 * B
    ins = [s for i, s in enumerate(seqs) if i % 2 == 0]  # every second sequence goes in, all are asked for
    ins_vals = np.concatenate(bm.h0_values(ins, k, st))
    for lead, first in ((0, 5), (7, 3)):  # the walk's source lead: the address of the first base modulo 16; the first offset is not 0
        d_ins, o_ins = put(ins, (lead - first) % 16, first)
        d_all, o_all = put(seqs, (lead - first) % 16, first)
        assert int(o_all[0]) == first != 0 and (d_all.data_ptr() + first) % 16 == lead
        for n_blocks, n_hash in ((64, 3), (1, 3), (64, 8)):
            m = 512 * n_blocks
            want = bb.image_of(ins_vals, n_hash, k, m)
            f, whole = guarded(nt, m, n_hash, k, strand)
            assert f.insert(d_ins, o_ins) == ins_vals.size
            assert np.array_equal(f.bytes(), want), (lead, n_blocks, n_hash)
            w, h = f.query(d_all, o_all)
            mw, mh = bb.query(want, seqs, k, st, n_hash, m)
            assert np.array_equal(w, mw) and np.array_equal(h, mh), (lead, n_blocks, n_hash)
            assert int(mw.sum()) >= 3 * B and guards_are_zero(f, whole)
            if n_blocks == 64 and n_hash == 3 and k > 1:
                # the fill is one at which the MODEL shows false positives and misses among the queried windows (k = 1 has four k-mers: no such fill)
                allv = np.concatenate(vals)
                hit, known = bb.test_values(want, allv, n_hash, k, m), np.isin(allv, ins_vals)
                assert (hit & ~known).any() and (~hit).any() and hit[known].all()


def test_twice_halves_popcount_and_file(nt, tmp_path):
    k, n_hash, m = 32, 3, 1000 * 512
    seqs = walk_reads(k)
    a, b = seqs[:len(seqs) // 2], seqs[len(seqs) // 2:]
    d, o = put(seqs)
    da, oa = put(a)
    db, ob = put(b)
    want, n_all = bb.build(seqs, k, sm.CANONICAL, n_hash, m)
    img_a, na = bb.build(a, k, sm.CANONICAL, n_hash, m)
    img_b, nb = bb.build(b, k, sm.CANONICAL, n_hash, m)
    assert np.array_equal(img_a | img_b, want) and not np.array_equal(img_a, want) and not np.array_equal(img_b, want)
    f = nt.BlockedBloomFilter(m, n_hash, k)
    assert f.insert(d, o) == n_all and np.array_equal(f.bytes(), want)
    assert f.insert(d, o) == n_all and np.array_equal(f.bytes(), want)  # the second pass finds every bit set: loads only
    assert f.n_inserted == 2 * n_all
    g, h = nt.BlockedBloomFilter(m, n_hash, k), nt.BlockedBloomFilter(m, n_hash, k)
    assert g.insert(da, oa) == na and h.insert(db, ob) == nb
    g.merge(h)  # ntc_bloom_or_device, unchanged
    assert np.array_equal(g.bytes(), want) and np.array_equal(h.bytes(), img_b)
    assert g.popcount() == bm.popcount(want) == f.popcount()  # ntc_bloom_popcount_device, unchanged
    assert g.fpr() == pytest.approx(bb.realised_fpr(want, n_hash), rel=1e-12)
    with pytest.raises(ValueError):
        g.merge(nt.BlockedBloomFilter(m, n_hash, 31))
    with pytest.raises(ValueError):
        g.merge(nt.BloomFilter(m, n_hash, k))
    path = tmp_path / "g.bbf"
    g.write(path)
    raw = path.read_bytes()
    assert raw[:8] == b"NTCBB1\0\0" and raw[40:] == want.tobytes()
    back = nt.BlockedBloomFilter.read(path)
    assert (back.m_bits, back.n_hash, back.k, back.strand, back.n_inserted) == (m, n_hash, k, "canonical", na + nb)
    assert np.array_equal(back.bytes(), want)
    w, hh = back.query(d, o)
    assert np.array_equal(w, hh) and int(w.sum()) == n_all


@pytest.mark.parametrize("shift", [0, 4])
def test_block_histogram(nt, shift):
    """a zeroed filter, a part-filled one and one with every bit of some blocks set; at 16-byte alignment (16-byte loads) and off it (dword loads)"""
    n_blocks, n_hash, k = 3000, 3, 32  # more blocks than one workgroup has lanes
    m = 512 * n_blocks
    f, whole = guarded(nt, m, n_hash, k, shift=shift)
    hist = f.block_hist()
    assert hist.dtype == np.uint64 and hist.size == 513 and int(hist[0]) == n_blocks and int(hist.sum()) == n_blocks and f.fpr() == 0.0
    rng = np.random.default_rng(9)
    h0 = rng.integers(0, 2**64, size=40_000, dtype=np.uint64)
    h0 = h0[(h0 % np.uint64(n_blocks)) % np.uint64(3) != 0]  # a third of the blocks stays empty
    f.insert_hashes(h0)
    img = f.bytes()
    assert np.array_equal(img, bb.image_of(h0, n_hash, k, m))
    want = bb.block_hist(img)
    assert np.array_equal(f.block_hist(), want) and int(want[0]) == n_blocks // 3 and (want[1:] != 0).sum() > 10
    assert f.fpr() == pytest.approx(bb.realised_fpr(img, n_hash), rel=1e-12)
    full = [0, 1, 777, n_blocks - 1]
    for b in full:
        f.filter[64 * b: 64 * b + 64] = 0xFF
    f.filter[64 * 5: 64 * 5 + 64] = 0xFF
    f.filter[64 * 5] = 0x7F  # 511 bits
    img = f.bytes()
    want = bb.block_hist(img)
    got = f.block_hist()
    assert np.array_equal(got, want) and int(got[512]) == len(full) and int(got[511]) >= 1 and int(got.sum()) == n_blocks
    assert guards_are_zero(f, whole)


@pytest.mark.parametrize("min_count", [1, 2, 255])
def test_solid_insert_into_a_blocked_filter(nt, min_count):
    """cbloom_model's counters, then the blocked image of the windows whose count passes; a k-mer that occurs 300 times reaches 255"""
    k, c_hash, c_m = 32, 3, (1 << 16) + 7
    rng = random.Random(77)
    base = [rand_seq(rng, rng.randint(60, 300), pn=0.005) for _ in range(60)]
    seqs = base + base[:25] + [b"A" * (300 + k - 1), b"", rand_seq(rng, k - 1)] + base[:5]
    cnt, n_win = cm.counters(seqs, k, sm.CANONICAL, c_hash, c_m)
    solid = cm.solid_values(cnt, seqs, k, sm.CANONICAL, c_hash, min_count)
    assert 0 < solid.size < n_win if min_count > 1 else solid.size == n_win
    d, o = put(seqs, lead=3, first=2)
    cbf = nt.CountingBloomFilter(c_m, c_hash, k)
    assert cbf.insert(d, o) == n_win and np.array_equal(cbf.counters(), cnt)
    for n_blocks, n_hash in ((64, 3), (1, 5)):
        m = 512 * n_blocks
        f, whole = guarded(nt, m, n_hash, k)
        assert f.insert_solid(cbf, d, o, min_count) == solid.size
        assert np.array_equal(f.bytes(), bb.image_of(solid, n_hash, k, m)) and guards_are_zero(f, whole)
        assert f.n_inserted == solid.size
    assert np.array_equal(cbf.counters(), cnt)  # the counting filter is only read
