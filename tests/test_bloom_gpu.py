"""GPU tests of the Bloom filters (include/ntcard_hip.h: ntc_bloom_*_device; ntcard_amd/bloom.py): the filter a build leaves is BYTE for byte the image of
tests/bloom_model.py — the oracle's windows and multi-hash, positions % m, the reference's bit rule — for every k class, strand and hash count, across the
seams of the block grid, at every alignment of the source; inserts are idempotent and commute with OR; the remainder by m_bits is exact on adversarial
values up to a 1 GiB filter; the popcount counts the first m_bits bits only; a query counts per sequence what the model's membership test counts, false
positives included."""
import functools
import random

import numpy as np
import pytest

import bloom_model as bm
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401  (nt: the fixture)
from support import offsets_of, rand_seq

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 4096  # NTC_BLOOM_BLOCK (asserted below)
M = (1 << 20) + 7
STRANDS = ["canonical", "forward", "reverse"]


@functools.lru_cache(maxsize=None)
def mixed_seqs(k, seed=11, n=295):
    """about 300 sequences: the lengths 0, 1, k - 1, k, k + 1, then 100 .. 400, a non-base letter here and there"""
    rng = random.Random(seed * 1000 + k)
    lens = [0, 1, k - 1, k, k + 1] + [rng.randint(100, 400) for _ in range(n)]
    return tuple(rand_seq(rng, L, pn=rng.choice([0.0, 0.0, 0.01])) for L in lens)


@functools.lru_cache(maxsize=None)
def model_values(seqs, k, strand):
    vals = bm.h0_values(list(seqs), k, strand)
    return np.concatenate(vals) if vals else np.zeros(0, dtype=np.uint64)


def model_image(seqs, k, strand, n_hash, m):
    v = model_values(tuple(seqs), k, strand)
    return bm.image_of(bm.positions(v, n_hash, k, m), m), int(v.size)


def put(seqs, lead=0):
    """the sequences behind one another on the device, `lead` bytes of '#' in front -> (tensor, host offsets)"""
    host = np.frombuffer(b"#" * lead + b"".join(seqs) + b"#", dtype=np.uint8).copy()
    return dev(host), offsets_of(list(seqs), lead)


def padding_is_zero(f):
    """the bits from m_bits on, up to the end of the filter's tensor"""
    raw = f.filter.cpu().numpy()
    tail = np.unpackbits(raw)[f.m_bits:]
    return not tail.any()


def test_block_constant(nt):
    assert nt.BLOOM_BLOCK == B


@pytest.mark.parametrize("strand", STRANDS)
@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 64, 65, 127])
def test_image_is_the_models_byte_for_byte(nt, k, strand):
    seqs = mixed_seqs(k)
    d, offs = put(seqs)
    for n_hash in (1, 3, 8, 32):
        want, n_win = model_image(seqs, k, sm.STRANDS[strand], n_hash, M)
        f = nt.BloomFilter(M, n_hash, k, strand)
        assert f.insert(d, offs) == n_win and n_win > 0
        assert np.array_equal(f.bytes(), want), (k, strand, n_hash)
        assert padding_is_zero(f)


def seam_layouts(k, rng):
    """name -> sequences whose boundaries, non-base letters and empty runs sit on the seams of the block grid (offsets[0] = 0 at a 16-byte boundary)"""
    out = {}
    for d in (-1, 0, 1):
        seqs = [rand_seq(rng, B + d), rand_seq(rng, B)]  # boundaries at byte B + d and 2 B + d
        seqs.append(rand_seq(rng, 2 * B + 200))           # one sequence over three blocks
        total = sum(map(len, seqs))
        seqs.append(rand_seq(rng, 5 * B - total))         # up to the seam at 5 B
        seqs += [rand_seq(rng, k - 1) for _ in range(B // max(k - 1, 1) + 2)]  # block 5 holds only sequences shorter than k
        total = sum(map(len, seqs))
        seqs.append(rand_seq(rng, 7 * B - total))         # up to the seam at 7 B
        assert sum(map(len, seqs)) == 7 * B and 5 * B + B + k - 1 <= sum(map(len, seqs[:-1]))
        seqs += [b""] * 70                                # 70 empty sequences at the seam
        seqs.append(rand_seq(rng, 300))
        out[f"boundary{d:+d}"] = seqs
    for name, at in (("N@B-1", B - 1), ("N@B", B), ("N@B+1", B + 1), ("N@B+k-2", B + k - 2), ("N@2B+k-1", 2 * B + k - 1)):
        s = bytearray(rand_seq(rng, 3 * B + 50))
        s[at] = ord("N")
        out[name] = [bytes(s)]
    return out


@pytest.mark.parametrize("k", [32, 127])
def test_block_seams(nt, k):
    for name, seqs in seam_layouts(k, random.Random(k)).items():
        assert sum(map(len, seqs)) > 3 * B
        d, offs = put(seqs)
        assert d.data_ptr() % 16 == 0
        want, n_win = model_image(seqs, k, sm.CANONICAL, 3, M)
        f = nt.BloomFilter(M, 3, k)
        assert f.insert(d, offs) == n_win, name
        assert np.array_equal(f.bytes(), want), name
        # the same seams under the query's per-sequence sums: a smaller filter of the same input, so that misses and false positives both occur
        g = nt.BloomFilter(4093, 2, k)
        half = [s for i, s in enumerate(seqs) if i % 2 == 0]
        dh, oh = put(half)
        g.insert(dh, oh)
        img, _ = model_image(half, k, sm.CANONICAL, 2, 4093)
        assert np.array_equal(g.bytes(), img), name
        w, h = g.query(d, offs)
        mw, mh = bm.query(img, seqs, k, sm.CANONICAL, 2, 4093)
        assert np.array_equal(w, mw) and np.array_equal(h, mh), name


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 7, 15])
def test_any_alignment_and_first_offset(nt, lead):
    """d_bases at byte offsets 0 .. 3 (and 7, 15) from a 16-byte boundary, offsets[0] = 5: the same image"""
    k = 32
    seqs = mixed_seqs(k)
    want, n_win = model_image(seqs, k, sm.CANONICAL, 3, M)
    host = np.frombuffer(b"#" * (lead + 5) + b"".join(seqs) + b"#", dtype=np.uint8).copy()
    d = dev(host)[lead:]
    assert d.data_ptr() % 16 == lead
    offs = offsets_of(list(seqs), 5)
    assert int(offs[0]) == 5
    f = nt.BloomFilter(M, 3, k)
    assert f.insert(d, offs) == n_win and np.array_equal(f.bytes(), want)
    w, h = f.query(d, offs)
    mw, _ = bm.query(want, seqs, k, sm.CANONICAL, 3, M)
    assert np.array_equal(w, mw) and np.array_equal(h, w)


def test_idempotence_union_and_or(nt, tmp_path):
    k, n_hash = 32, 3
    a, b = mixed_seqs(k, seed=21, n=120), mixed_seqs(k, seed=22, n=120)
    da, oa = put(a)
    db, ob = put(b)
    img_a, na = model_image(a, k, sm.CANONICAL, n_hash, M)
    img_b, nb = model_image(b, k, sm.CANONICAL, n_hash, M)
    both = img_a | img_b
    assert not np.array_equal(both, img_a) and not np.array_equal(both, img_b)
    f = nt.BloomFilter(M, n_hash, k)
    assert f.insert(da, oa) == na
    assert f.insert(da, oa) == na and np.array_equal(f.bytes(), img_a)  # the second pass finds every bit set: loads only
    assert f.insert(db, ob) == nb and np.array_equal(f.bytes(), both)
    assert f.n_inserted == 2 * na + nb
    g, h = nt.BloomFilter(M, n_hash, k), nt.BloomFilter(M, n_hash, k)
    g.insert(da, oa)
    h.insert(db, ob)
    g.merge(h)
    assert np.array_equal(g.bytes(), both) and np.array_equal(h.bytes(), img_b) and padding_is_zero(g)
    with pytest.raises(ValueError):
        g.merge(nt.BloomFilter(M, n_hash, 31))
    # save / load: the file's bytes behind the header are the image
    path = tmp_path / "g.bf"
    g.save(path)
    assert path.read_bytes()[40:] == both.tobytes()
    back = nt.BloomFilter.load(path)
    assert (back.m_bits, back.n_hash, back.k, back.strand, back.n_inserted) == (M, n_hash, k, "canonical", na + nb)
    assert np.array_equal(back.bytes(), both) and back.popcount() == bm.popcount(both)


def adversarial(m, rng):
    top = (2**64 - 1) // m
    vals = [0, 1, m - 1, m, m + 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1] + [(top - i) * m for i in range(64)]
    vals += [rng.getrandbits(64) for _ in range(4096)]
    return np.array([v & (2**64 - 1) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 31, 32, 33, 1 << 20, (1 << 20) + 7, 2**32 - 5, 2**32 + 15, 2**33 + 9])
def test_remainder_is_exact(nt, m):
    """h % m by mask or by multiply-high, driven without hashing: n_hash = 1 puts h_0 itself through the remainder, n_hash = 3 the multi-hashes too"""
    rng = random.Random(m)
    h0 = adversarial(m, rng)
    for n_hash in (1, 3):
        pos = bm.positions(h0, n_hash, 32, m)
        assert pos[:, 0].tolist() == [int(x) % m for x in h0]
        f = nt.BloomFilter(m, n_hash, 32)
        f.insert_hashes(h0)
        if m <= (1 << 20) + 7:
            assert np.array_equal(f.bytes(), bm.image_of(pos, m)), (m, n_hash)
        else:  # two checks that together are identity: no bit beyond the model's, and every bit of the model's
            assert f.popcount() == np.unique(pos).size
            idx = torch.from_numpy((pos.ravel() >> np.uint64(3)).astype(np.int64)).cuda()
            got = f.filter[idx].cpu().numpy()
            assert ((got & (0x80 >> (pos.ravel() & np.uint64(7)).astype(np.int64)).astype(np.uint8)) != 0).all()
        assert padding_is_zero(f) if m <= 1 << 21 else True
        assert f.query_hashes(h0).all()
        other = np.array([rng.getrandbits(64) for _ in range(512)], dtype=np.uint64)
        if m <= (1 << 20) + 7:
            want = bm.bits_set(bm.image_of(pos, m), bm.positions(other, n_hash, 32, m)).all(axis=1)
            assert np.array_equal(f.query_hashes(other), want)
        else:
            assert not f.query_hashes(other).any()  # (at most 12.5 k bits of 2^32 are set and the values are fixed: no false positive among them)
        del f
    assert nt.BloomFilter(m, 1, 32).query_hashes(np.zeros(0, dtype=np.uint64)).size == 0


@pytest.mark.parametrize("m", [9, (1 << 20) + 7])
def test_popcount_counts_the_first_m_bits(nt, m):
    rng = random.Random(m + 1)
    h0 = np.array([rng.getrandbits(64) for _ in range(3000)] + list(range(m if m < 100 else 100)), dtype=np.uint64)
    f = nt.BloomFilter(m, 3, 32)
    assert f.popcount() == 0 and f.fpr() == 0.0
    f.insert_hashes(h0)
    img = bm.image_of(bm.positions(h0, 3, 32, m), m)
    pop = bm.popcount(img)
    assert f.popcount() == pop and 0 < pop <= m and padding_is_zero(f)
    assert f.fpr() == (pop / m) ** 3
    if m == 9:
        assert pop == 9  # every position 0 .. 8 went in: a full filter, and still nothing behind bit 8
    # a bit behind m_bits is no part of the filter: the popcount refuses to count such an array
    f.filter[f.filter.numel() - 1] |= 1
    with pytest.raises(nt.NtcError) as e:
        f.popcount()
    assert e.value.code == -4 and "behind" in str(e.value)


def test_query_counts_what_the_model_counts(nt):
    """m = 4093 with two hashes: the filter is nearly full, so false positives certainly occur — and the model, which tests the same bits, counts the same ones"""
    k, n_hash, m = 32, 2, 4093
    ins, rest = mixed_seqs(k, seed=31, n=20), mixed_seqs(k, seed=32, n=150)
    d, offs = put(ins)
    for strand in STRANDS:
        f = nt.BloomFilter(m, n_hash, k, strand)
        f.insert(d, offs)
        img, _ = model_image(ins, k, sm.STRANDS[strand], n_hash, m)
        assert np.array_equal(f.bytes(), img)
        w, h = f.query(d, offs)  # what was inserted is found
        mw, mh = bm.query(img, ins, k, sm.STRANDS[strand], n_hash, m)
        assert np.array_equal(w, mw) and np.array_equal(h, w) and np.array_equal(mh, mw)
        dq, oq = put(rest, lead=3)
        w, h = f.query(dq, oq)
        mw, mh = bm.query(img, rest, k, sm.STRANDS[strand], n_hash, m)
        assert np.array_equal(w, mw) and np.array_equal(h, mh)
        assert 0 < int(mh.sum()) < int(mw.sum())  # false positives and misses both occur
        assert w.dtype == np.uint32 and w.shape == (len(rest),)


def test_query_of_many_short_sequences(nt):
    """more than 2^16 sequences of length k: one window each; and sequences of one base under k = 1, thousands per block — more than a workgroup's table
    of sums in LDS holds"""
    k = 32
    rng = np.random.default_rng(5)
    n = (1 << 16) + 1234
    arr = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, k))]
    d = dev(np.concatenate([arr.ravel(), np.zeros(1, dtype=np.uint8)]))
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
    f = nt.BloomFilter(1 << 24, 3, k)
    assert f.insert(d, offs) == n
    w, h = f.query(d, offs)
    assert (w == 1).all() and (h == 1).all()
    fs, rs, ok = sm.array_window_values(arr, "1" * k)
    assert ok.all() and np.array_equal(f.bytes(), bm.image_of(bm.positions(np.minimum(fs, rs).ravel(), 3, k, 1 << 24), 1 << 24))
    # k = 1
    prng = random.Random(6)
    seqs = [rand_seq(prng, prng.choice([0, 1, 1, 1, 1, 2]), pn=0.1) for _ in range(3 * B)]
    d1, o1 = put(seqs)
    g = nt.BloomFilter(64, 1, 1)
    g.insert_hashes(bm.h0_values([b"A"], 1)[0])  # A, T and U of either case share this value; C and G do not
    img = g.bytes()
    w, h = g.query(d1, o1)
    mw, mh = bm.query(img, seqs, 1, sm.CANONICAL, 1, 64)
    assert np.array_equal(w, mw) and np.array_equal(h, mh) and 0 < int(mh.sum()) < int(mw.sum())
