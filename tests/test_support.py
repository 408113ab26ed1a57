"""tests/support.py carries the suite, so its statements are pinned on their own: ntComp against the oracle, the scalar form against the vectorised one,
the tiled layout against ntcard_amd.tile_reads, the row slots, the -g mask against the oracle's seed.  CPU only, small inputs."""
import functools
import random

import numpy as np
import pytest

import ntcard_amd as nt
import orc
import strand_model as sm
import support


@functools.lru_cache(maxsize=None)
def small_values(k):
    v = np.concatenate([orc.hash_read(r, k)[0] for r in support.small_reads()])
    v.setflags(write=False)
    return v


# dense sampling (sBits 2, 3): both of ntComp's samples fill up
@pytest.mark.parametrize("r_bits,s_bits", [(14, 7), (10, 2), (10, 3)])
def test_ntcomp_is_the_oracles(r_bits, s_bits):
    oc, of1 = orc.sketch_reads(support.small_reads(), [32], 0, r_bits, s_bits)
    assert oc[0, 0].any() and oc[0, 1].any() and of1[0] > 0  # the oracle alone: both samples occur
    tc, f1 = support.sketch_from_values([small_values(32)], r_bits, s_bits)
    assert tc.dtype == oc.dtype and np.array_equal(f1, of1) and np.array_equal(tc, oc)
    sample, _ = support.nt_comp(small_values(32), r_bits, s_bits)
    assert np.array_equal(support.sampled(small_values(32), s_bits), sample < 2) and int((sample < 2).sum()) == int(oc.sum())


def scalar_ntcomp(h, r_bits, s_bits):
    """ntcard.cpp:132-145 on a Python int, written out here on purpose: the second test overrides the first"""
    ind = None
    if h >> (63 - s_bits) == 1:
        ind = 0
    if h >> (64 - s_bits) == (1 << (s_bits - 1)) - 1:
        ind = 1
    return None if ind is None else ind * (1 << r_bits) + (h & ((1 << r_bits) - 1))


@pytest.mark.parametrize("s", [2, 7, 11, 24])
def test_scalar_key_is_the_vectorised_rule(s):
    r_bits = 14
    rng = random.Random(s)
    edges = [1 << (63 - s), (1 << (63 - s)) - 1, ((1 << (s - 1)) - 1) << (64 - s)]
    values = sorted({(e + d) & (2**64 - 1) for e in edges for d in (-1, 0, 1)} | {0, 2**64 - 1, (2 << (63 - s)) - 1, (1 << (s - 1)) << (64 - s)})
    values += [e | rng.getrandbits(63 - s) for e in edges for _ in range(20)] + [rng.getrandbits(64) for _ in range(200)]
    sample, index = support.nt_comp(np.array(values, dtype=np.uint64), r_bits, s)
    assert {0, 1, 2} <= set(sample.tolist())
    for h, sm_, ix in zip(values, sample.tolist(), index.tolist()):
        want = scalar_ntcomp(h, r_bits, s)
        assert support.key_of(h, r_bits, s) == want, hex(h)
        assert (None if sm_ == 2 else (sm_ << r_bits) + ix) == want, hex(h)
        assert bool(support.sampled(h, s)) == (want is not None)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 150])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_tile_array_is_tile_reads(n, L):
    rng = np.random.default_rng(1000 * n + L)
    arr = support.random_reads(rng, n, L, 0.02)
    rows = [arr[i].tobytes() for i in range(n)]
    want = nt.tile_reads(rows, L)
    assert want.size == nt.tiled_bytes(n, L)
    assert np.array_equal(support.tile_array(arr), want)
    assert np.array_equal(support.tile(rows, L), want)
    # the slots behind the batch's last read hold `unused`; nothing that belongs to a read moves.  owner: 1 in every read's row, 'A' elsewhere
    owner = support.tile_array(np.ones((n, (L + 15) // 16 * 16), dtype=np.uint8)) == 1
    other = support.tile(rows, L, unused=0x23)
    assert np.array_equal(other[owner], want[owner]) and np.all(other[~owner] == 0x23) and np.all(want[~owner] == ord("A"))
    assert int(owner.sum()) == n * ((L + 15) // 16 * 16)


def test_tile_pads_a_shorter_read_with_a_base():
    rows = [b"ACGTACGTACGTACGTAC", b"CCC", b""]
    t = support.tile(rows, 18, unused=0x23).reshape(1, 2, 2048, 16)
    assert t[0, 0, 0].tobytes() == rows[0][:16] and t[0, 1, 0].tobytes() == b"AC" + b"A" * 14
    assert t[0, 0, 1].tobytes() == b"CCC" + b"A" * 13 and t[0, 1, 1].tobytes() == b"A" * 16 == t[0, 0, 2].tobytes()
    assert np.all(t[0, :, 3:] == 0x23)


@pytest.mark.parametrize("n,chunks", [(1, 1), (2047, 3), (2049, 7), (5000, 10)])
def test_tile_ragged_is_tile_reads_ragged(n, chunks):
    rng = np.random.default_rng(n + chunks)
    full = support.random_reads(rng, n, 16 * chunks, 0.02)
    lens = rng.integers(16 * chunks - 15, 16 * chunks + 1, size=n)
    reads = [full[i, :lens[i]].tobytes() for i in range(n)]
    tiles, tails = support.tile_ragged(reads, chunks)
    want_tiles, want_tails, _ = nt.tile_reads_ragged(reads, chunks)
    assert tails.dtype == np.uint32 and np.array_equal(tails, want_tails) and np.array_equal(tiles, want_tiles)
    assert int(tails[:, 0].sum()) == n and np.all(np.diff(tails.astype(np.int64), axis=1) <= 0)


def test_spans_round_trip():
    reads = [b"ACGT", b"", b"N", b"ACGTACGTA"]
    buf, starts, lens = support.spans_of(reads, lead=2, gap=1)
    assert starts.dtype == np.uint64 and lens.dtype == np.uint32 and starts.tolist() == [2, 7, 8, 10] and lens.tolist() == [4, 0, 1, 9]
    assert [buf[s:s + n].tobytes() for s, n in zip(starts.tolist(), lens.tolist())] == reads
    assert buf.tobytes() == b"##ACGT##N#ACGTACGTA#"


def test_row_slots_round_trip():
    rng = random.Random(4)
    reads = [support.rseq(rng, n, pn=0.1) for n in (0, 1, 7, 8, 150, 151, 152)]
    for stride, fill, tail in ((152, ord("A"), 16), (156, 10, 16), (200, 0, 0)):
        buf = support.to_slots(reads, stride, fill=fill, tail=tail)
        assert buf.dtype == np.uint8 and buf.size == len(reads) * stride + tail
        for i, r in enumerate(reads):
            assert buf[i * stride: i * stride + len(r)].tobytes() == r
            assert np.all(buf[i * stride + len(r): (i + 1) * stride] == fill)
        assert np.all(buf[len(reads) * stride:] == fill)
    assert np.array_equal(support.to_slots(reads, 152), support.to_slots(reads, 152, fill=65, tail=16))


def test_offsets():
    seqs = [b"", b"ACG", b"T", b""]
    assert support.offsets_of(seqs).tolist() == [0, 0, 3, 4, 4] and support.offsets_of(seqs).dtype == np.uint64
    assert support.offsets_of(seqs, 3).tolist() == [3, 3, 6, 7, 7]
    assert np.array_equal(support.offsets_of([len(s) for s in seqs], 3), support.offsets_of(seqs, 3))
    assert np.array_equal(support.offsets_of(np.array([0, 3, 1, 0])), support.offsets_of(seqs))
    assert support.offsets_of([]).tolist() == [0]


@pytest.mark.parametrize("k,gap", [(12, 2), (32, 8)])
def test_gap_mask_is_the_seed_ntcard_derives(k, gap):
    """ntcard.cpp:407-413 as the oracle restates it (orc_gap_positions): the don't-care positions of the one -g seed"""
    m = support.gap_mask(k, gap)
    assert len(m) == k and [i for i, c in enumerate(m) if c == "0"] == orc.gap_positions(k, gap).tolist()
    assert m == "1" * ((k - gap) // 2) + "0" * gap + "1" * ((k - gap) // 2)  # (k - gap even: the halves are equal)
    assert [m] == next(c[1] for c in sm.SKETCH_CONFIGS if c[0] == "gap%d_%d" % (k, gap))
    assert support.gap_mask(k, 0) == "1" * k


def test_generators_draw_as_they_always_did():
    """the first bytes of the fixed-seed read sets the GPU tests are built on (a changed draw order would move every pinned figure at once)"""
    assert support.rseq(random.Random(21), 12, pn=0.3) == b"YTTU-N-CCATA"
    assert support.rseq_acgt(random.Random(7), 12) == b"GCTAAAGACAAT"
    assert support.random_reads(np.random.default_rng(1), 2, 8, 0.3).tobytes() == b"C*TTAATTKCU*CnCC"
    assert len(support.small_reads()) == 5000 and support.small_reads()[0][:12] == b"CTTCTAGATNTA"
