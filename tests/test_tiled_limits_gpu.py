"""GPU tests of the tiled kernels K1h + K1f (ntc_sketch_k1h.hip, gen_k1h.py) at the read lengths the API declares and the rest of the suite never
reaches: equal-length batches of 1009 .. 65535 bases (ntc_submit_tiled_device takes 1 .. 65535), ragged batches of 257 and 4095 chunks
(ntc_submit_tiled_ragged_device takes 1 .. 4095), and one launch over bins of both extremes.  Every comparison is exact: t_Counter and F1 against
tests/orc.py (a forward-strand engine: against tests/limits_model.py's vectorised form of tests/strand_model.py, pinned in tests/test_limits_host.py).

What these lengths reach and 150 bp reads do not: the 12-bit chunk field of K1f's F1 items and the 13-bit block field of its slow path's items, a window
start above 2^15 in a suspect entry, nb_magic = 2^32 / blocks for thousands of blocks, a wave's share of less than one tile's blocks, the hand-over sizing of
plan_k1h.  Every test asserts that its input is beyond the threshold it is there for.

Every batch of 70 or more reads begins with the nine directed reads of limits_model.DIRECTED; the slot byte among them sends the launch down K1f's
slow path, so the *_fast_path tests run the same batches without it."""
import functools

import numpy as np
import pytest

import limits_model as lm
import orc
from gpu_support import nt  # noqa: F401
from support import assert_same_sketch, oracle_counts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENGTHS = (1009, 4097, 32769, 65520, 65535)
OLD_MAX = 1008  # the longest tiled read of the rest of the suite (the default piece of test_long_gpu.py)


@pytest.fixture(scope="module")
def tile_buf(nt):
    """one tile of 65535-base reads, 134 MB: every test of the module lays its largest batch into it"""
    n = nt.tiled_bytes(2048, 65535)
    assert n == 4096 * 2048 * 16 and n >= nt.tiled_bytes(2049, 4097)
    return torch.empty(n, dtype=torch.uint8, device="cuda")


def upload(buf, tiles):
    assert tiles.size <= buf.numel()
    buf[:tiles.size].copy_(torch.from_numpy(tiles))
    return buf.data_ptr()


same = functools.partial(assert_same_sketch, nonempty=True)  # (the oracle counted something in every plane)


def count_equal(nt, buf, arr, klist, gap=0, r_bits=16, s_bits=7, **kw):
    n, L = arr.shape
    ptr = upload(buf, lm.tile_array(arr))
    with nt.Engine(list(klist), gap=gap, r_bits=r_bits, s_bits=s_bits, flags=nt.FLAG_REQUIRE_TILED, **kw) as e:
        e.submit_tiled_device(ptr, n, L)
        tc, _, f1 = e.finish(counters=True)
    return tc, f1


def batch(n, L, k, seed=0, slot_byte=True):
    rng = np.random.default_rng(1000 * L + 10 * n + k + seed)
    arr = lm.directed_batch(rng, n, L, k)
    if n >= 70:
        if not slot_byte:
            arr[6, L - 20] = lm.N
            assert not np.isin(arr, (1, 3, 4, 5, 7)).any()
        else:
            lm.assert_directed(arr, k)
    else:
        arr[0, L - k - 5] = lm.N  # (a lone read of 1009 random bases would often be clean)
    return arr


def assert_reaches(L, k):
    """the input is beyond what the test is there for"""
    C, nb = (L + 15) // 16, lm.k1h_blocks(k, L)
    assert OLD_MAX < L <= 0xffff  # ntc_submit.hip:615 (ntc_submit_tiled_device: 1 .. 65535)
    if L >= 4097:
        assert C - 1 >= 256  # a chunk index of nine bits
    if L >= 65520:
        assert (C - 1) >> 11 == 1       # ntc_sketch_k1h.hip:145: the chunk field of an F1 item, 12 bits, holds an index with its top bit set
        assert (L - k) >> 15 == 1       # ntc_sketch_k1h.hip:266: a window start (e.z >> 11) of 16 bits
        assert nb - 1 >= 4094 and nb > 2048  # ntc_sketch_k1h.hip:641: nb_magic = 2^32 / blocks with thousands of blocks; fewer than one tile's blocks per wave
    if (L, k) == (65535, 12):
        assert nb - 1 == 4096  # ntc_sketch_k1h.hip:402: the block field of a slow-path item, 13 bits, holds 2^12 (phi = 11: one block more than chunks)
    if (L, k) == (65535, 32):
        assert C == 4096 and nb == 4096 and (1 << 32) % nb == 0  # nb_magic exact here, inexact at k = 12 (4097 blocks)


EQUAL = sorted([(L, n, k) for L in LENGTHS for n in (1, 70) for k in (12, 32)] + [(L, 2049, k) for L in (1009, 4097) for k in (12, 32)])


@pytest.mark.parametrize("L,n,k", EQUAL)
def test_equal_length(nt, tile_buf, L, n, k):
    """ntc_submit_tiled_device: one read, 70 reads (the directed ones and 61 random), and two tiles of which the second holds one read"""
    assert_reaches(L, k)
    if n == 2049:
        assert L <= 4097 and (n + 2047) // 2048 == 2 and n % 2048 == 1
    arr = batch(n, L, k)
    r_bits = 14 if k == 12 else 16
    same(count_equal(nt, tile_buf, arr, [k], r_bits=r_bits), oracle_counts(arr, [k], r_bits=r_bits), (L, n, k))


@pytest.mark.parametrize("L,k", [(L, k) for L in (4097, 65520, 65535) for k in (12, 32)])
def test_equal_length_fast_path(nt, tile_buf, L, k):
    """the batches of 70 without the slot byte (an N in its place): no launch of them takes K1f's slow path, so the suspects K1h hands over — their
    window starts, their dirty marks in three chunks — decide the counts"""
    assert_reaches(L, k)
    arr = batch(70, L, k, slot_byte=False)
    same(count_equal(nt, tile_buf, arr, [k], r_bits=15), oracle_counts(arr, [k], r_bits=15), (L, k))


@pytest.mark.parametrize("L,k,gap", [(L, k, g) for L in (4097, 65535) for k, g in ((12, 2), (32, 8))])
def test_tiled_gap_seeds(nt, tile_buf, L, k, gap):
    """ntcard's -g seeds that have a tiled kernel (stRead, ntcard.cpp:160-171)"""
    assert_reaches(L, k)
    arr = batch(70, L, k, seed=1)
    same(count_equal(nt, tile_buf, arr, [k], gap=gap, r_bits=14), oracle_counts(arr, [k], gap=gap, r_bits=14), (L, k, gap))


@pytest.mark.parametrize("L", [4097, 65520])
def test_k_list(nt, tile_buf, L):
    """one K1h launch per k over the same tiles; the hand-over arrays are sized for the most demanding k of the list (plan_k1h)"""
    kl = (21, 25, 31)
    for k in kl:
        assert_reaches(L, k)
    arr = batch(70, L, max(kl), seed=2)
    same(count_equal(nt, tile_buf, arr, kl, r_bits=15), oracle_counts(arr, kl, r_bits=15), (L, kl))


def test_larger_s_bits_at_65520(nt, tile_buf):
    """sBits = 11: the walk tests 8-bit prefixes of ntComp's patterns, the resolve pass the rest"""
    L, k = 65520, 32
    assert_reaches(L, k)
    arr = batch(70, L, k, seed=3)
    same(count_equal(nt, tile_buf, arr, [k], r_bits=16, s_bits=11), oracle_counts(arr, [k], r_bits=16, s_bits=11), "sBits 11")


def test_forward_strand_at_65535(nt, tile_buf):
    """the one-strand K1h + K1f (NTC_FLAG_STRAND_TILED); the slot byte of the directed reads takes the launch down the slow path, which then counts fh"""
    L, k = 65535, 32
    assert_reaches(L, k)
    arr = batch(70, L, k, seed=4)
    got = count_equal(nt, tile_buf, arr, [k], r_bits=14, strand="forward", strand_tiled=True)
    want = lm.forward_sketch(arr, k, 14, 7)
    same(got, want, "forward")
    assert not np.array_equal(want[0], oracle_counts(arr, [k], r_bits=14)[0])  # (the input tells the strands apart)


def ragged_reads(rng, n, C, k, slot_byte):
    """n reads of C chunks whose tails cycle through 1 .. 16, a few non-base bytes, an N on the last base, on the first base of the last window and on the
    first byte of the last chunk of three of them; slot_byte: a byte 1 (a base to the reference) in the last chunk of a fourth"""
    arr = lm.random_reads(rng, n, 16 * C, lm.P_BAD)
    lens = 16 * (C - 1) + 1 + (np.arange(n) % 16)
    arr[0, lens[0] - 1] = lm.N
    arr[1, lens[1] - k] = lm.N
    arr[2, 16 * (C - 1)] = lm.N
    if slot_byte:
        arr[3, 16 * (C - 1)] = 1
    else:
        assert not np.isin(arr, (1, 3, 4, 5, 7)).any()
    return [arr[i, :lens[i]].tobytes() for i in range(n)]


@pytest.mark.parametrize("C,k", [(257, 32), (257, 17), (4095, 32), (4095, 17)])
def test_ragged(nt, tile_buf, C, k):
    """ntc_submit_tiled_ragged_device: K1h masks the windows behind every read's end in the last chunk, K1f takes every read's length from tails[tile][16];
    k = 17 (phi = 0: blocks = chunks + 1) with a slot byte — the slow path —, k = 32 without — the fast path"""
    n = 70
    assert C - 1 >= 256 and C <= 0xffff // 16  # ntc_submit.hip:627 (1 .. 4095 chunks); a chunk index of nine bits
    if C == 4095:
        assert (C - 1) >> 11 == 1  # ntc_sketch_k1h.hip:145
    reads = ragged_reads(np.random.default_rng(C + k), n, C, k, slot_byte=k == 17)
    assert {len(r) - 16 * (C - 1) for r in reads} == set(range(1, 17))  # every tail
    tiles, tails, _ = nt.tile_reads_ragged(reads, C)
    ptr = upload(tile_buf, tiles)
    dl = torch.from_numpy(tails.reshape(-1).astype(np.int32)).cuda()
    with nt.Engine([k], r_bits=16, s_bits=7, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_tiled_ragged_device(ptr, n, C, dl.data_ptr())
        tc, _, f1 = e.finish(counters=True)
    same((tc, f1), orc.sketch_reads(reads, [k], 0, 16, 7), (C, k))


def test_bins_of_both_extremes_in_one_launch(nt, tile_buf):
    """ntc_submit_tiled_bins_device: a ragged bin of 4095 chunks, an equal-length bin of 150 bp and a ragged bin of 257 chunks share ONE K1h launch
    (K1hMulti): every bin its own chunk count, block count, nb_magic and share of the workgroups (plan_sketch_k1h)"""
    k = 32
    rng = np.random.default_rng(99)
    big = ragged_reads(rng, 70, 4095, k, slot_byte=False)
    mid = ragged_reads(rng, 100, 257, k, slot_byte=False)
    uni = lm.random_reads(rng, 3000, 150, 0.002)
    uni_reads = [uni[i].tobytes() for i in range(3000)]
    assert len(big) == 70 and len(mid) == 100 and max(len(r) for r in big) == 65520 and max(len(r) for r in mid) == 16 * 257
    t_big, l_big, _ = nt.tile_reads_ragged(big, 4095)
    t_mid, l_mid, _ = nt.tile_reads_ragged(mid, 257)
    d_mid, d_uni = torch.from_numpy(t_mid).cuda(), torch.from_numpy(lm.tile_array(uni)).cuda()
    dl_big, dl_mid = (torch.from_numpy(x.reshape(-1).astype(np.int32)).cuda() for x in (l_big, l_mid))
    bins = [(upload(tile_buf, t_big), 70, 16 * 4095, dl_big.data_ptr()), (d_uni.data_ptr(), 3000, 150, 0), (d_mid.data_ptr(), 100, 16 * 257, dl_mid.data_ptr())]
    with nt.Engine([k], r_bits=16, s_bits=7, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_tiled_bins_device(bins)
        tc, _, f1 = e.finish(counters=True)
    same((tc, f1), orc.sketch_reads(big + uni_reads + mid, [k], 0, 16, 7), "bins")
