"""GPU tests of the signature kernels above their grid caps (ntcard_amd/csrc/ntc_signature.hip, ntc_sig_sort.hip, ntc_sig_lists.hip; DESIGN.md §4 "Sort and compare", the table
of thresholds).  Every kernel there caps its grid and walks the rest of its input in a grid-stride loop, the matrix cuts its work into rounds of 2^18 items
and the sort's scan walks its row 256 tiles at a time: each case here is the smallest that takes such a loop into a second turn, asserts the size that
makes it do so before it touches the device, and compares with numpy or the oracle (np.unique, np.argsort(kind="stable"), np.intersect1d, a
membership-matrix product, sig_model.model, orc.sketch_reads), never with the code under test.

Not tested, here or elsewhere: the 2^30-per-launch split of sig_inject_device, n >= 2^32 (beyond the refusals of the argument checks) and the
out-of-memory returns — each needs many GiB on the device or has to exhaust a card that others share."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
import sig_model
from test_sig_device_gpu import dev32, dev64
from test_sig_sort_gpu import KEY_SETS, check_sort
from gpu_support import nt  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 14
ERR_ARG = -1
U32_MAX = 2**32 - 1
INSERT_STRIDE = 4096 * 256   # sig_insert_kernel, sig_compact_kernel: entries (slots) per turn
ASCENT_STRIDE = 1024 * 256   # sig_ascent_kernel: the first turn covers the entries 1 .. ASCENT_STRIDE
COMPARE_STRIDE = 8192 * 256  # sig_compare_kernel: entries of the shorter list per turn
MAT_CHUNK, MAT_ITEMS = 4096, 2**18  # ntc_signature_matrix_device: entries per work item, work items per round
SORT_TILE, SCAN_TILES = 4096, 256   # the sort: pairs per tile, tiles per turn of sort_scan_kernel
DEFAULT_SLOTS = 2**16


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def same_sig(got, wh, wc):
    h, c = got
    return h.dtype == np.uint64 and c.dtype == np.uint32 and np.array_equal(h, wh) and np.array_equal(c.astype(np.uint64), np.asarray(wc).astype(np.uint64))


# ---- A. the container above one stride ----
@functools.lru_cache(maxsize=None)
def many_keys():
    """1 250 000 distinct non-zero keys and 100 000 repeats of them, shuffled -> (keys, np.unique of them, counts)"""
    rng = np.random.default_rng(51)
    base = np.unique(rng.integers(1, 2**64, size=1_260_000, dtype=np.uint64))
    base = base[rng.permutation(base.size)[:1_250_000]]
    keys = np.concatenate([base, rng.choice(base, size=100_000)])
    rng.shuffle(keys)
    wh, wc = np.unique(keys, return_counts=True)
    return frozen(keys, wh, wc)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_countless_inject_and_rehash_of_a_large_table(nt, device):
    keys, wh, wc = many_keys()
    first, rest = keys[:600_000], keys[600_000:]
    live = np.unique(first).size
    assert keys.size == 1_350_000 and keys.size % 64 != 0 and wh.size == 1_250_000 and int(wc.max()) >= 2 and not np.any(keys == 0)
    assert DEFAULT_SLOTS < 2 * first.size <= 2**21  # the first call grows the table to 2^21 slots,
    assert 2**21 < 2 * (live + rest.size) <= 2**22  # the second to 2^22: it re-inserts 2^21 old slots
    assert 2**21 >= 2 * INSERT_STRIDE and 2**22 >= 4 * INSERT_STRIDE  # two turns of the rehash, four of the compaction
    assert rest.size <= INSERT_STRIDE < keys.size  # the second call's own insert is one turn; all keys in one call are two
    d = dev64(keys)

    def inject(e, lo, hi):
        if device:
            e.signature_inject((d.data_ptr() + 8 * lo, hi - lo), device=True)
        else:
            e.signature_inject(keys[lo:hi])

    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e, nt.Engine([32], r_bits=R, s_bits=7, signature=True) as one:
        assert e.signature_stats() == (DEFAULT_SLOTS, 0)
        inject(e, 0, first.size)
        assert e.signature_stats() == (2**21, 5)
        inject(e, first.size, keys.size)
        assert e.signature_stats() == (2**22, 6)
        assert same_sig(e.signature(), wh, wc)
        inject(one, 0, keys.size)  # sig_insert_kernel<false> itself in two turns
        assert one.signature_stats() == (2**22, 6)
        assert same_sig(one.signature(), wh, wc)


def test_counted_inject_above_one_stride(nt):
    rng = np.random.default_rng(52)
    base = rng.integers(1, 2**64, size=900_000, dtype=np.uint64)
    hot_exact, hot_sat = np.uint64(0x0123456789abcdef), np.uint64(0xfedcba9876543211)
    keys = np.concatenate([base, rng.choice(base, size=40_001), np.full(60_000, hot_exact), np.full(100_000, hot_sat)])
    counts = np.concatenate([rng.integers(1, 1001, size=940_001), np.full(160_000, 70_000)]).astype(np.uint32)
    order = rng.permutation(keys.size)
    keys, counts = keys[order], counts[order]
    assert keys.size == 1_100_001 and keys.size > INSERT_STRIDE and not np.any(keys == 0)
    for hot in (hot_exact, hot_sat):  # both turns hold copies of both hot keys
        at = np.flatnonzero(keys == hot)
        assert at[0] < INSERT_STRIDE <= at[-1] and np.count_nonzero(at >= INSERT_STRIDE) > 1000
    wh, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(wh.size, dtype=np.uint64)
    np.add.at(sums, inv.reshape(-1), counts.astype(np.uint64))
    wc = np.minimum(sums, np.uint64(U32_MAX))
    assert wh.size <= 900_002 and int(sums[wh == hot_exact][0]) == 4_200_000_000 < U32_MAX < int(sums[wh == hot_sat][0]) == 7_000_000_000
    assert np.count_nonzero(sums > U32_MAX) == 1
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e:
        e.signature_inject(keys, counts)
        h, c = e.signature()
        assert same_sig((h, c), wh, wc)
        assert int(c[h == hot_exact][0]) == 4_200_000_000 and int(c[h == hot_sat][0]) == U32_MAX


@functools.lru_cache(maxsize=None)
def generated():
    """20 000 generated reads of 150 bases -> (row slots as the oracle's generator writes them, the reads, the model of their signature at k 32, sBits 2)"""
    n, L, stride = 20_000, 150, 152
    slots = orc.gen_reads(5, 0, n, L, stride, 0)
    reads = [slots[i * stride: i * stride + L].tobytes() for i in range(n)]
    wh, wc = sig_model.model(reads, 32, "canonical", 2)
    return frozen(slots), reads, frozen(wh, wc)


def test_value_log_above_one_stride(nt):
    slots, reads, (wh, wc) = generated()
    n, L, stride = len(reads), 150, 152
    pairs = int(wc.sum())
    assert pairs == 1_227_176 and int(wc.max()) == 1  # one flush inserts them all: more than a turn of sig_insert_kernel<false>,
    assert INSERT_STRIDE < pairs and n * (L - 32 + 1) + 2**20 < 2**27  # and the default log (chunks of 1024) holds the batch's windows in one launch
    d = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
    nt.gen_reads_device(d.data_ptr(), 5, 0, n, L, stride, 0)
    torch.cuda.synchronize()
    assert np.array_equal(d[: n * stride].cpu().numpy(), slots)
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        e.submit_device(d.data_ptr(), n, L, stride)
        assert same_sig(e.signature(), wh, wc)
        e.submit_device(d.data_ptr(), n, L, stride)
        h, c = e.signature()
        assert np.array_equal(h, wh) and c.dtype == np.uint32 and bool(np.all(c == 2))
        tc, _, f1 = e.finish(counters=True)
    oc, of1 = orc.sketch_reads(reads + reads, [32], 0, R, 2)
    assert int(of1[0]) == 2 * n * (L - 32 + 1) and np.array_equal(f1, of1) and np.array_equal(tc, oc)


def test_one_hot_value_across_strides(nt):
    n, L = 40_000, 64
    wh, wc = sig_model.model([b"C" * L], 32, "canonical", 2)
    assert wh.size == 1 and int(wc[0]) == 33  # every window is sampled and they are one value
    entries = n * int(wc[0])
    assert entries == 1_320_000 and entries > INSERT_STRIDE and entries + 2**20 < 2**27  # one launch, one flush, two turns of the hot-value shortcut
    d = torch.from_numpy(np.concatenate([np.full(n * L, ord("C"), np.uint8), np.full(16, ord("A"), np.uint8)])).cuda()
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        e.submit_device(d.data_ptr(), n, L, L)
        h, c = e.signature()
        assert np.array_equal(h, wh) and c.tolist() == [entries]
        assert int(e.finish()[2][0]) == entries


# ---- B. compare and ascent above one stride ----
@functools.lru_cache(maxsize=None)
def big_pool():
    p = np.unique(np.random.default_rng(61).integers(1, 2**64 - 1, size=3_500_000, dtype=np.uint64))
    assert p.size == 3_500_000
    return frozen(p)


def test_compare_above_one_stride(nt):
    p = big_pool()
    rng = np.random.default_rng(62)
    a = p[np.sort(rng.permutation(p.size)[:2_200_000])]
    b = p[np.sort(rng.permutation(p.size)[:2_300_000])]
    ca = rng.integers(1, 2**32, size=a.size, dtype=np.uint64).astype(np.uint32)
    cb = rng.integers(1, 2**32, size=b.size, dtype=np.uint64).astype(np.uint32)
    assert min(a.size, b.size) > COMPARE_STRIDE  # the shorter list is the one a lane takes an entry of
    common, ia, ib = np.intersect1d(a, b, assume_unique=True, return_indices=True)
    want_sum = int(np.minimum(ca[ia], cb[ib]).astype(np.uint64).sum(dtype=np.uint64))
    assert 1_300_000 < common.size < 1_600_000 and np.count_nonzero(ia >= COMPARE_STRIDE) > 10_000 and want_sum > 2**50
    da, db, dca, dcb = dev64(a), dev64(b), dev32(ca), dev32(cb)
    assert nt.signature_compare_device(da.data_ptr(), dca.data_ptr(), a.size, db.data_ptr(), dcb.data_ptr(), b.size) == (common.size, want_sum)
    assert nt.signature_compare_device(db.data_ptr(), dcb.data_ptr(), b.size, da.data_ptr(), dca.data_ptr(), a.size) == (common.size, want_sum)
    assert nt.signature_compare_device(da.data_ptr(), 0, a.size, db.data_ptr(), 0, b.size) == (common.size, None)


ASCENT_N = 300_001


def planted(kinds):
    """big_pool()'s first ASCENT_N entries with one violation per (entry, kind): "dup" repeats the entry before, "step" falls back to the one before that"""
    x = big_pool()[:ASCENT_N].copy()
    for at, kind in kinds:
        assert 2 <= at < ASCENT_N
        x[at] = x[at - 1] if kind == "dup" else x[at - 2]
    bad = np.flatnonzero(x[:-1] >= x[1:]) + 1
    assert bad.tolist() == sorted(at for at, _ in kinds)  # exactly the planted entries
    return x


@pytest.mark.parametrize("kinds, names", [
    (((ASCENT_STRIDE, "dup"),), ASCENT_STRIDE),           # the last entry of the first turn
    (((ASCENT_STRIDE + 1, "step"),), ASCENT_STRIDE + 1),  # the first of the second turn
    (((ASCENT_N - 1, "step"),), ASCENT_N - 1),            # the last entry
    (((290_000, "dup"), (ASCENT_STRIDE + 1, "step")), ASCENT_STRIDE + 1),  # two: the first one is named
], ids=["last_of_first_turn", "first_of_second_turn", "last_entry", "two_violations"])
def test_compare_refuses_a_violation_beyond_the_first_turn(nt, kinds, names):
    assert ASCENT_N > ASCENT_STRIDE + 1 and ASCENT_N - 1 > ASCENT_STRIDE + 1  # the list has a second turn, and its last entry is not the turn's first
    assert names == ASCENT_STRIDE or names > ASCENT_STRIDE
    good, bad = big_pool()[:70_000], planted(kinds)
    dg, db = dev64(good), dev64(bad)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_compare_device(db.data_ptr(), 0, bad.size, dg.data_ptr(), 0, good.size)
    assert ei.value.code == ERR_ARG and "first list" in str(ei.value) and f"entry {names} " in str(ei.value)  # (" (status ...)" follows the number)
    with pytest.raises(nt.NtcError) as ei:
        nt.signature_compare_device(dg.data_ptr(), 0, good.size, db.data_ptr(), 0, bad.size)
    assert ei.value.code == ERR_ARG and "second list" in str(ei.value) and f"entry {names} " in str(ei.value)


def test_matrix_refuses_a_violation_beyond_the_first_turn(nt):
    p = big_pool()
    at = ASCENT_N - 2
    assert at > ASCENT_STRIDE
    lists = [p[:3000], p[1000:1500], planted(((at, "dup"),)), p[2000:2007]]
    dl = [dev64(x) for x in lists]
    L = nt._abi.lib()
    ptrs = (C.c_void_p * 4)(*[d.data_ptr() for d in dl])
    ns = (C.c_uint64 * 4)(*[x.size for x in lists])
    out = np.full((4, 4), 0x5a5a5a5a, dtype=np.uint64)
    assert L.ntc_signature_matrix_device(0, None, 4, ptrs, ns, out.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert b"list 2 " in L.ntc_last_error() and L.ntc_last_error().endswith(b"entry %d" % at) and bool(np.all(out == 0x5a5a5a5a))


# ---- C. the matrix in more than one round ----
def work_items(ns):
    """the work items ntc_signature_matrix_device cuts the pairs into: ceil(min(n_i, n_j) / MAT_CHUNK), summed over i < j"""
    ns = np.asarray(ns, dtype=np.int64)
    return int(np.triu(-(-np.minimum.outer(ns, ns) // MAT_CHUNK), 1).sum())


def drawn_lists(universe, sizes, rng):
    """-> (lists: sizes[i] values of the universe each, ascending; M: bool[list, value of the universe])"""
    M = np.zeros((len(sizes), universe.size), dtype=bool)
    for i, n in enumerate(sizes):
        M[i, rng.permutation(universe.size)[:n]] = True
    return [universe[M[i]] for i in range(len(sizes))], M


def membership_product(M):
    m = M.astype(np.float64)
    return (m @ m.T).astype(np.uint64)  # exact: every sum is a whole number far below 2^53


def matrix_on_device(nt, lists):
    """all lists in ONE device allocation (every offset a multiple of 8 bytes); an empty list passes a null pointer"""
    d = dev64(np.concatenate(lists))
    offs = np.concatenate([[0], np.cumsum([x.size for x in lists])])
    assert d.data_ptr() % 8 == 0
    got = nt.signature_matrix_device([d.data_ptr() + 8 * int(o) if x.size else 0 for o, x in zip(offs, lists)], [x.size for x in lists])
    assert got.dtype == np.uint64 and got.shape == (len(lists), len(lists))
    return got


def test_matrix_of_1024_lists_takes_two_rounds(nt):
    rng = np.random.default_rng(71)
    universe = np.unique(rng.integers(1, 2**64 - 1, size=512, dtype=np.uint64))
    sizes = rng.integers(1, 25, size=1024)
    empty = [0, 1, 500, 777, 1023]
    sizes[empty] = 0
    sizes[[2, 3]] = 1, 24
    assert universe.size == 512 and sizes.size == 1024 and sizes.max() == 24
    full = 1024 - len(empty)
    assert work_items(np.maximum(sizes, 1)) == 523_776 and work_items(sizes) == full * (full - 1) // 2 == 518_671
    assert MAT_ITEMS < work_items(sizes) < 2 * MAT_ITEMS  # two rounds, the second not full
    lists, M = drawn_lists(universe, sizes, rng)
    want = membership_product(M)
    assert want.diagonal().tolist() == sizes.tolist() and not want[empty].any() and int(want.max()) == 24
    got = matrix_on_device(nt, lists)
    assert np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def round_lists():
    """604 lists in shuffled order whose pairs are exactly 2^18 work items, and a 605th of one entry -> (lists, their product, the index of a short list)"""
    rng = np.random.default_rng(72)
    universe = np.unique(rng.integers(1, 2**64 - 1, size=12_288, dtype=np.uint64))
    assert universe.size == 12_288
    long_, mid, short = rng.integers(8193, 9001, size=46), rng.integers(4097, 8193, size=352), rng.integers(1, 4097, size=206)
    long_[:2], mid[:2], short[:2] = (8193, 9000), (4097, 8192), (1, 4096)  # the ends of every class
    sizes = np.concatenate([long_, mid, short])[rng.permutation(604)]
    sizes = np.concatenate([sizes, [1]])
    lists, M = drawn_lists(universe, sizes, rng)
    drop = int(np.flatnonzero(sizes[:604] <= MAT_CHUNK)[-1])
    return lists, frozen(membership_product(M)), drop


@pytest.mark.parametrize("variant", ["below", "exact", "above"])
def test_matrix_at_one_full_round(nt, variant):
    lists, want, drop = round_lists()
    keep = {"below": [i for i in range(604) if i != drop], "exact": list(range(604)), "above": list(range(605))}[variant]
    lists, want = [lists[i] for i in keep], want[np.ix_(keep, keep)]
    ns = [x.size for x in lists]
    # C(604, 2) + C(398, 2) + C(46, 2) = 182 106 + 79 003 + 1 035 = 2^18: the round fills inside the loop over the pairs and the closing one is empty;
    # a short list less: one round that is not full; a list more: a second round of 604 items
    assert work_items(ns) == {"below": MAT_ITEMS - 603, "exact": MAT_ITEMS, "above": MAT_ITEMS + 604}[variant]
    assert want.diagonal().tolist() == ns and int(want.min()) == 0 < int(np.triu(want, 1).max())
    got = matrix_on_device(nt, lists)
    assert np.array_equal(got, want)


# ---- D. the sort's tile loop with a carry ----
@pytest.mark.parametrize("name", ["uniform", "top_byte_only", "sixteen_values"])
def test_sort_scans_its_rows_in_four_turns(nt, name):
    n = 769 * SORT_TILE + 5
    tiles = -(-n // SORT_TILE)
    assert tiles == 770 and -(-tiles // SCAN_TILES) == 4 and tiles - 3 * SCAN_TILES == 2  # three turns with a full carry, the last with two live threads
    keys = KEY_SETS[name](n)
    assert keys.size == n and keys.dtype == np.uint64
    check_sort(nt, keys)
