"""GPU tests of gather (include/ntcard_hip.h: ntc_signature_gather_device; ntcard_amd/csrc/ntc_sig_gather.hip; DESIGN.md §4 "Gather") against the numpy
model tests/sig_gather_model.py.  Every result is an integer and is compared for equality.  Lists are cut from one np.unique pool of random uint64, as
test_sig_matrix_cli_gpu.py cuts them."""
import ctypes as C
import functools

import numpy as np
import pytest

import sig_gather_model
from gpu_support import nt  # noqa: F401
from support import ERR_ARG, random_reads
from test_sig_device_gpu import dev32, dev64

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U32_MAX = 2**32 - 1
SENTINEL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def pool():
    p = np.unique(np.random.default_rng(81).integers(1, 2**64 - 1, size=120_000, dtype=np.uint64))
    assert p.size == 120_000
    p.setflags(write=False)
    return p


def pick(rng, a, n):
    """n entries of a, ascending"""
    return a[np.sort(rng.permutation(a.size)[:n])]


def on_device(q, counts, refs):
    """the query and the DISTINCT arrays of refs in one device allocation (every offset a multiple of 8 bytes) -> (keep-alive, query pointer, counts
    pointer, reference pointers, lengths).  An empty list passes a null pointer; an array listed twice passes one pointer twice"""
    distinct = {}
    for r in refs:
        distinct.setdefault(id(r), r)
    arrays = [q] + list(distinct.values())
    d = dev64(np.concatenate(arrays))
    offs = np.concatenate([[0], np.cumsum([a.size for a in arrays])])
    at = {id(a): d.data_ptr() + 8 * int(o) if a.size else 0 for a, o in zip(arrays, offs)}
    dc = dev32(counts) if counts is not None and q.size else None
    assert d.data_ptr() % 8 == 0
    return (d, dc), at[id(q)], dc.data_ptr() if dc is not None else 0, [at[id(r)] for r in refs], [r.size for r in refs]


def checked(nt, q, counts, refs, **kw):
    """gather on the device == the model; the consequences the header states -> the device's (rows, unassigned, unassigned_weight)"""
    keep, pq, pc, ptrs, ns = on_device(q, counts, refs)
    got = nt.signature_gather_device(pq, pc, q.size, ptrs, ns, **kw)
    want = sig_gather_model.gather(q, counts, refs, **kw)
    rows, rest, rest_w = got
    assert rows.dtype == nt.GATHER_ROW_DTYPE and sig_gather_model.same(got, want), (got, want)
    u = rows["unique"].astype(np.int64)
    assert bool(np.all(u[:-1] >= u[1:])) and int(u.sum()) + rest == q.size and np.unique(rows["ref"]).size == rows.size
    total_w = int(q.size if counts is None else counts.astype(np.uint64).sum(dtype=np.uint64))
    assert int(rows["unique_weight"].sum(dtype=np.uint64)) + rest_w == total_w
    del keep
    return got


def test_overlapping_references(nt):
    p = pool()
    rng = np.random.default_rng(1)
    q = p[:20_000]
    counts = rng.integers(1, 51, size=q.size).astype(np.uint32)
    refs = [p[2000:12_000], np.concatenate([p[3000:9000], p[15_000:15_500]]), p[16_000:25_000]]
    rows, rest, rest_w = checked(nt, q, counts, refs)
    assert rows["ref"].tolist() == [0, 2, 1] and rows["common"].tolist() == [10_000, 4000, 6500] and rows["unique"].tolist() == [10_000, 4000, 500]
    assert rest == 5500 and rest_w == int(counts.astype(np.int64).sum() - rows["unique_weight"].astype(np.int64).sum()) > rest
    assert int(rows["unique_weight"][0]) == int(counts[2000:12_000].astype(np.int64).sum())


def test_tie_goes_to_the_lower_index(nt):
    p = pool()
    q = p[:10_000]
    a = np.concatenate([p[0:1000], p[5000:5200]])  # 1200 common, 200 of them in c
    b = p[2000:3000]                               # 1000 common, none in c
    c = p[5000:8000]
    rows, _, _ = checked(nt, q, None, [a, b, c])
    assert rows["ref"].tolist() == [2, 0, 1] and rows["unique"].tolist() == [3000, 1000, 1000]
    rows, _, _ = checked(nt, q, None, [b, a, c])
    assert rows["ref"].tolist() == [2, 0, 1] and rows["common"].tolist() == [3000, 1000, 1200]
    rows, _, _ = checked(nt, q, None, [p[0:500], p[500:1000]])  # a tie in the first round
    assert rows["ref"].tolist() == [0, 1]


def test_duplicate_and_contained_references_are_reported_once(nt):
    p = pool()
    q, r = p[:5000], p[1000:4000]
    sub = r[100:600]
    d, dq = dev64(r), dev64(q)
    rows, rest, rest_w = nt.signature_gather_device(dq.data_ptr(), 0, q.size, [d.data_ptr(), d.data_ptr(), d.data_ptr() + 8 * 100], [r.size, r.size, sub.size])
    assert sig_gather_model.same((rows, rest, rest_w), sig_gather_model.gather(q, None, [r, r, sub]))
    assert rows.tolist() == [(0, 0, 3000, 3000, 3000)] and (rest, rest_w) == (2000, 2000)
    rows, _, _ = checked(nt, q, None, [sub, r, r])  # the subset first in the list: still only the larger one
    assert rows.tolist() == [(1, 0, 3000, 3000, 3000)]


def test_empty_lists(nt):
    p = pool()
    empty = p[:0]
    rows, rest, rest_w = checked(nt, empty, None, [p[:100], p[50:300]])  # an empty query
    assert rows.size == 0 and (rest, rest_w) == (0, 0)
    rows, rest, _ = checked(nt, p[:1000], None, [p[:100], empty, p[50:300]])  # an empty reference: a null pointer with length 0
    assert rows["ref"].tolist() == [2, 0] and rest == 700
    rows, _, _ = checked(nt, p[:1000], None, [empty])
    assert rows.size == 0
    counts = np.arange(1, 1001, dtype=np.uint32)
    rows, rest, rest_w = checked(nt, p[:1000], counts, [p[1000:1500], p[2000:2001], p[3000:9000]])  # all disjoint from the query
    assert rows.size == 0 and (rest, rest_w) == (1000, 500_500)


@pytest.mark.parametrize("nq, nr", [(200, 20_000), (20_000, 200)], ids=["query_short", "query_long"])
def test_both_search_directions(nt, nq, nr):
    p = pool()
    rng = np.random.default_rng(2)
    q = pick(rng, p[:40_000], nq)
    counts = rng.integers(1, 1000, size=nq).astype(np.uint32)
    refs = [pick(rng, p[:40_000], nr), pick(rng, p[:40_000], nr), pick(rng, p[10_000:50_000], nr + 1), pick(rng, p[:40_000], min(nq, nr))]
    rows, _, _ = checked(nt, q, counts, refs)
    assert rows.size >= 3 and int(rows["common"].min()) >= 1 and int(rows["common"].max()) < min(nq, nr)


def test_slice_edges(nt):
    p = pool()
    q = p[5000:15_000]
    a, b = q[0:4096], q[4096:8193]                    # exactly 4096 hits; 4097: a second work item of one hit
    c = np.concatenate([p[0:4096], q[9000:9001]])     # 4097 entries: a second work item of one entry, the only hit
    d = np.concatenate([q[9500:9501], p[20_000:24_096]])  # ... the first entry the only hit
    assert a.size == 4096 and b.size == 4097 and c.size == 4097 and d.size == 4097 and bool(np.all(c[:-1] < c[1:])) and bool(np.all(d[:-1] < d[1:]))
    rows, rest, _ = checked(nt, q, None, [a, b, c, d])
    assert rows["ref"].tolist() == [1, 0, 2, 3] and rows["unique"].tolist() == [4097, 4096, 1, 1] and rest == 10_000 - 8195
    rows, _, _ = checked(nt, q[8000:9200], None, [a, b, c, d])  # the query is the shorter one: its entries are searched in the references
    assert rows["ref"].tolist() == [1, 2] and rows["unique"].tolist() == [193, 1]


def test_weights_beyond_32_bits(nt):
    p = pool()
    q = p[:3000]
    counts = np.ones(q.size, dtype=np.uint32)
    counts[[10, 1500]] = U32_MAX
    counts[2000] = U32_MAX
    refs = [p[0:1600], p[1500:2500]]
    rows, rest, rest_w = checked(nt, q, counts, refs)
    assert rows["ref"].tolist() == [0, 1] and int(rows["unique_weight"][0]) == 2 * U32_MAX + 1598 > 2**33 and int(rows["unique_weight"][1]) == U32_MAX + 899
    assert (rest, rest_w) == (500, 500)
    rows, rest, rest_w = checked(nt, q, None, refs)  # no counts: every weight is a number of entries
    assert np.array_equal(rows["unique_weight"], rows["unique"]) and rest_w == rest == 500


def disjoint_refs(sizes):
    p = pool()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return [p[int(a): int(b)] for a, b in zip(offs[:-1], offs[1:])], int(offs[-1])


@pytest.mark.parametrize("n", [31, 32, 33])
def test_rows_across_the_read_back_of_a_batch(nt, n):
    """the host reads `done` back every 32 rounds: 31, 32 and 33 rows"""
    refs, used = disjoint_refs([200 - 3 * i for i in range(n)])
    q = pool()[:used + 77]
    counts = np.random.default_rng(3).integers(1, 9, size=q.size).astype(np.uint32)
    rows, rest, _ = checked(nt, q, counts, refs, threshold=5)
    assert rows["ref"].tolist() == list(range(n)) and rows["unique"].tolist() == [200 - 3 * i for i in range(n)] and rest == 77


def test_threshold_stops_inside_a_batch(nt):
    """rounds 4 .. 8 are enqueued behind the stop: they must clear nothing"""
    refs, used = disjoint_refs([500, 400, 300, 50, 40, 30, 20])
    q = pool()[:used + 10]
    rows, rest, rest_w = checked(nt, q, None, refs, threshold=100)
    assert rows["ref"].tolist() == [0, 1, 2] and rest == 50 + 40 + 30 + 20 + 10 == rest_w
    rows, rest, _ = checked(nt, q, None, refs, threshold=50)  # the threshold itself is reported
    assert rows["ref"].tolist() == [0, 1, 2, 3] and rest == 100


def test_rows_cap(nt):
    refs, used = disjoint_refs([500, 400, 300, 50])
    q = pool()[:used]
    counts = np.full(q.size, 3, dtype=np.uint32)
    rows, rest, rest_w = checked(nt, q, counts, refs, max_rows=2)
    assert rows["ref"].tolist() == [0, 1] and (rest, rest_w) == (350, 1050)  # the state after the reported rows
    rows, rest, rest_w = checked(nt, q, counts, refs, max_rows=0)
    assert rows.size == 0 and (rest, rest_w) == (q.size, 3 * q.size)
    rows, rest, _ = checked(nt, q, counts, refs, max_rows=9)  # more room than references
    assert rows.size == 4 and rest == 0


def test_threshold_zero_is_threshold_one(nt):
    p = pool()
    q = p[:1000]
    refs = [p[999:1500], p[100:300]]  # one common entry
    for threshold in (0, 1):
        rows, rest, _ = checked(nt, q, None, refs, threshold=threshold)
        assert rows["ref"].tolist() == [1, 0] and rows["unique"].tolist() == [200, 1] and rest == 799
    rows, _, _ = checked(nt, q, None, refs, threshold=2)
    assert rows["ref"].tolist() == [1]


def raw_call(nt, q, refs):
    """the C entry itself over sentinel outputs -> (rc, message, outputs untouched?)"""
    L = nt._abi.lib()
    keep, pq, _, ptrs, ns = on_device(q, None, refs)
    arr = (C.c_void_p * len(refs))(*ptrs)
    n = (C.c_uint64 * len(refs))(*ns)
    rows = np.full(4 * len(refs), SENTINEL, dtype=np.uint64)
    n_rows, rest, rest_w = C.c_uint32(SENTINEL), C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    rc = L.ntc_signature_gather_device(0, None, C.c_void_p(pq), None, q.size, len(refs), arr, n, 1, rows.ctypes.data_as(C.POINTER(nt._abi.NtcGatherRow)), len(refs),
                                       C.byref(n_rows), C.byref(rest), C.byref(rest_w))
    del keep
    return rc, L.ntc_last_error().decode(), bool(np.all(rows == SENTINEL)) and (n_rows.value, rest.value, rest_w.value) == (SENTINEL,) * 3


def test_unsorted_lists_are_refused(nt):
    p = pool()
    q, refs = p[:2000], [p[0:100], p[50:400], p[300:900], p[1000:1001]]
    bad_q = q.copy()
    bad_q[1234] = bad_q[1233]  # a repeat
    rc, msg, untouched = raw_call(nt, bad_q, refs)
    assert rc == ERR_ARG and "the query is not strictly ascending at entry 1234" in msg and untouched
    bad_r = refs[2].copy()
    bad_r[[17, 18]] = bad_r[[18, 17]]  # a step back
    rc, msg, untouched = raw_call(nt, q, refs[:2] + [bad_r] + refs[3:])
    assert rc == ERR_ARG and "reference 2 is not strictly ascending at entry 18" in msg and untouched
    # the query and reference 0 are both bad: the query is named
    small_q, small_r = p[:8].copy(), p[2:8].copy()
    small_q[6], small_r[2] = small_q[4], small_r[1]
    rc, msg, untouched = raw_call(nt, small_q, [small_r, p[3:7]])
    assert rc == ERR_ARG and "the query is not strictly ascending at entry 6" in msg and "reference" not in msg and untouched
    rc, msg, untouched = raw_call(nt, q, refs)
    assert rc == 0 and not untouched


def test_1024_small_references(nt):
    p = pool()
    rng = np.random.default_rng(4)
    q = pick(rng, p[:80_000], 50_000)
    counts = rng.integers(1, 2**20, size=q.size).astype(np.uint32)
    sizes = rng.integers(100, 401, size=1024)
    refs = [pick(rng, p[:100_000], int(n)) for n in sizes]
    refs[700] = refs[3]  # one listed twice
    rows, rest, _ = checked(nt, q, counts, refs, threshold=150)
    assert 40 < rows.size < 1024 and int(rows["ref"].max()) > 768 and 700 not in rows["ref"].tolist() and 0 < rest < q.size
    rows, _, _ = checked(nt, q, counts, refs, max_rows=70, threshold=1)  # past two read-backs, stopped by the cap
    assert rows.size == 70


def test_engine_round_trip(nt):
    """real signatures: two read sets counted alone are the references, both together are the query"""
    rng = np.random.default_rng(5)
    sets = [[r.tobytes() for r in random_reads(rng, n, 150, 0.0)] for n in (300, 400)]
    with nt.Engine([32], r_bits=14, s_bits=7, signature=True) as ea, nt.Engine([32], r_bits=14, s_bits=7, signature=True) as eb, \
            nt.Engine([32], r_bits=14, s_bits=7, signature=True) as eq:
        ea.submit_reads(sets[0])
        eb.submit_reads(sets[1])
        eq.submit_reads(sets[0])
        eq.submit_reads(sets[1])
        (ha, _, na), (hb, _, nb), (hq, cq, nq) = ea.signature_device(), eb.signature_device(), eq.signature_device()
        host = [x.cpu().numpy().view(np.uint64) for x in (ha, hb, hq)]
        assert np.array_equal(host[0], ea.signature()[0]) and min(na, nb) > 300 and na != nb
        got = nt.signature_gather_device(hq.data_ptr(), cq.data_ptr(), nq, [ha.data_ptr(), hb.data_ptr()], [na, nb])
    rows, rest, rest_w = got
    assert sig_gather_model.same(got, sig_gather_model.gather(host[2], cq.cpu().numpy().view(np.uint32), host[:2]))
    first = 0 if na > nb else 1
    assert rows["ref"].tolist() == [first, 1 - first] and int(rows["unique"][0]) == max(na, nb) and (rest, rest_w) == (0, 0)
    assert int(rows["unique"].sum()) == nq and int(rows["common"][1]) == min(na, nb)
