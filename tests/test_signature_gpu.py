"""GPU tests of signatures (include/ntcard_hip.h: NTC_FLAG_SIGNATURE): every plane's (hash, count) pairs exactly against tests/sig_model.py — the oracle's
values, ntComp's two patterns, np.unique — and t_Counter / F1 exactly against the oracle and against the same engine without the flag.  rBits 14 and
strand_model.sketch_reads_equal() (320 reads x 150 bases, 36 451 windows at k = 32) throughout; the container is also driven on chosen keys, without
hashing, through ntc_signature_inject*."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
import sig_model
import strand_model as sm
from test_hpc_gpu import MASK
from gpu_support import device_slots, nt, on_device, submit_slots  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 14
ERR_ARG, ERR_STATE = -1, -4


def reads():
    return list(sig_model.equal_reads())


@functools.lru_cache(maxsize=None)
def oracle(kl, s):
    return orc.sketch_reads(reads(), list(kl), 0, R, s)


def same_sig(got, want, times=1):
    h, c = got
    return h.dtype == np.uint64 and c.dtype == np.uint32 and np.array_equal(h, want[0]) and np.array_equal(c.astype(np.int64), want[1] * times)


# ---- 1. basic ----
def test_basic(nt):
    want = sig_model.equal_model(32, "canonical", 7)
    assert want[0].size == 593 and int(want[1].sum()) == 593
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e, nt.Engine([32], r_bits=R, s_bits=7) as plain:
        submit_slots(e, sig_model.equal_reads())
        submit_slots(plain, sig_model.equal_reads())
        assert e.signature_size() == 593
        assert same_sig(e.signature(), want)
        tc, ph, f1 = e.finish(counters=True)
        tc0, ph0, f10 = plain.finish(counters=True)
        oc, of1 = oracle((32,), 7)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
        assert np.array_equal(f1, f10) and np.array_equal(tc, tc0) and np.array_equal(ph, ph0)
        assert int(tc.sum()) == 593  # every sampled k-mer is one increment and one signature entry
        # a short array is refused with nothing written
        h = np.full(593, 7, dtype=np.uint64)
        c = np.full(593, 7, dtype=np.uint32)
        n = C.c_uint64(12345)
        L = nt._abi.lib()
        rc = L.ntc_signature(e._h, 0, h.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), 592, C.byref(n))
        assert rc == ERR_ARG and n.value == 12345 and np.all(h == 7) and np.all(c == 7)
        assert L.ntc_signature(e._h, 1, h.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), 593, C.byref(n)) == ERR_ARG  # no such plane
        assert same_sig(e.signature(), want)  # (asking twice changes nothing)
        # an engine without the flag has no signature
        with pytest.raises(nt.NtcError) as ei:
            plain.signature_size()
        assert ei.value.code == ERR_STATE


# ---- 2. growth, 3. several insert rounds ----
@pytest.mark.parametrize("log_entries", [None, 4096, 64])
def test_growth_from_64_slots(nt, monkeypatch, log_entries):
    want = sig_model.equal_model(32, "canonical", 2)
    assert want[0].size == 18636 and int(want[1].max()) == 1
    monkeypatch.setenv("NTC_SIG_SLOTS", "64")
    if log_entries is not None:
        assert log_entries < int(want[1].sum())  # one batch needs several insert rounds (64: the floor of four slots' windows per launch)
        monkeypatch.setenv("NTC_SIG_LOG_ENTRIES", str(log_entries))
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        assert e.signature_stats() == (64, 0)
        submit_slots(e, sig_model.equal_reads())
        assert same_sig(e.signature(), want)
        submit_slots(e, sig_model.equal_reads())
        h, c = e.signature()
        assert np.array_equal(h, want[0]) and np.all(c == 2)
        slots, grows = e.signature_stats()
        assert grows >= 9 and slots >= 2 * 18636 and slots & (slots - 1) == 0
        tc, _, f1 = e.finish(counters=True)
        oc, of1 = oracle((32,), 2)
        assert np.array_equal(f1, 2 * of1) and np.array_equal(tc, (2 * oc.astype(np.uint32)).astype(np.uint16))


# ---- 4. one hot key ----
def test_one_hot_key(nt, monkeypatch):
    poly = [b"C" * 64] * 4096
    wh, wc = sig_model.model(poly[:1], 32, "canonical", 2)
    assert wh.size == 1 and int(wc[0]) == 33  # all 33 windows are sampled and they are one value
    monkeypatch.setenv("NTC_SIG_SLOTS", "64")
    a = np.frombuffer(b"".join(poly), dtype=np.uint8).copy()
    d = torch.from_numpy(np.concatenate([a, np.full(16, ord("A"), np.uint8)])).cuda()
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        e.submit_device(d.data_ptr(), 4096, 64, 64)
        h, c = e.signature()
        assert np.array_equal(h, wh) and c.tolist() == [4096 * 33]
    mixed = reads() + poly
    mh, mc = sig_model.equal_model(32, "canonical", 2)
    assert wh[0] not in mh
    at = int(np.searchsorted(mh, wh[0]))
    want = (np.insert(mh, at, wh[0]), np.insert(mc, at, 4096 * 33))
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        e.submit_reads(mixed)
        assert same_sig(e.signature(), want)


def test_every_window_sampled_fills_the_booked_log_exactly(nt, monkeypatch):
    """a ragged (slot table) batch booked by its stride in which every window is sampled, under a log so small that every launch books it to the brim:
    a wave wastes nothing at a chunk boundary, so the booking (windows + one chunk per wave) holds"""
    monkeypatch.setenv("NTC_SIG_LOG_ENTRIES", "4096")
    monkeypatch.setenv("NTC_SIG_SLOTS", "64")
    rs = [b"C" * 64] * 2000 + [b"C" * 50, b"C" * 63, b"C" * 31]
    wh, wc = sig_model.model(rs, 32, "canonical", 2)
    assert wh.size == 1 and int(wc[0]) == 2000 * 33 + 19 + 32
    with nt.Engine([32], r_bits=R, s_bits=2, signature=True) as e:
        e.submit_reads(rs)
        h, c = e.signature()
        assert np.array_equal(h, wh) and c.tolist() == [int(wc[0])]
        assert int(e.finish()[2][0]) == int(wc[0])


# ---- 5. planes ----
def test_fused_k_list(nt):
    kl = (24, 32, 48, 64)
    models = [sig_model.equal_model(k, "canonical", 2) for k in kl]
    assert all(m[0].size > 10000 for m in models)
    assert all(not np.array_equal(models[i][0], models[j][0]) for i in range(4) for j in range(i))
    with nt.Engine(list(kl), r_bits=R, s_bits=2, signature=True) as e:
        submit_slots(e, sig_model.equal_reads())
        for pl in range(4):
            assert same_sig(e.signature(pl), models[pl]), kl[pl]
        tc, _, f1 = e.finish(counters=True)
        oc, of1 = oracle(kl, 2)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
        assert e.signature_stats()[0] >= sum(2 * m[0].size for m in models)


def test_k12_counts_up_to_three(nt):
    want = sig_model.equal_model(12, "canonical", 2)
    assert (int(want[1].sum()), want[0].size, int(want[1].max())) == (22622, 22482, 3)
    with nt.Engine([12], r_bits=R, s_bits=2, signature=True) as e:
        submit_slots(e, sig_model.equal_reads())
        assert same_sig(e.signature(), want)


# ---- 6. forms ----
FORMS = {
    "mask": dict(spec=MASK, strand="canonical", hpc=False),
    "forward": dict(spec=32, strand="forward", hpc=False),
    "reverse_strand_tiled": dict(spec=32, strand="reverse", hpc=False, strand_tiled=True),
    "hpc": dict(spec=32, strand="canonical", hpc=True),
    "mask_forward_hpc": dict(spec=MASK, strand="forward", hpc=True),
}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_forms(nt, name):
    f = FORMS[name]
    s = 4
    want = sig_model.equal_model(f["spec"], f["strand"], s, f["hpc"])
    assert want[0].size > 1000
    plain = sig_model.equal_model(32 if isinstance(f["spec"], int) else len(f["spec"]), "canonical", s)
    assert not np.array_equal(want[0], plain[0])  # the form changes which values are sampled
    kw = dict(r_bits=R, s_bits=s, strand=f["strand"], hpc=f["hpc"], signature=True, strand_tiled=f.get("strand_tiled", False))
    e = nt.Engine([f["spec"]], **kw) if isinstance(f["spec"], int) else nt.Engine.from_seeds([f["spec"]], **kw)
    with e:
        e.submit_reads(reads())
        assert same_sig(e.signature(), want)
        hd = e.signature_header()
        assert hd["mask"] == ("1" * 32 if isinstance(f["spec"], int) else f["spec"]) and hd["strand"] == sm.STRANDS[f["strand"]] and hd["hpc"] == int(f["hpc"]) and hd["s_bits"] == s
        tc, ph, f1 = e.finish(counters=True)
    del kw["signature"]
    e = nt.Engine([f["spec"]], **kw) if isinstance(f["spec"], int) else nt.Engine.from_seeds([f["spec"]], **kw)
    with e:  # the same engine without the flag: bit-identical counters (what THEY must be is tests/test_strand_gpu.py's, test_seeds_gpu.py's, test_hpc_gpu.py's)
        e.submit_reads(reads())
        tc0, ph0, f10 = e.finish(counters=True)
    assert np.array_equal(f1, f10) and np.array_equal(tc, tc0) and np.array_equal(ph, ph0) and int(f1[0]) > 20000
    assert int(tc.sum()) == int(want[1].sum())  # every sampled value is one increment


def test_fused_k_list_of_one_strand(nt):
    """K1's row <true, 0, 10, false, false, true, true> (profiles/k1_variants.txt), which no other test dispatches: a fused k list on a forward engine, 130 reads in
    row slots (two full waves and a partial one) — every plane's pairs against the model, the counters against strand_model"""
    d, _, L, stride = device_slots(sig_model.equal_reads(), 150, 152)
    rs, klist = reads()[:130], [64, 96]
    with nt.Engine(klist, r_bits=R, s_bits=4, strand="forward", signature=True) as e:
        e.submit_device(d.data_ptr(), len(rs), L, stride)
        for pl, k in enumerate(klist):
            want = sig_model.model(rs, k, "forward", 4)
            assert want[0].size > 100 and same_sig(e.signature(pl), want)
        tc, _, f1 = e.finish(counters=True)
    wc, wf1 = sm.model_sketch(rs, ["1" * k for k in klist], sm.FORWARD, R, 4)
    assert np.array_equal(f1, wf1) and np.array_equal(tc, wc)


# ---- 7. routes ----
def test_tiled_batches_are_relaid_out(nt):
    want = sig_model.equal_model(32, "canonical", 7)
    tiles = torch.from_numpy(nt.tile_reads(reads(), 150)).cuda()
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e:
        e.submit_tiled_device(tiles.data_ptr(), 320, 150)
        assert same_sig(e.signature(), want) and want[0].size == 593
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        with pytest.raises(nt.NtcError) as ei:
            e.submit_tiled_device(tiles.data_ptr(), 320, 150)
        assert ei.value.code == ERR_ARG
        h, c = e.signature()
        assert h.size == 0 and c.size == 0 and e.signature_size() == 0
        assert int(e.finish()[2][0]) == 0


def test_ragged_and_binned_tiled_device_batches_are_relaid_out(nt):
    """a canonical plain-k signature engine has no tiled plane: its ragged tiled batches and bins go through the re-layout to K1 like a strand engine's"""
    rag = sm.sketch_reads_ragged()
    assert min(len(r) for r in rag) >= 145 and max(len(r) for r in rag) <= 160 and len(set(len(r) for r in rag)) > 5  # one bin of 10 chunks
    tiles, tails, order = nt.tile_reads_ragged(rag, 10)
    d_tiles, d_tails = torch.from_numpy(tiles).cuda(), torch.from_numpy(tails.view(np.int32).copy()).cuda()
    eq = torch.from_numpy(nt.tile_reads(reads(), 150)).cuda()
    want_rag = sig_model.model(rag, 32, "canonical", 4)
    want_both = sig_model.model(rag + reads(), 32, "canonical", 4)
    assert want_rag[0].size > 3000 and want_both[0].size > want_rag[0].size
    with nt.Engine([32], r_bits=R, s_bits=4, signature=True) as e, nt.Engine([32], r_bits=R, s_bits=4) as plain:
        e.submit_tiled_ragged_device(d_tiles.data_ptr(), len(rag), 10, d_tails.data_ptr())
        assert same_sig(e.signature(), want_rag)
        e.reset()
        e.submit_tiled_bins_device([(eq.data_ptr(), 320, 150, 0), (d_tiles.data_ptr(), len(rag), 160, d_tails.data_ptr())])
        plain.submit_reads(rag + reads())  # (without the flag a canonical engine at sBits 4 refuses ragged tiles, as before: it gets the reads from the host)
        assert same_sig(e.signature(), want_both)
        tc, _, f1 = e.finish(counters=True)
        tc0, _, f10 = plain.finish(counters=True)
        oc, of1 = orc.sketch_reads(rag + reads(), [32], 0, R, 4)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc) and np.array_equal(f1, f10) and np.array_equal(tc, tc0)
    with nt.Engine([32], r_bits=R, s_bits=4, signature=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        with pytest.raises(nt.NtcError) as ei:
            e.submit_tiled_ragged_device(d_tiles.data_ptr(), len(rag), 10, d_tails.data_ptr())
        assert ei.value.code == ERR_ARG and e.signature_size() == 0


def test_ragged_host_reads(nt):
    rs = sm.sketch_reads_ragged()
    want = sig_model.model(rs, 32, "canonical", 4)
    assert want[0].size > 3000
    with nt.Engine([32], r_bits=R, s_bits=4, signature=True) as e:
        e.submit_reads(rs)
        assert same_sig(e.signature(), want)


@functools.lru_cache(maxsize=None)
def long_set():
    import random
    rng = random.Random(77)
    return (sm.rseq(rng, 5000, pn=0.001),), (sm.rseq(rng, 5000, pn=0.001), sm.rseq(rng, 31), sm.rseq(rng, 2500), b"", sm.rseq(rng, 32))


def test_one_long_read_through_the_chunked_row_slots(nt):
    one, _ = long_set()
    want = sig_model.model(one, 32, "canonical", 3)
    assert int(want[1].sum()) > 500
    with nt.Engine([32], r_bits=R, s_bits=3, signature=True) as e:
        e.submit_reads(list(one))
        assert same_sig(e.signature(), want)  # every window once: the chunks' overlaps are not counted twice
        assert int(e.finish()[2][0]) == orc.hash_read(one[0], 32)[0].size


def test_long_device_takes_the_gather_route(nt):
    _, seqs = long_set()
    want = sig_model.model(seqs, 32, "canonical", 3)
    assert int(want[1].sum()) > 800
    d, offs = on_device(seqs, lead=2)
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e7, nt.Engine([32], r_bits=R, s_bits=3, signature=True) as e:
        for eng in (e7, e):
            eng.submit_long_device(d.data_ptr(), offs)
            assert eng.long_stats() == (0, 0)
        assert same_sig(e.signature(), want)
        assert same_sig(e7.signature(), sig_model.model(seqs, 32, "canonical", 7))


# ---- 8. the container on chosen keys ----
@functools.lru_cache(maxsize=None)
def chosen():
    rng = np.random.default_rng(11)
    base = rng.integers(1, 2**64, size=45000, dtype=np.uint64)
    keys = np.concatenate([base, rng.choice(base, size=5000)])
    rng.shuffle(keys)
    keys.setflags(write=False)
    return keys


def test_inject_host_and_device(nt, monkeypatch):
    monkeypatch.setenv("NTC_SIG_SLOTS", "64")
    keys = chosen()
    wh, wc = np.unique(keys, return_counts=True)
    assert keys.size == 50000 and 45000 - 10 <= wh.size <= 45000 and int(wc.max()) >= 2 and not np.any(keys == 0)
    d = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as eh, nt.Engine([32], r_bits=R, s_bits=7, signature=True) as ed:
        eh.signature_inject(keys)
        ed.signature_inject((d.data_ptr(), keys.size), device=True)
        for e in (eh, ed):
            assert same_sig(e.signature(), (wh, wc))
            slots, grows = e.signature_stats()
            assert slots >= 2 * wh.size and grows >= 10
        # zeros are skipped, counts add up
        with_zeros = np.concatenate([np.zeros(3, np.uint64), wh[:100], np.zeros(1, np.uint64)])
        cnt = np.arange(1, 105, dtype=np.uint32)
        eh.signature_inject(with_zeros, cnt)
        dz, dc = torch.from_numpy(with_zeros.view(np.int64).copy()).cuda(), torch.from_numpy(cnt.view(np.int32).copy()).cuda()
        ed.signature_inject((dz.data_ptr(), with_zeros.size), dc.data_ptr(), device=True)
        wc2 = wc.copy()
        wc2[:100] += np.arange(4, 104)
        for e in (eh, ed):
            assert same_sig(e.signature(), (wh, wc2))
        assert int(eh.finish()[2][0]) == 0  # inject touches neither F1 nor t_Counter
        assert int(eh.finish(counters=True)[0].sum()) == 0


def test_counts_saturate(nt):
    key = np.array([0x0123456789abcdef, 5], dtype=np.uint64)
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e:
        e.signature_inject(key, np.array([2**32 - 2, 2**31 - 1], dtype=np.uint32))
        for _ in range(3):
            e.signature_inject(key[:1])
        e.signature_inject(np.array([5, 5, 5], dtype=np.uint64))  # (a count at 2^31 and beyond takes the saturating path of the count-less insert too)
        h, c = e.signature()
        assert h.tolist() == [5, 0x0123456789abcdef] and c.tolist() == [2**31 + 2, 2**32 - 1]
        e.signature_inject(key[:1], np.array([2**32 - 1], dtype=np.uint32))
        assert e.signature()[1].tolist() == [2**31 + 2, 2**32 - 1]


def test_inject_then_submit_adds_up(nt):
    want = sig_model.equal_model(32, "canonical", 7)
    extra = np.array([3, int(want[0][10]), int(want[0][10]), int(want[0][-1])], dtype=np.uint64)
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e:
        e.signature_inject(extra)
        submit_slots(e, sig_model.equal_reads())
        h, c = e.signature()
        wc = want[1].copy()
        wc[10] += 2
        wc[-1] += 1
        assert np.array_equal(h, np.concatenate([[np.uint64(3)], want[0]])) and np.array_equal(c.astype(np.int64), np.concatenate([[1], wc]))


# ---- 9. lifecycle ----
def test_reset_empties(nt, monkeypatch):
    monkeypatch.setenv("NTC_SIG_SLOTS", "128")
    want = sig_model.equal_model(32, "canonical", 7)
    with nt.Engine([32], r_bits=R, s_bits=7, signature=True) as e:
        submit_slots(e, sig_model.equal_reads())
        e.reset()  # (with the values still in the log)
        assert e.signature_size() == 0 and e.signature_stats() == (128, 0)
        submit_slots(e, sig_model.equal_reads())
        assert same_sig(e.signature(), want)
        assert e.signature_stats()[1] >= 4
        e.reset()
        assert e.signature()[0].size == 0 and e.signature_stats() == (128, 0)
        submit_slots(e, sig_model.equal_reads())
        assert same_sig(e.signature(), want)


def test_merge_devices(nt):
    rs = reads()
    a, b = rs[:200], rs[120:]
    want = sig_model.model(a + b, 32, "canonical", 4)
    assert int(want[1].max()) >= 2 and want[0].size > 2000
    with nt.Engine([32, 20], r_bits=R, s_bits=4, signature=True) as e0, nt.Engine([32, 20], r_bits=R, s_bits=4, signature=True) as e1, \
            nt.Engine([32, 20], r_bits=R, s_bits=4) as plain:
        e0.submit_reads(a)
        e1.submit_reads(b)
        with pytest.raises(nt.NtcError) as ei:
            nt.merge_devices([e0, plain])
        assert ei.value.code == ERR_ARG
        with pytest.raises(nt.NtcError):
            nt.merge_devices([plain, e1])
        nt.merge_devices([e0, e1])
        assert same_sig(e0.signature(0), want)
        assert same_sig(e0.signature(1), sig_model.model(a + b, 20, "canonical", 4))
        assert e1.signature_size(0) == 0 and e1.signature_size(1) == 0
        tc, _, f1 = e0.finish(counters=True)
        oc, of1 = orc.sketch_reads(a + b, [32, 20], 0, R, 4)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
