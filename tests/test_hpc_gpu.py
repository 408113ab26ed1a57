"""GPU tests of homopolymer-compressed counting (include/ntcard_hip.h: NTC_FLAG_HPC, ntc_hpc_compress_device, ntc_hpc_stats): the device compaction
byte for byte against the pure-Python model (tests/hpc_model.py), and every engine result exactly against tests/orc.py (tests/strand_model.py for a
strand or a mask) run on the MODEL's output — never against anything the code under test produced.

The sequences (hpc_model.device_set) hold: empty and 1-byte sequences; neighbours that end and begin with the same base; a run of 70 000 x A with case
flips; runs of three that straddle the 4-, 64-, 256- and 4096-byte positions of the buffer for every lead 0 .. 3; TU / tU / aA pairs; an N run longer
than a piece; RR, CR, bytes 1 and 3; a sequence that compresses to one byte; 40 sequences of 1 .. 400 bytes; one of 300 000 bases whose runs have a
geometric length; an empty sequence at the very end."""
import functools

import numpy as np
import pytest

import hpc_model as hm
import orc
import strand_model as sm
from gpu_support import nt, on_device, planned  # noqa: F401
from support import same_sketch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, S_BITS = 14, 7
K, PL = 32, 48
MASK = "1111111101111111100111111"


def seqs():
    """what the engines count: the sequences of the compaction tests with the bytes 1, 3, 4, 5, 7 turned into other non-bases (hpc_model.engine_set says why)"""
    return hm.engine_set()


@functools.lru_cache(maxsize=None)
def comp():
    return tuple(hm.model(seqs()))


@functools.lru_cache(maxsize=None)
def device_input(lead=3, raw=False):
    """the sequences (raw: hpc_model.device_set, the bytes 1 and 3 included) on the device, uploaded once per lead -> (tensor, host offsets)"""
    return on_device(hm.device_set() if raw else seqs(), lead=lead)


@functools.lru_cache(maxsize=None)
def oracle(kl=(K,), gap=0):
    return orc.sketch_reads(list(comp()), list(kl), gap, R, S_BITS)


@functools.lru_cache(maxsize=None)
def oracle_raw():
    return orc.sketch_reads(list(seqs()), [K], 0, R, S_BITS)


@functools.lru_cache(maxsize=None)
def model_sketch(mask, strand):
    return sm.model_sketch(list(comp()), [mask], strand, R, S_BITS)


def totals():
    return sum(len(s) for s in seqs()), sum(len(c) for c in comp())


def planned_comp(nt, kmax, pl):
    return planned(nt, map(len, comp()), kmax, pl)


def count_device(e, piece_len=PL, lead=3):
    d, offs = device_input(lead)
    e.submit_long_device(d.data_ptr(), offs, piece_len)
    tc, _, f1 = e.finish(counters=True)
    return tc, f1


# ---- the compaction itself ----
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("out_lead", [0, 1, 2, 3])
def test_compress_device_matches_the_model(nt, lead, out_lead):
    d, offs = device_input(lead, raw=True)
    raw, want_seqs = hm.device_set(), hm.model(hm.device_set())
    assert any(1 in s and 3 in s for s in raw)
    total_in, total_out = totals()
    out = torch.full((total_in + 8,), 0x23, dtype=torch.uint8, device="cuda")
    new = nt.hpc_compress_device(d.data_ptr(), offs, out.data_ptr() + out_lead)
    want = hm.offsets_of(want_seqs)
    assert new.dtype == np.uint64 and np.array_equal(new, want)
    got = out.cpu().numpy()
    assert got[out_lead:out_lead + total_out].tobytes() == b"".join(want_seqs)
    assert np.all(got[:out_lead] == 0x23) and np.all(got[out_lead + total_out:] == 0x23)  # nothing written outside the result
    assert d.cpu().numpy()[lead:lead + total_in].tobytes() == b"".join(raw)  # the source is untouched


def test_compress_device_subrange_and_empty(nt):
    """a call may start in the middle of a buffer (offsets[0] != 0) and may hold nothing"""
    d, offs = device_input(2, raw=True)
    out = torch.zeros(400_000, dtype=torch.uint8, device="cuda")
    new = nt.hpc_compress_device(d.data_ptr(), offs[5:20], out.data_ptr())
    c = hm.model(hm.device_set())[5:19]
    assert np.array_equal(new, hm.offsets_of(c)) and out.cpu().numpy()[:int(new[-1])].tobytes() == b"".join(c)
    assert np.array_equal(nt.hpc_compress_device(d.data_ptr(), offs[1:3] * 0 + offs[1], out.data_ptr()), [0, 0])


# ---- the compaction beyond its kernels' thresholds (hpc_model.compress_many is the model: tests/test_hpc_host.py pins it to compress() per sequence) ----
def compress_on_device(nt, buf, offs, lead=3, out_lead=0):
    """the sequences [offs[i], offs[i + 1]) of buf through ntc_hpc_compress_device, `lead` bytes behind an aligned address: offsets and bytes against
    the model, nothing written outside the result -> the chunks of the compaction"""
    d, d_offs = on_device(buf, offs, lead)  # (at an address that is a multiple of 4: the source's phase in its dword is `lead`)
    assert int(offs[0]) == 0
    out = torch.full((buf.size + 8,), 0x23, dtype=torch.uint8, device="cuda")
    new = nt.hpc_compress_device(d.data_ptr(), d_offs, out.data_ptr() + out_lead)
    want, want_offs = hm.compress_many(buf, offs)
    assert 0 < want.size < buf.size
    assert np.array_equal(new, want_offs)
    got = out.cpu().numpy()
    assert np.array_equal(got[out_lead:out_lead + want.size], want)
    assert np.all(got[:out_lead] == 0x23) and np.all(got[out_lead + want.size:] == 0x23)
    return hm.chunks_of(lead, buf.size)


@pytest.mark.parametrize("lead", [0, 3])
def test_every_pair_of_byte_values_on_the_device(nt, lead):
    """hpc_class on all 256 values, in front of and behind every other: as one sequence and as 65536 sequences of two bytes"""
    compress_on_device(nt, *hm.pair_seq(), lead=lead)
    compress_on_device(nt, *hm.pair_seqs(), lead=lead, out_lead=1)
    want, want_offs = hm.pair_want()
    got, got_offs = hm.compress_many(*hm.pair_seqs())
    assert np.array_equal(got, want) and np.array_equal(got_offs, want_offs)  # (the model against the definition, pair by pair)


def test_more_sequences_than_threads_and_more_chunks_than_scan_threads(nt):
    buf, offs = hm.many_short()
    assert len(offs) > hm.SEQ_THREADS  # ntc_hpc.hip:261: the stride loops of hpc_mark_kernel and hpc_offsets_kernel take a second turn
    n_chunks = compress_on_device(nt, buf, offs)
    assert n_chunks > hm.SCAN_THREADS  # ntc_hpc.hip:117: per = 2, a thread of hpc_scan_kernel owns two chunks


@pytest.mark.parametrize("extra,chunks", [(0, 1024), (1, 1025), (5, 1025)])
def test_scan_at_one_chunk_per_thread_and_just_beyond(nt, extra, chunks):
    """lead + total = 4 194 304 + extra: 1024 chunks are the last size with one chunk per thread of the scan, 1025 the first with two (the last chunk then
    holds one or five positions); a run of G lies across the last 4096 positions, the chunk boundary at 4 194 304 and the join of two sequences"""
    lead = 3
    buf, offs = hm.three_seqs(4_194_304 - lead + extra)
    assert lead + buf.size == 4_194_304 + extra
    assert np.all((buf[-5000:] | 0x20) == ord("g")) and buf.size - 4096 < int(offs[2]) < buf.size
    n_chunks = compress_on_device(nt, buf, offs, lead=lead, out_lead=extra % 4)
    assert n_chunks == chunks and (n_chunks + 1023) // 1024 == (1 if extra == 0 else 2)  # ntc_hpc.hip:117


def test_scan_with_three_chunks_per_thread(nt):
    buf, offs = hm.few_large()
    n_chunks = compress_on_device(nt, buf, offs, lead=1, out_lead=2)
    per = (n_chunks + 1023) // 1024
    assert per == 3 and per * 1023 >= n_chunks  # ntc_hpc.hip:117-118: the trailing threads of the scan have no chunk


def test_engine_counts_many_short_sequences(nt):
    """Engine([12], hpc=True) on the 530 000 short sequences: a compaction beyond both thresholds, then — no compressed sequence holds a piece — a gather
    launch of more row slots than it has waves (ntc_long.hip:143), against the oracle run on the model's output"""
    buf, offs = hm.many_short()
    want, want_offs = hm.compress_many(buf, offs)
    lens = np.diff(want_offs).astype(np.int64)
    assert len(lens) > 8192 * 4 and lens.max() >= 12 and lens.max() < 1008  # every sequence a row slot, none a piece
    oc = np.zeros((1, 2, 1 << R), dtype=np.uint16)
    of1 = orc.sketch_update(oc, want, want_offs, [12], 0, R, S_BITS)
    assert int(of1[0]) > 0
    d, d_offs = on_device(buf, offs)
    with nt.Engine([12], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        e.submit_long_device(d.data_ptr(), d_offs)
        tc, _, f1 = e.finish(counters=True)
        assert e.hpc_stats() == (buf.size, want.size) and e.long_stats() == (0, 0)
    assert np.array_equal(f1, of1), (f1, of1)
    assert np.array_equal(tc, oc)


# ---- engines that qualify for the cut ----
def test_k32(nt):
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        got = count_device(e)
        assert same_sketch(got, oracle()), (got[1], oracle()[1])
        assert e.hpc_stats() == totals()
        assert e.long_stats() == planned_comp(nt, K, PL) and e.long_stats()[0] > 2048
    assert not np.array_equal(oracle()[1], oracle_raw()[1])  # (the inputs tell the flag from its absence)


def test_table_slot_bytes_inside_the_pieces(nt):
    """the bytes 1 and 3 where the tiled kernels alone see them (no window of a remainder holds one): bases to the reference, kept by the compression,
    counted as the oracle counts them"""
    raw = hm.slot_piece_set(K, PL)
    c = hm.model(raw)
    assert all(1 in s or 3 in s for s in c)
    d, offs = on_device(raw, lead=1)
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_long_device(d.data_ptr(), offs, PL)
        tc, _, f1 = e.finish(counters=True)
        assert e.long_stats()[1] == len(raw)
    assert same_sketch((tc, f1), orc.sketch_reads(c, [K], 0, R, S_BITS))


def test_k_list_on_one_cut(nt):
    kl = (21, 25, 31)
    with nt.Engine(list(kl), r_bits=R, s_bits=S_BITS, hpc=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        assert same_sketch(count_device(e), oracle(kl))
        assert e.hpc_stats() == totals() and e.long_stats() == planned_comp(nt, 31, PL)


@pytest.mark.parametrize("k,gap,pl", [(12, 2, 32), (32, 8, 64)])
def test_tiled_gap_seeds(nt, k, gap, pl):
    with nt.Engine([k], gap=gap, r_bits=R, s_bits=S_BITS, hpc=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        assert same_sketch(count_device(e, pl), oracle((k,), gap))
        assert e.hpc_stats() == totals() and e.long_stats() == planned_comp(nt, k, pl)


def test_forward_strand_on_the_tiled_kernels(nt):
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True, strand="forward", strand_tiled=True, flags=nt.FLAG_REQUIRE_TILED) as e:
        assert same_sketch(count_device(e), model_sketch("1" * K, sm.FORWARD))
        assert e.hpc_stats() == totals() and e.long_stats() == planned_comp(nt, K, PL)


# ---- engines that do not ----
def other_engines(nt):
    return {
        "k64": (lambda **kw: nt.Engine([64], r_bits=R, s_bits=S_BITS, **kw), lambda: oracle((64,))),
        "list": (lambda **kw: nt.Engine([16, 32], r_bits=R, s_bits=S_BITS, **kw), lambda: oracle((16, 32))),
        "mask": (lambda **kw: nt.Engine.from_seeds([MASK], r_bits=R, s_bits=S_BITS, **kw), lambda: model_sketch(MASK, sm.CANONICAL)),
    }


@pytest.mark.parametrize("name", ["k64", "list", "mask"])
def test_engines_that_do_not_qualify(nt, name):
    make, want = other_engines(nt)[name]
    with make(hpc=True) as e:
        e.submit_reads(list(seqs()))
        host = e.finish(counters=True)
        host = (host[0], host[2])
        assert e.hpc_stats() == totals()
    with make(hpc=True) as e:
        dev = count_device(e, 0)
        assert e.long_stats() == (0, 0) and e.hpc_stats() == totals()
    assert int(want()[1].sum()) > 0
    assert same_sketch(dev, host) and same_sketch(dev, want())


# ---- the host path ----
@pytest.mark.parametrize("long_min", [None, "1"])
def test_host_submits(nt, monkeypatch, long_min):
    if long_min is None:
        monkeypatch.delenv("NTC_LONG_MIN", raising=False)
    else:
        monkeypatch.setenv("NTC_LONG_MIN", long_min)
    s = list(seqs())
    buf = b"".join(s)
    lens = np.array([len(x) for x in s], dtype=np.uint32)
    starts = hm.offsets_of(s)[:-1]
    for spans in (False, True):
        with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
            if spans:
                e.submit_spans(buf, starts, lens)
            else:
                e.submit_reads(s)
            tc, _, f1 = e.finish(counters=True)
            assert same_sketch((tc, f1), oracle()), spans
            assert e.hpc_stats() == totals()
            if long_min is not None:  # the compressed sequences of two or more default pieces are cut on the device
                assert e.long_stats()[1] == sum(1 for c in comp() if nt.long_plan(K, 1008, len(c))[0] >= 2) > 0


def test_one_sequence_per_round(nt, monkeypatch):
    monkeypatch.setenv("NTC_HPC_ROUND_BYTES", "1")
    monkeypatch.setenv("NTC_LONG_ROUND_BYTES", "1")
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        assert same_sketch(count_device(e), oracle())
        assert e.hpc_stats() == totals() and e.long_stats() == planned_comp(nt, K, PL)


def test_rounds_of_several_sequences(nt, monkeypatch):
    """a budget that ends rounds between the short sequences and leaves the long ones rounds of their own (the scratch grows to them)"""
    monkeypatch.setenv("NTC_HPC_ROUND_BYTES", "1000")
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        assert same_sketch(count_device(e), oracle())
        assert e.hpc_stats() == totals() and e.long_stats() == planned_comp(nt, K, PL)


def test_nthll(nt):
    with nt.HllEngine(K, hpc=True) as e:
        d, offs = device_input(3)
        e.submit_long_device(d.data_ptr(), offs)
        regs, f1 = e.finish()
        assert e.hpc_stats() == totals()
    with nt.HllEngine(K, hpc=True) as e:
        e.submit_reads(list(seqs()))
        regs_h, f1_h = e.finish()
    with nt.HllEngine(K) as e:
        e.submit_reads(list(comp()))
        want_regs, want_f1 = e.finish()
        assert e.hpc_stats() == (0, 0)
    assert want_f1 == int(oracle()[1][0]) > 0
    assert f1 == want_f1 and np.array_equal(regs, want_regs)
    assert f1_h == want_f1 and np.array_equal(regs_h, want_regs)
    assert np.array_equal(want_regs, orc.hll_reads(list(comp()), K, 16)[0])


def test_source_may_change_behind_the_call_on_a_deferring_engine(nt):
    d0, offs = device_input(3)
    d = d0.clone()
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True, flags=nt.FLAG_DEFER_REDO) as e:
        e.submit_long_device(d.data_ptr(), offs, PL)
        d.fill_(ord("N"))  # same stream, behind the call: the engine counts from its own scratch
        tc, _, f1 = e.finish(counters=True)
    assert same_sketch((tc, f1), oracle())


def test_fixed_layout_batches_are_refused(nt):
    reads = [c[:150] for c in comp() if len(c) >= 150][:4] * 16
    slots = torch.from_numpy(np.frombuffer(b"".join(r + b"AA" for r in reads), dtype=np.uint8).copy()).cuda()
    tiles = torch.from_numpy(nt.tile_reads(reads, 150)).cuda()
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        for call in (lambda: e.submit_device(slots.data_ptr(), len(reads), 150, 152), lambda: e.submit_tiled_device(tiles.data_ptr(), len(reads), 150),
                     lambda: e.submit_tiled_bins_device([(tiles.data_ptr(), len(reads), 150, 0)])):
            with pytest.raises(nt.NtcError) as ei:
                call()
            assert ei.value.code == -1 and "NTC_FLAG_HPC" in str(ei.value)
        assert int(e.finish()[2][0]) == 0 and e.hpc_stats() == (0, 0)


def test_reset_zeroes_the_stats_and_submits_accumulate(nt):
    d, offs = device_input(3)
    t_in, t_out = totals()
    oc, of1 = oracle()
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as e:
        e.set_profiling(True)
        e.submit_long_device(d.data_ptr(), offs, PL)
        e.sync()
        assert e.hpc_stats() == (t_in, t_out) and e.hpc_time() > 0.0
        e.reset()
        assert e.hpc_stats() == (0, 0) and e.hpc_time() == 0.0
        e.submit_long_device(d.data_ptr(), offs, PL)
        e.submit_reads(list(seqs()))
        tc, _, f1 = e.finish(counters=True)
        assert e.hpc_stats() == (2 * t_in, 2 * t_out)
    assert np.array_equal(f1, 2 * of1)
    assert np.array_equal(tc, (2 * oc.astype(np.uint32)).astype(np.uint16))  # t_Counter wraps at 16 bits


def test_merge_refuses_engines_that_differ_in_the_flag(nt):
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as a, nt.Engine([K], r_bits=R, s_bits=S_BITS) as b:
        with pytest.raises(nt.NtcError) as ei:
            nt.merge_devices([a, b])
        assert ei.value.code == -1
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as a, nt.Engine([K], r_bits=R, s_bits=S_BITS, hpc=True) as b:
        a.submit_reads(list(seqs()[:30]))
        b.submit_reads(list(seqs()[30:]))
        nt.merge_devices([a, b])
        tc, _, f1 = a.finish(counters=True)
    assert same_sketch((tc, f1), oracle())


def test_an_engine_without_the_flag_is_unchanged(nt):
    with nt.Engine([K], r_bits=R, s_bits=S_BITS) as e:
        assert same_sketch(count_device(e), oracle_raw())
        assert e.hpc_stats() == (0, 0) and e.hpc_time() == 0.0
