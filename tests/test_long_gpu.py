"""GPU tests of long sequences on the tiled kernels (include/ntcard_hip.h: ntc_submit_long_device, ntc_long_stats): the device-side cut into pieces,
the gather of remainders and short sequences, engines that do not qualify, the host path behind NTC_LONG_MIN.  Every comparison is exact, against
tests/orc.py or against ntc_submit on the same sequences."""
import functools
import random

import numpy as np
import pytest

import orc
from gpu_support import count_long, nt, on_device, planned  # noqa: F401
from support import rseq_acgt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, S_BITS = 14, 7
K, PL = 32, 48  # piece_len 48 at k = 32: S = 17 window starts per piece
STEP = PL - K + 1


@functools.lru_cache(maxsize=None)
def one_long():
    """one sequence of more than 2048 pieces (the cut crosses a tile boundary) whose remainder has windows"""
    rng = random.Random(7)
    return (rseq_acgt(rng, PL + STEP * 2100 + 20),)


@functools.lru_cache(maxsize=None)
def mixed():
    """about 40 sequences: every boundary length of the plan, dirty bytes, a few of several thousand bases"""
    rng = random.Random(11)
    lens = [0, K - 1, K, PL - 1, PL, PL + STEP - 1, PL + STEP, 5 * STEP + K - 1,  # (the last: m = 5 and a remainder of exactly k - 1 bytes — no window)
            3001, 5003, 7777, 2222] + [rng.randrange(1, 400) for _ in range(28)]
    seqs = [bytearray(rseq_acgt(rng, n)) for n in lens]
    assert 5 * STEP + K - 1 >= PL and (5 * STEP + K - 1 - PL) // STEP + 1 == 5
    big = seqs[8]
    big[100] = ord("N")
    big[500:505] = b"acgtn"
    big[900] = ord("U")
    big[1200] = ord("R")
    big[2000:2000 + PL + 12] = b"N" * (PL + 12)  # a run of N longer than a piece
    seqs[9][47] = ord("N")
    seqs[9][48 + 16] = ord("n")
    seqs[10][7776] = ord("N")
    for s in seqs[12:20]:
        if len(s) > 40:
            s[len(s) // 2] = ord("N")
    seqs = tuple(bytes(s) for s in seqs)
    offs = np.cumsum([3] + [len(s) for s in seqs])
    assert any(int(o) % 4 for o in offs)
    return seqs


@functools.lru_cache(maxsize=None)
def oracle(which, k=K, gap=0):
    seqs = {"one": one_long, "mixed": mixed}[which]()
    return orc.sketch_reads(list(seqs), [k], gap, R, S_BITS)


def test_one_sequence_across_a_tile_boundary(nt):
    """48 + 17 * 2100 + 20 bases at piece_len 48, k = 32.  ntc_long_plan's m = floor((n - L) / S) + 1 gives 2102 full pieces for this length (the 20 bases
    behind piece 2100 hold one more step of 17) and a remainder of 34 bytes = 3 windows; the stats are checked against the plan."""
    seqs = one_long()
    assert planned(nt, map(len, seqs), K, PL) == (2102, 1) and len(seqs[0]) - 2102 * STEP >= K
    tc, f1, stats = count_long(nt, *on_device(seqs), [K], PL)
    oc, of1 = oracle("one")
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
    assert stats == (2102, 1)


def test_many_sequences_every_boundary_length(nt):
    seqs = mixed()
    tc, f1, stats = count_long(nt, *on_device(seqs), [K], PL)
    oc, of1 = oracle("mixed")
    assert np.array_equal(f1, of1), (f1, of1)
    assert np.array_equal(tc, oc)
    assert stats == planned(nt, map(len, seqs), K, PL) and stats[0] > 0


def test_several_rounds_of_bounded_scratch(nt, monkeypatch):
    """NTC_LONG_ROUND_BYTES = 1: a round is one tile of pieces / 64 row slots, so both inputs take several"""
    monkeypatch.setenv("NTC_LONG_ROUND_BYTES", "1")
    for which, seqs in (("one", one_long()), ("mixed", mixed())):
        tc, f1, stats = count_long(nt, *on_device(seqs), [K], PL)
        oc, of1 = oracle(which)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc), which
        assert stats == planned(nt, map(len, seqs), K, PL)


@pytest.mark.parametrize("k,gap,pl", [(12, 2, 32), (32, 8, 64)])
def test_tiled_gap_seeds(nt, k, gap, pl):
    seqs = mixed()
    tc, f1, stats = count_long(nt, *on_device(seqs), [k], pl, gap=gap, flags=nt.FLAG_REQUIRE_TILED)
    oc, of1 = oracle("mixed", k, gap)
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
    assert stats == planned(nt, map(len, seqs), k, pl) and stats[0] > 0


def test_engine_chooses_the_piece_length(nt):
    gen = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[gen.integers(0, 4, size=3_000_000)]
    seq[gen.integers(0, seq.size, size=50)] = ord("N")
    seqs = (seq.tobytes(),)
    tc, f1, stats = count_long(nt, *on_device(seqs), [K], 0)
    oc, of1 = orc.sketch_reads(list(seqs), [K], 0, R, S_BITS)
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
    assert stats[0] > 0 and stats[1] == 1


def test_piece_length_below_k_plus_15_is_refused(nt):
    d, offs = on_device(mixed())
    with nt.Engine([K], r_bits=R, s_bits=S_BITS) as e:
        with pytest.raises(nt.NtcError) as ei:
            e.submit_long_device(d.data_ptr(), offs, 32)
        assert ei.value.code == -1
        assert int(e.finish()[2][0]) == 0 and e.long_stats() == (0, 0)


def other_engines(nt):
    return {
        "k64": lambda **kw: nt.Engine([64], r_bits=R, s_bits=S_BITS, **kw),
        "list": lambda **kw: nt.Engine([16, 32], r_bits=R, s_bits=S_BITS, **kw),
        "forward": lambda **kw: nt.Engine([K], r_bits=R, s_bits=S_BITS, strand="forward", **kw),
        "mask": lambda **kw: nt.Engine.from_seeds(["1111111101111111100111111"], r_bits=R, s_bits=S_BITS, **kw),
    }


@pytest.mark.parametrize("name", ["k64", "list", "forward", "mask"])
def test_engines_that_do_not_qualify_count_like_submit(nt, name):
    make = other_engines(nt)[name]
    seqs = mixed()
    d, offs = on_device(seqs)
    with make() as e:
        e.submit_reads(list(seqs))
        want_tc, _, want_f1 = e.finish(counters=True)
    with make() as e:
        e.submit_long_device(d.data_ptr(), offs)
        tc, _, f1 = e.finish(counters=True)
        assert e.long_stats() == (0, 0)
    assert int(want_f1.sum()) > 0
    assert np.array_equal(f1, want_f1) and np.array_equal(tc, want_tc)
    with make(flags=nt.FLAG_REQUIRE_TILED) as e:
        with pytest.raises(nt.NtcError) as ei:
            e.submit_long_device(d.data_ptr(), offs)
        assert ei.value.code == -1
        assert not e.finish()[2].any()


def test_nthll_engine_counts_like_submit(nt):
    seqs = mixed()
    d, offs = on_device(seqs)
    with nt.HllEngine(K) as e:
        e.submit_reads(list(seqs))
        want_regs, want_f1 = e.finish()
    with nt.HllEngine(K) as e:
        e.submit_long_device(d.data_ptr(), offs)
        regs, f1 = e.finish()
        assert e.long_stats() == (0, 0)
    assert want_f1 > 0 and f1 == want_f1 and np.array_equal(regs, want_regs)


def test_host_batches_take_the_path_behind_NTC_LONG_MIN(nt, monkeypatch):
    rng = random.Random(3)
    seqs = list(mixed()) + [rseq_acgt(rng, 150) for _ in range(3000)]
    oc, of1 = orc.sketch_reads(seqs, [K], 0, R, S_BITS)
    buf = b"".join(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    starts = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.uint64))).astype(np.uint64)

    def run(spans):
        with nt.Engine([K], r_bits=R, s_bits=S_BITS) as e:
            if spans:
                e.submit_spans(buf, starts, lens)
            else:
                e.submit_reads(seqs)
            tc, _, f1 = e.finish(counters=True)
            return tc, f1, e.long_stats()

    monkeypatch.delenv("NTC_LONG_MIN", raising=False)
    for spans in (False, True):
        tc, f1, stats = run(spans)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
        assert stats == (0, 0)  # the default leaves host batches on row slots
    monkeypatch.setenv("NTC_LONG_MIN", "1")
    for spans in (False, True):
        tc, f1, stats = run(spans)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
        assert stats[0] > 0 and stats[1] == sum(1 for s in seqs if nt.long_plan(K, 1008, len(s))[0] >= 2)


def test_source_may_change_behind_the_call_on_a_deferring_engine(nt):
    seqs = mixed()
    d, offs = on_device(seqs)
    oc, of1 = oracle("mixed")
    with nt.Engine([K], r_bits=R, s_bits=S_BITS, flags=nt.FLAG_DEFER_REDO) as e:
        e.submit_long_device(d.data_ptr(), offs, PL)
        d.fill_(ord("N"))  # same stream, behind the call: the engine counts from its own scratch and never defers this work
        tc, _, f1 = e.finish(counters=True)
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)


def test_reset_zeroes_the_stats_and_submits_accumulate(nt):
    seqs = mixed()
    d, offs = on_device(seqs)
    oc, of1 = oracle("mixed")
    want = planned(nt, map(len, seqs), K, PL)
    with nt.Engine([K], r_bits=R, s_bits=S_BITS) as e:
        e.submit_long_device(d.data_ptr(), offs, PL)
        e.sync()
        assert e.long_stats() == want
        e.reset()
        assert e.long_stats() == (0, 0)
        e.submit_long_device(d.data_ptr(), offs, PL)
        e.submit_long_device(d.data_ptr(), offs, PL)
        tc, _, f1 = e.finish(counters=True)
        assert e.long_stats() == (2 * want[0], 2 * want[1])
    assert np.array_equal(f1, 2 * of1)
    assert np.array_equal(tc, (2 * oc.astype(np.uint32)).astype(np.uint16))  # t_Counter wraps at 16 bits
