"""GPU tests of every generated K1h body (ntcard_amd/csrc/gen_k1h.py: (k, gap) x sBits class x canonical / forward / reverse, 138 bodies) and of the sBits
range of the tiled pair, from the case table of tests/k1h_variant_cases.py alone: each case goes through ntc_submit_tiled_device on an engine with
NTC_FLAG_REQUIRE_TILED (and NTC_FLAG_STRAND_TILED for a strand), and t_Counter and F1 must equal the model's exactly — the C oracle for a canonical case,
tests/strand_model.py's array form (pinned to the oracle's fh / rh in tests/test_strand_host.py) for a strand.  tests/test_k1h_variant_cases_host.py proves
that the cases cover the bodies and are not vacuous; tests/test_k1h_emulator.py and tests/test_k1h_strand_emulator.py run the same bodies on the CPU."""
import numpy as np
import pytest

import k1h_variant_cases as vc
import strand_model as sm
from gpu_support import count_long, dev, nt, on_device, planned  # noqa: F401
from support import assert_same_sketch, tile_array

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ONE = [sm.FORWARD, sm.REVERSE]


def flags_of(nt, strand, extra=0, require=True):
    f = {sm.CANONICAL: 0, sm.FORWARD: nt.FLAG_STRAND_FORWARD | nt.FLAG_STRAND_TILED, sm.REVERSE: nt.FLAG_STRAND_REVERSE | nt.FLAG_STRAND_TILED}[strand]
    return f | (nt.FLAG_REQUIRE_TILED if require else 0) | extra


def engine(nt, c, extra=0, require=True):
    e = nt.Engine([c.k], gap=c.gap, r_bits=c.r_bits, s_bits=c.s_bits, flags=flags_of(nt, c.strand, extra, require))
    e.set_profiling(True)
    return e


def tiles_of(c):
    """the case's equal-length reads in the tiled layout, on the device"""
    arr = vc.reads_of(c)
    assert arr.shape == (c.n, c.L) and not (arr == ord("#")).any()
    return dev(tile_array(arr))


def run_tiled(nt, c):
    t = tiles_of(c)
    with engine(nt, c) as e:
        e.submit_tiled_device(t.data_ptr(), c.n, c.L)
        got = e.finish(counters=True)
        ms, launches = e.kernel_time()
        assert ms > 0.0 and launches >= 1, (ms, launches)  # a hash launch happened (K1h: the engine requires the tiled pair)
    return got


@pytest.mark.parametrize("c", vc.GPU_BODY_CASES, ids=vc.case_id)
def test_every_body(nt, c):
    assert_same_sketch(run_tiled(nt, c), vc.want(c), vc.case_id(c), nonempty=True)


@pytest.mark.parametrize("c", vc.RANGE_CASES + vc.PLANT_CASES, ids=vc.case_id)
def test_s_bits_up_to_the_table_word(nt, c):
    """sBits 13, 16, 20 and 24: up to 17 extra hash bits above the counter index in K1h's table word (build_k1h_table), which the resolve pass and K1f's
    verdict on a suspect test; sBits 20 at r_bits 18 and sBits 24 at r_bits 14 fill the 32 bits.  At sBits 24 the hits are planted windows
    (k1h_variant_cases.planted_reads): clean ones, suspects beside an N, and windows over an N, which must not count"""
    assert c.r_bits + 1 + c.s_bits - 7 <= 32
    assert_same_sketch(run_tiled(nt, c), vc.want(c), vc.case_id(c), nonempty=True)


@pytest.mark.parametrize("c", vc.REFUSE_CASES, ids=vc.case_id)
def test_one_bit_beyond_the_table_word_is_refused(nt, c):
    """r_bits + 1 + (s_bits - 7) = 33: NTC_FLAG_REQUIRE_TILED refuses the submit before any launch and counts nothing; without the flag the general kernel
    counts the same planted reads"""
    assert c.r_bits + 1 + c.s_bits - 7 == 33
    t = tiles_of(c)
    with engine(nt, c) as e:
        with pytest.raises(nt.NtcError, match="REQUIRE_TILED") as ei:
            e.submit_tiled_device(t.data_ptr(), c.n, c.L)
        assert ei.value.code == -1
        tc, _, f1 = e.finish(counters=True)
        assert not f1.any() and not tc.any() and e.kernel_time()[1] == 0
    with engine(nt, c, require=False) as e:
        e.submit_tiled_device(t.data_ptr(), c.n, c.L)
        assert_same_sketch(e.finish(counters=True), vc.want(c), vc.case_id(c), nonempty=True)
        assert e.kernel_time()[1] >= 1


@pytest.mark.parametrize("c", vc.RAGGED_CASES, ids=vc.case_id)
def test_ragged_batch_and_deferred_fixups(nt, c):
    """k = 23, a body tests/test_strand_tiled_gpu.py does not run: a ragged batch (ntc_submit_tiled_ragged_device) behind the equal-length batch of the same
    body, with K1f after every launch and with NTC_FLAG_DEFER_REDO (one K1f over both launches)"""
    equal = next(b for b in vc.GPU_BODY_CASES if vc.body_of(b) == vc.body_of(c) and b.s_bits == c.s_bits and b.r_bits == c.r_bits and b.p_bad > 0)
    reads = vc.ragged_list(vc.reads_of(c))
    tiles, tails, _ = nt.tile_reads_ragged(reads, c.L // 16)
    dt, dl, de = dev(tiles), dev(tails), tiles_of(equal)
    (wt, wf), (et, ef) = vc.want(c), vc.want(equal)
    for extra in (0, nt.FLAG_DEFER_REDO):
        with engine(nt, c, extra) as e:
            e.submit_tiled_device(de.data_ptr(), equal.n, equal.L)
            e.submit_tiled_ragged_device(dt.data_ptr(), c.n, c.L // 16, dl.data_ptr())
            assert_same_sketch(e.finish(counters=True), (wt + et, wf + ef), (vc.case_id(c), extra), nonempty=True)
            assert e.kernel_time()[1] >= 2


@pytest.mark.parametrize("c", vc.SHORT_READ_CASES, ids=vc.case_id)
def test_many_tiles_per_team_short_reads(nt, c):
    """the one-strand form of tests/test_tiled_gpu.py::test_tiled_many_tiles_per_team_short_reads: 3.2 M reads of 1 .. 2 chunks with 1.5 % non-base bytes, so
    every team of waves walks several tiles and the dirty-piece queue's tile tags, the suspects' tile tags and the ring phase wrap within one launch"""
    assert_same_sketch(run_tiled(nt, c), vc.want(c), vc.case_id(c), nonempty=True)


@pytest.mark.parametrize("strand", ONE, ids=["forward", "reverse"])
def test_long_sequences_under_a_k_list(nt, strand):
    """ntc_submit_long_device on the shared cut: k = 13, 19, 28 (class-8 bodies no other long-sequence test runs) over pieces of 272 bases at sBits 8"""
    seqs = vc.long_seqs()
    arr = sm.pad_reads(seqs)
    sk = [sm.array_sketches(arr, "1" * k, [(strand, vc.LONG_R_BITS, vc.LONG_S_BITS)])[strand, vc.LONG_R_BITS, vc.LONG_S_BITS] for k in vc.LONG_KLIST]
    want = np.concatenate([s[0] for s in sk]), np.concatenate([s[1] for s in sk])
    d, offs = on_device(seqs)
    tc, f1, stats = count_long(nt, d, offs, vc.LONG_KLIST, vc.LONG_PIECE, flags=flags_of(nt, strand), r_bits=vc.LONG_R_BITS, s_bits=vc.LONG_S_BITS)
    assert_same_sketch((tc, f1), want, ("long", strand), nonempty=True)
    assert stats == planned(nt, map(len, seqs), max(vc.LONG_KLIST), vc.LONG_PIECE) and stats[0] > 0
