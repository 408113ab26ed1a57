"""GPU tests of long sequences under a k list (include/ntcard_hip.h: ntc_submit_long_device): ONE cut with the overlap of the largest k serves every
k of a list whose spread is at most 15 — a smaller k is launched with the trimmed read length L - (kmax - k) over the same tiles — and the cut kernel
derives every piece's offset from a per-sequence table.  Every comparison is exact, per k: F1 (counting a window of the overlap twice shows there at
once) and t_Counter against tests/orc.py.

The plan leaves a remainder of kmax - 1 .. L - 1 bytes behind the last full piece (tests/test_long_klist_host.py pins it), so a remainder of exactly
kmin - 1 or kmin bytes does not exist under a list with kmin < kmax - 1; the boundary set holds the remainders of kmax - 1 bytes (windows of the
smaller k only) and of kmax bytes, and whole sequences of kmin - 1 and kmin bytes."""
import functools
import random

import numpy as np
import pytest

import orc
from gpu_support import count_long, nt, on_device, planned  # noqa: F401
from support import assert_same_sketch, rseq_acgt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, S_BITS = 14, 7
PL = 48
LISTS = [(17, 32), (20, 26, 32), (12, 27)]  # spread 15 (L_17 = 33 = 2 x 16 + 1, S = 17); three k; kmax < 32 (S = 22)
INPUTS = ["one", "mixed", "short"]


def step_of(kl):
    return PL - max(kl) + 1


def one_long(kl):
    """one sequence of more than 2048 pieces (the cut crosses a tile boundary) whose remainder has windows of every k"""
    rng = random.Random(7)
    s = rseq_acgt(rng, PL + step_of(kl) * 2100 + 20)
    m = (len(s) - PL) // step_of(kl) + 1
    assert m > 2048 and len(s) - m * step_of(kl) >= max(kl)
    return (s,)


def mixed(kl):
    """about 40 sequences: every boundary length of the plan, non-base bytes in and around the overlap, a few of several thousand bases"""
    rng = random.Random(11)
    kmin, kmax, S = min(kl), max(kl), step_of(kl)
    lens = [0, kmin - 1, kmin, kmax - 1, kmax, PL - 1, PL, PL + S - 1, PL + S,
            5 * S + kmax - 1, 5 * S + kmax,  # m = 5 and a remainder of kmax - 1 bytes (windows of the smaller k only) / of kmax bytes
            9001, 15003, 17777, 12222, 2222] + [rng.randrange(1, 400) for _ in range(24)]
    for n in lens[9:11]:
        assert (n - PL) // S + 1 == 5
    seqs = [bytearray(rseq_acgt(rng, n)) for n in lens]
    big = seqs[11]
    # piece-relative positions just in front of the overlap [S, L), on its first byte, inside it and on its last byte, in different pieces
    for j, pos in enumerate([S - 2, S - 1, S, S + 1, (S + PL) // 2, PL - 2, PL - 1, kmin - 1, S + kmin - 1, PL - kmin]):
        big[(20 + 7 * j) * S + pos] = ord("N")
    big[4000:4005] = b"acgtn"  # lower case
    big[4500] = ord("U")
    big[5000] = ord("R")  # an IUPAC letter
    big[6000:6000 + PL + 12] = b"N" * (PL + 12)  # a run of N longer than a piece
    seqs[12][PL - 1] = ord("N")
    seqs[12][PL + 16] = ord("n")
    seqs[13][17776] = ord("N")
    seqs[14][0] = ord("N")
    for s in seqs[16:24]:
        if len(s) > 40:
            s[len(s) // 2] = ord("N")
    seqs = tuple(bytes(s) for s in seqs)
    assert any(int(o) % 4 for o in np.cumsum([3] + [len(s) for s in seqs]))
    assert sum((len(s) - PL) // S + 1 for s in seqs if len(s) >= PL) > 2048  # bounded scratch: a round ends inside a sequence
    return seqs


def many_short(kl):
    """1200 sequences of 1 - 3 pieces, every other one followed by a sequence without a piece: a 64-piece block of the cut spans dozens of sequences"""
    rng = random.Random(13)
    S = step_of(kl)
    seqs = []
    for i in range(1200):
        seqs.append(rseq_acgt(rng, PL + (rng.randrange(1, 4) - 1) * S + rng.randrange(0, S)))
        if i % 2:
            seqs.append(rseq_acgt(rng, rng.randrange(0, PL)))
        if i % 97 == 0:
            dirty = bytearray(seqs[-1])
            if dirty:
                dirty[len(dirty) // 2] = ord("N")
                seqs[-1] = bytes(dirty)
    return tuple(seqs)


@functools.lru_cache(maxsize=None)
def inputs(which, kl):
    return {"one": one_long, "mixed": mixed, "short": many_short}[which](kl)


@functools.lru_cache(maxsize=None)
def oracle(which, kl):
    return orc.sketch_reads(list(inputs(which, kl)), list(kl), 0, R, S_BITS)


@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_one_sequence_across_a_tile_boundary(nt, kl):
    seqs = inputs("one", kl)
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL)
    assert stats == (sum(nt.long_plan(max(kl), PL, len(s))[0] for s in seqs), 1)  # (0, 0) without the list route
    assert_same_sketch((tc, f1), oracle("one", kl), kl)


@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_many_sequences_every_boundary_length(nt, kl):
    seqs = inputs("mixed", kl)
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL)
    assert stats == planned(nt, map(len, seqs), max(kl), PL) and stats[0] > 0
    assert_same_sketch((tc, f1), oracle("mixed", kl), kl)


@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_many_short_sequences_in_one_block_of_the_cut(nt, kl):
    seqs = inputs("short", kl)
    assert sum(1 for s in seqs if len(s) >= PL) >= 200 and any(len(s) < PL for s in seqs)
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL)
    assert stats == planned(nt, map(len, seqs), max(kl), PL) and stats[1] == 1200
    assert_same_sketch((tc, f1), oracle("short", kl), kl)


@pytest.mark.parametrize("which", INPUTS)
@pytest.mark.parametrize("kl", LISTS, ids=str)
def test_several_rounds_of_bounded_scratch(nt, monkeypatch, kl, which):
    """NTC_LONG_ROUND_BYTES = 1: a round is one tile of pieces / 64 row slots; every input holds more than 2048 pieces, so a round begins inside a sequence"""
    monkeypatch.setenv("NTC_LONG_ROUND_BYTES", "1")
    seqs = inputs(which, kl)
    assert planned(nt, map(len, seqs), max(kl), PL)[0] > 2048
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL)
    assert stats == planned(nt, map(len, seqs), max(kl), PL)
    assert_same_sketch((tc, f1), oracle(which, kl), (kl, which))


@pytest.mark.parametrize("rounds", [False, True])
@pytest.mark.parametrize("which", INPUTS)
def test_one_k_on_the_same_inputs(nt, monkeypatch, which, rounds):
    """the engine [32] on the inputs of [17, 32] (the same cut): the sequence table on the single-k route"""
    if rounds:
        monkeypatch.setenv("NTC_LONG_ROUND_BYTES", "1")
    seqs = inputs(which, (17, 32))
    tc, f1, stats = count_long(nt, *on_device(seqs), (32,), PL)
    oc, of1 = oracle(which, (17, 32))
    assert stats == planned(nt, map(len, seqs), 32, PL)
    assert_same_sketch((tc, f1), (oc[1:], of1[1:]), which)


def test_require_tiled_accepts_a_list(nt):
    kl = (17, 32)
    seqs = inputs("mixed", kl)
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL, flags=nt.FLAG_REQUIRE_TILED)  # raises without the list route
    assert stats == planned(nt, map(len, seqs), max(kl), PL)
    assert_same_sketch((tc, f1), oracle("mixed", kl), kl)


def test_submits_accumulate_on_a_deferring_engine(nt):
    kl = (20, 26, 32)
    seqs = inputs("mixed", kl)
    oc, of1 = oracle("mixed", kl)
    want = planned(nt, map(len, seqs), max(kl), PL)
    tc, f1, stats = count_long(nt, *on_device(seqs), kl, PL, flags=nt.FLAG_DEFER_REDO, submits=2)
    assert stats == (2 * want[0], 2 * want[1])
    assert np.array_equal(f1, 2 * of1), (f1, of1)
    assert np.array_equal(tc, (2 * oc.astype(np.uint32)).astype(np.uint16))  # t_Counter wraps at 16 bits


def test_piece_length_below_kmax_plus_15_is_refused(nt):
    d, offs = on_device(inputs("mixed", (12, 27)))
    with nt.Engine([12, 27], r_bits=R, s_bits=S_BITS) as e:
        with pytest.raises(nt.NtcError) as ei:
            e.submit_long_device(d.data_ptr(), offs, 32)  # fine for k = 12 alone, below 27 + 15
        assert ei.value.code == -1
        assert not e.finish()[2].any() and e.long_stats() == (0, 0)


def test_host_batches_take_the_path_behind_NTC_LONG_MIN(nt, monkeypatch):
    kl = (20, 26, 32)
    rng = random.Random(3)
    seqs = list(inputs("mixed", kl)) + [rseq_acgt(rng, 150) for _ in range(3000)]
    want = orc.sketch_reads(seqs, list(kl), 0, R, S_BITS)
    buf = b"".join(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    starts = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.uint64))).astype(np.uint64)

    def run(spans):
        with nt.Engine(list(kl), r_bits=R, s_bits=S_BITS) as e:
            if spans:
                e.submit_spans(buf, starts, lens)
            else:
                e.submit_reads(seqs)
            tc, _, f1 = e.finish(counters=True)
            return tc, f1, e.long_stats()

    monkeypatch.delenv("NTC_LONG_MIN", raising=False)
    for spans in (False, True):
        tc, f1, stats = run(spans)
        assert_same_sketch((tc, f1), want, ("default", spans))
        assert stats == (0, 0)  # the default leaves host batches of this size on row slots
    monkeypatch.setenv("NTC_LONG_MIN", "1")
    for spans in (False, True):
        tc, f1, stats = run(spans)
        assert_same_sketch((tc, f1), want, ("NTC_LONG_MIN=1", spans))
        assert stats[0] > 0 and stats[1] == sum(1 for s in seqs if nt.long_plan(max(kl), 1008, len(s))[0] >= 2)
