"""GPU tests of the device re-layout kernels in front of the tiled kernels (ntc_long.hip: cut_tiles_kernel, gather_slots_kernel) on the paths the other
long-sequence tests never enter: pieces of several 256-byte runs with a sequence table of many entries (piece lengths 256 .. 65520), the 64-way table search
at and beyond its second and third step (64 / 65 and 4096 / 4097 sequences with a full piece), and a gather launch of more row slots than its grid has
waves (more than 32768).  Every comparison is exact: F1 and t_Counter against tests/orc.py, ntc_long_stats against ntc_long_plan.  Every test asserts
that its input is beyond the threshold it is there for."""
import functools

import numpy as np
import pytest

import limits_model as lm
import orc
from gpu_support import count_long, nt, on_device, planned  # noqa: F401
from support import assert_same_sketch, offsets_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, S_BITS, K = 14, 7, 32
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CUT_RUN = 16  # chunks of a piece one workgroup of cut_tiles_kernel moves (ntc_long.hip:13)


def sketch(buf, offs, kl):
    counters = np.zeros((len(kl), 2, 1 << R), dtype=np.uint16)
    f1 = orc.sketch_update(counters, buf if buf.size else np.zeros(1, dtype=np.uint8), offs, list(kl), 0, R, S_BITS)
    return counters, f1


same = functools.partial(assert_same_sketch, nonempty=True)  # (the oracle counted something in every plane)


# ---- piece lengths of several runs ----
PIECES = (256, 272, 1008, 4096, 65520)


def boundary_lengths(pl):
    """the lengths at which ntc_long_plan(32, pl, .) changes: one byte short of a piece, a piece, one byte short of a second piece, two pieces, and a remainder
    of k - 1 (no window) and of k bytes (one window) behind 2 and 3 pieces"""
    S = pl - (K - 1)
    return [pl - 1, pl, pl + S - 1, pl + S, 2 * S + K - 1, 2 * S + K, 3 * S + K - 1, 3 * S + K]


@functools.lru_cache(maxsize=None)
def piece_input(pl):
    """-> (buf, offs): the boundary lengths clean, with N around the overlap of the pieces, and in lower case with U; three random sequences of 3 .. 6 pieces
    with N, lower case and a run of N longer than a step (at 65520: the clean boundary lengths only, a megabyte)"""
    rng = np.random.default_rng(pl)
    S = pl - (K - 1)
    seqs = []
    for variant in range(1 if pl == 65520 else 3):
        for n in boundary_lengths(pl):
            s = ACGT[rng.integers(0, 4, size=n)]
            if variant == 1:  # the last byte in front of the overlap [S, pl) of the first piece, its first and last byte, the byte behind it
                for pos in (S - 1, S, pl - 1, pl, 2 * S - 1, 2 * S):
                    if pos < n and rng.random() < 0.7:
                        s[pos] = lm.N
            if variant == 2:
                s = np.frombuffer(b"acgtuACGTU", dtype=np.uint8)[rng.integers(0, 10, size=n)]
            seqs.append(s)
    if pl != 65520:
        for m in (3, 4, 6):
            n = pl + (m - 1) * S + int(rng.integers(0, S))
            s = ACGT[rng.integers(0, 4, size=n)]
            s[rng.integers(0, n, size=6)] = lm.N
            lo = int(rng.integers(0, n - 40))
            s[lo:lo + 20] |= 0x20  # lower case
            run = int(rng.integers(0, n - (S + 12)))
            s[run:run + S + 12] = lm.N  # longer than a step: some piece holds nothing else
            seqs.append(s)
    for n, s in zip(boundary_lengths(pl), seqs):
        assert len(s) == n
    return np.concatenate(seqs), offsets_of([len(s) for s in seqs])


@functools.lru_cache(maxsize=None)
def piece_oracle(pl, kl):
    return sketch(*piece_input(pl), kl)


def assert_runs(nt, pl, offs):
    """the piece length takes cut_tiles_kernel where the test wants it"""
    n_chunks = pl // 16
    n_runs = (n_chunks + CUT_RUN - 1) // CUT_RUN  # ntc_long.hip:132
    if pl == 256:
        assert n_runs == 1 and n_chunks == CUT_RUN  # exactly one full run
    elif pl == 272:
        assert n_runs == 2 and n_chunks % CUT_RUN == 1  # a last run of one chunk (ntc_long.hip:42)
    else:
        assert n_runs > 1
    pieces, with_piece = planned(nt, np.diff(offs), K, pl)
    assert with_piece > 1 and pieces > with_piece  # ntc_long.hip:50-72: a table of several entries, sequences of several pieces
    lens = np.diff(offs).astype(np.int64)
    S = pl - (K - 1)
    for n, (m, rem) in zip(boundary_lengths(pl), ((0, pl - 1), (1, K - 1), (1, pl - 1), (2, K - 1), (2, K - 1), (2, K), (3, K - 1), (3, K))):
        assert n in lens and nt.long_plan(K, pl, n) == (m, m * S) and n - m * S == rem, (pl, n)


@pytest.mark.parametrize("pl,lead", [(256, 3), (272, 0), (272, 1), (272, 2), (272, 3), (1008, 3), (4096, 3), (65520, 3)])
def test_piece_lengths_of_several_runs(nt, pl, lead):
    buf, offs = piece_input(pl)
    assert_runs(nt, pl, offs)
    *got, stats = count_long(nt, *on_device(buf, offs, lead), (K,), pl, flags=nt.FLAG_REQUIRE_TILED)
    assert stats == planned(nt, np.diff(offs), K, pl)
    same(got, piece_oracle(pl, (K,)), (pl, lead))


@pytest.mark.parametrize("pl", [272, 4096])
def test_piece_lengths_under_a_k_list(nt, pl):
    """17,32: one cut with the overlap of k = 32; k = 17 counts the same tiles as reads of pl - 15 bases, and the remainders of 31 bytes count for it alone"""
    kl = (17, K)
    buf, offs = piece_input(pl)
    assert_runs(nt, pl, offs)
    *got, stats = count_long(nt, *on_device(buf, offs), kl, pl, flags=nt.FLAG_REQUIRE_TILED)
    assert stats == planned(nt, np.diff(offs), K, pl)
    same(got, piece_oracle(pl, kl), (pl, kl))


# ---- the depth of the table search ----
PL = 48
STEP = PL - K + 1
DEPTHS = {64: 1, 65: 2, 4096: 2, 4097: 3, 5000: 3}  # sequences with a full piece -> steps of the 64-way search (ntc_long.hip:50-55)


@functools.lru_cache(maxsize=None)
def table_input(n_full):
    """n_full sequences of 1 .. 3 pieces of 48, every other one followed by a sequence without a piece; now and then an N"""
    rng = np.random.default_rng(n_full)
    lens = []
    for i in range(n_full):
        lens.append(PL + (int(rng.integers(1, 4)) - 1) * STEP + int(rng.integers(0, STEP)))
        if i % 2:
            lens.append(int(rng.integers(0, PL)))
    offs = offsets_of(lens)
    buf = ACGT[rng.integers(0, 4, size=int(offs[-1]))]
    buf[rng.integers(0, buf.size, size=buf.size // 3000)] = lm.N
    return buf, offs


@functools.lru_cache(maxsize=None)
def table_oracle(n_full, kl):
    return sketch(*table_input(n_full), kl)


def assert_depth(nt, n_full, offs):
    pieces, with_piece = planned(nt, np.diff(offs), K, PL)
    assert with_piece == n_full and len(offs) - 1 == n_full + n_full // 2  # the table cut_tiles_kernel gets has exactly n_full entries
    assert n_full <= pieces <= 3 * n_full
    assert max(lm.cut_search_steps(n_full, t) for t in {0, 1, 63, 64, n_full // 2, n_full - 2, n_full - 1} if t < n_full) == DEPTHS[n_full]
    return pieces, with_piece


@pytest.mark.parametrize("n_full", sorted(DEPTHS))
def test_table_search_depth(nt, n_full):
    buf, offs = table_input(n_full)
    want = assert_depth(nt, n_full, offs)
    *got, stats = count_long(nt, *on_device(buf, offs), (K,), PL, flags=nt.FLAG_REQUIRE_TILED)
    assert stats == want
    same(got, table_oracle(n_full, (K,)), n_full)


def test_table_search_depth_under_a_k_list(nt):
    buf, offs = table_input(4097)
    want = assert_depth(nt, 4097, offs)
    *got, stats = count_long(nt, *on_device(buf, offs), (17, K), PL, flags=nt.FLAG_REQUIRE_TILED)
    assert stats == want
    same(got, table_oracle(4097, (17, K)), "17,32")


def test_rounds_begin_in_the_middle_of_a_three_step_table(nt, monkeypatch):
    """NTC_LONG_ROUND_BYTES = 1: a round is one tile of pieces, so the later rounds pass a first piece that lies deep in the table"""
    monkeypatch.setenv("NTC_LONG_ROUND_BYTES", "1")
    buf, offs = table_input(4097)
    want = assert_depth(nt, 4097, offs)
    assert want[0] > 3 * 2048  # four rounds or more
    *got, stats = count_long(nt, *on_device(buf, offs), (K,), PL, flags=nt.FLAG_REQUIRE_TILED)
    assert stats == want
    same(got, table_oracle(4097, (K,)), "rounds")


# ---- the gather's stride loop ----
N_SLOTS = 40_000
GATHER_WAVES = 8192 * 4  # ntc_long.hip:143: at most 8192 workgroups of four waves, a wave per slot and turn


@functools.lru_cache(maxsize=None)
def slot_input(lo, hi):
    rng = np.random.default_rng(lo)
    offs = offsets_of(rng.integers(lo, hi + 1, size=N_SLOTS))
    buf = ACGT[rng.integers(0, 4, size=int(offs[-1]))]
    buf[rng.integers(0, buf.size, size=buf.size // 2000)] = lm.N
    return buf, offs


def assert_slots(offs, k):
    lens = np.diff(offs).astype(np.int64)
    # every sequence is one row slot: it holds a window (none is dropped), and none is longer than a slot's capacity of 256 bytes (ntc_engine.hpp:40: no chunks)
    assert len(lens) == N_SLOTS > GATHER_WAVES and lens.min() >= k and lens.max() <= 256


def test_gather_of_more_slots_than_waves(nt, monkeypatch):
    """40 000 sequences shorter than a piece on an engine that cuts: all of them row slots of ONE gather launch, whose waves take a second slot"""
    monkeypatch.delenv("NTC_LONG_ROUND_BYTES", raising=False)  # (one round)
    buf, offs = slot_input(32, 47)
    assert_slots(offs, K)
    assert planned(nt, np.diff(offs), K, PL) == (0, 0)
    *got, stats = count_long(nt, *on_device(buf, offs), (K,), PL)
    assert stats == (0, 0)
    same(got, sketch(buf, offs, (K,)), "slots")


def test_gather_whole_of_more_slots_than_waves(nt, monkeypatch):
    """the same count on an engine that does not qualify for the cut (k = 64): every sequence gathered whole"""
    monkeypatch.delenv("NTC_LONG_ROUND_BYTES", raising=False)
    buf, offs = slot_input(64, 100)
    assert_slots(offs, 64)
    *got, stats = count_long(nt, *on_device(buf, offs), (64,), 0)
    assert stats == (0, 0)
    same(got, sketch(buf, offs, (64,)), "whole")
