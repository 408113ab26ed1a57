"""The K1f case families of tests/k1f_cases.py on the CPU: the GENERATED K1h runs on the wave emulator, k1h_model.k1f_model plays K1f, and F1 and every
counter must equal the oracle's.  What this file adds to that is COVERAGE AS A CONDITION: tests/test_k1f_cases_gpu.py sends the same families through
the HIP kernels, and the assertions here say which branches of k1f_suspect_role / k1f_f1_role those inputs reach — the marks K1h hands over (16 / 32 /
64: the dirty pieces of the window, 4: a tie, 2: the pattern fails below the 8-bit prefix), all 16 offsets of the window in its first piece, suspects
that count and suspects that must not, every (chunk, offset) of a dirty byte — so that the GPU file cannot quietly test less than it claims.
"""
import collections
import ctypes as C
import itertools

import numpy as np
import pytest

import k1f_cases as kc
import k1h_model as km
import orc
from support import sampled

R_BITS = 14
SUS_CAP = 4096  # no family may overflow the suspect list at the engine's sizing (2048 + per wave at least)
BASES = frozenset(b"ACGTUacgtu")


def emulate(case, slow=False):
    """K1h on the emulator + the K1f model against the oracle -> the emulator's result"""
    reads = case.reads
    res = km.run_k1h(kc.tile(reads, case.read_len), len(reads), case.read_len, case.k, r_bits=R_BITS, s_bits=case.s_bits, n_waves=2, sus_cap=SUS_CAP,
                     gap=case.gap, tails=case.tails)
    assert not res["sus_overflow"]
    fk, f1_sub = km.k1f_model(reads, case.read_len, case.k, R_BITS, case.s_bits, res["dirty"], res["tie"], res["sus"], slow, gap=case.gap)
    got = np.bincount(np.concatenate([res["keys"], np.array(fk, dtype=np.uint32)]).astype(np.int64), minlength=2 << R_BITS).astype(np.uint32) + res["sketch"]
    oc, of1 = orc.sketch_reads(reads, [case.k], case.gap, R_BITS, case.s_bits)
    assert res["f1"] - f1_sub == int(of1[0])
    assert np.array_equal(got, oc[0].reshape(-1).astype(np.uint32))
    return res


def dirty_bit(res, r, c):
    return (int(res["dirty"][r // 2048, c, (r % 2048) % 64]) >> ((r % 2048) // 64)) & 1


def assert_every_dirty_position(case, res):
    """every (chunk, piece offset) of the read length holds a non-base byte in some read, and K1h marked that piece dirty"""
    seen = set()
    for r, seq in enumerate(case.reads):
        for p, b in enumerate(seq):
            if b not in BASES and dirty_bit(res, r, p // 16):
                seen.add(p)
    assert seen == set(range(case.read_len))


def suspects_of(case, res, planted):
    """the emulator's suspect entries that are planted windows -> [(read, window start, pool, mark, reached dirty bits, window is clean, oracle counts it)]"""
    at = {(r, w): name for r, w, name in planted}
    Cn = (case.read_len + 15) // 16
    out = []
    for x, t, rw, mark in res["sus"]:
        r, w = int(t) * 2048 + (int(rw) & 2047), int(rw) >> 11
        if (r, w) not in at:
            continue
        reach = sum(1 << j for j in range(3) if w // 16 + j < Cn and 16 * j < w % 16 + case.k)
        ok, fv, rv = km.window_hashes(case.reads[r][w:w + case.k], case.k, case.gap)
        counts = bool(ok) and bool(sampled(min(fv, rv), case.s_bits))
        out.append((r, w, at[(r, w)], int(mark), (int(mark) >> 4) & reach, bool(ok), counts))
    return out


def required_combos(k):
    """the non-empty sets of dirty pieces a window of k bases can show: piece c0 + j is reached iff 16 j < off + k for some offset 0 .. 15"""
    bits = [1 << j for j in range(3) if 16 * j < 15 + k]
    return {sum(c) for n in range(1, len(bits) + 1) for c in itertools.combinations(bits, n)}


def check_suspect_coverage(case, res, planted, all_offsets=True):
    sus = suspects_of(case, res, planted)
    print(f"suspects k={case.k} sBits={case.s_bits} gap={case.gap} L={case.read_len}: {len(case.reads)} reads, {len(res['sus'])} suspects, {len(sus)} planted; marks",
          dict(sorted(collections.Counter(int(m) for m in res["sus"][:, 3]).items())))
    for tie in (0, 4):
        mine = [s for s in sus if s[3] & 4 == tie]
        assert {s[4] for s in mine} >= required_combos(case.k), (tie, sorted({s[4] for s in mine}))
        assert any(s[5] and s[6] for s in mine), "no suspect with a clean window that counts"
        assert any(not s[5] for s in mine), "no suspect whose window holds a non-base byte"
    assert all(s[3] & 4 for s in sus if s[2] == "tie") and not any(s[3] & 4 for s in sus if s[2] == "plain")
    if all_offsets:
        assert {s[1] % 16 for s in sus} == set(range(16))
    if case.s_bits >= 8:
        below = [s for s in sus if s[3] & 2]
        assert any(s[4] for s in below) and any(not s[4] for s in below), "mark 2 with and without dirty bits"
    return sus


@pytest.mark.parametrize("k,L", [(k, L) for k in kc.F1_K for L in kc.f1_lengths(k)])
def test_f1_single(k, L):
    case = kc.f1_single(k, L)
    assert_every_dirty_position(case, emulate(case))


@pytest.mark.parametrize("k", kc.F1_K)
def test_f1_pairs(k):
    case = kc.f1_pairs(k)
    res = emulate(case)
    assert_every_dirty_position(case, res)  # (the first N alone covers piece 1; the second ones reach up to the read's last byte)


@pytest.mark.parametrize("k", kc.F1_K)
def test_f1_runs(k):
    case = kc.f1_runs(k)
    assert_every_dirty_position(case, emulate(case))


def test_bytes256():
    case = kc.bytes256()
    res = emulate(case)
    fh, rh, bad = C.c_uint64(), C.c_uint64(), C.c_uint()
    for i, v in enumerate(kc.BYTES256):
        for j, p in enumerate((32, 47)):
            r = 2 * i + j
            assert case.reads[r][p] == v
            is_base = bool(orc.lib().orc_window_hash(case.reads[r][p - 5:p + 27], 32, C.byref(fh), C.byref(rh), C.byref(bad)))
            assert is_base == (v in BASES), v  # (the oracle is pinned to the reference for exactly this)
            assert dirty_bit(res, r, p // 16) == (v not in b"ACGTacgt"), v  # U and u are dirty to K1h, and bases all the same
    for v in (ord("A") ^ 1, ord("C") ^ 1, ord("G") ^ 1, ord("T") ^ 2, ord("A") ^ 4, ord("G") ^ 8, ord("T") ^ 16, ord("a") ^ 64, ord("A") ^ 128):
        assert v in kc.BYTES256 and v not in BASES  # values one bit away from a letter are in the family, and no bases


@pytest.mark.parametrize("k,s_bits", [(12, 7), (17, 7), (32, 7), (32, 8), (32, 11)])
def test_suspects(k, s_bits):
    case = kc.suspects(k, s_bits)
    check_suspect_coverage(case, emulate(case), kc.suspects_planted(k, s_bits))


@pytest.mark.parametrize("k,gap", [(12, 2), (32, 8)])
def test_suspects_spaced_seed(k, gap):
    """the pools found with window_hashes(..., gap): the same matrix under the two spaced seeds the tiled kernels are built for"""
    case = kc.suspects(k, 7, gap)
    check_suspect_coverage(case, emulate(case), kc.suspects_planted(k, 7, gap))


@pytest.mark.parametrize("k,L", [(k, L) for k in kc.F1_K for L in kc.suspects_end_lengths(k)])
def test_suspects_window_ends_on_the_last_base(k, L):
    case = kc.suspects_end(k, L)
    res = emulate(case)
    sus = suspects_of(case, res, kc.suspects_end_planted(k, L))
    print(f"suspects_end k={k} L={L}: {len(case.reads)} reads, {len(sus)} planted suspects; marks", dict(sorted(collections.Counter(s[3] for s in sus).items())))
    ends = [s for s in sus if s[1] + k == L]
    for tie in (0, 4):
        assert any(not s[5] for s in ends if s[3] & 4 == tie)
        # (a window that starts on a piece boundary and ends on the read's last base leaves no byte of its pieces uncovered: no clean suspect exists)
        assert (L - k) % 16 == 0 or any(s[5] and s[6] for s in ends if s[3] & 4 == tie)
    if L == 64:  # the window's last piece is the read's last: fewer than three pieces behind c0
        assert any(s[1] // 16 + 2 >= 4 for s in ends)


@pytest.mark.parametrize("C,k", kc.RAGGED)
def test_ragged(C, k):
    case = kc.ragged(C, k)
    lens = [len(r) for r in case.reads]
    assert set(lens) == set(range(16 * C - 15, 16 * C + 1)) and lens == sorted(lens, reverse=True)
    res = emulate(case)
    # in every read length a read whose last real base is a non-base byte, marked dirty by K1h (and none behind it: the padding is 'A')
    assert {len(r) for i, r in enumerate(case.reads) if r[-1] not in BASES and dirty_bit(res, i, C - 1)} == set(lens)
    # ... and suspects whose window ends on the read's last base, clean ones and spoilt ones
    ends = collections.defaultdict(set)
    for x, t, rw, mark in res["sus"]:
        r, w = int(t) * 2048 + (int(rw) & 2047), int(rw) >> 11
        if w + k == len(case.reads[r]):
            ends[len(case.reads[r])].add(bool(km.window_hashes(case.reads[r][w:w + k], k, 0)[0]))
    assert all(ends[ln] == {True, False} for ln in set(lens)), dict(ends)


@pytest.mark.parametrize("v", (1, 7))  # (the GPU file runs all five)
def test_slot_bytes(v):
    """a reference-table slot byte: the model's slow path (every window of a dirty-affected block from the bytes)"""
    case = kc.slot_bytes(v)
    assert sum(r.count(bytes([v])) for r in case.reads) == 2
    emulate(case, slow=True)


def test_dense_suspects_fill_a_hit_log_region():
    """kc.dense: more than 4 x 256 counting suspects whose windows all end in ONE block of tile 0.  A block is walked by one K1h wave, so they share one
    suspect region; K1f's suspect role gives a region to one workgroup, whose four waves append to one hit-log region each — 256 entries with
    log_entries = 2^18 (ntc_plan.hip: plan_log) — and what does not fit goes to the sketch with device atomics (count_hit: pos >= klog_cap).
    The region must not overflow the engine's own suspect list (2752 per wave for this geometry), or the launch would take the slow path instead"""
    case = kc.dense()
    res = emulate(case)
    k, phi = case.k, (case.k - 1) % 16
    blocks = collections.Counter()
    for x, t, rw, mark in res["sus"]:
        r, w = int(t) * 2048 + (int(rw) & 2047), int(rw) >> 11
        ok, fv, rv = km.window_hashes(case.reads[r][w:w + k], k, 0)
        if ok and sampled(min(fv, rv), 7):
            blocks[(int(t), (w + k - 1 - phi) // 16 + 1)] += 1
    print("dense: counting suspects per (tile, block)", dict(blocks), "suspects in all", len(res["sus"]))
    assert max(blocks.values()) > 4 * 256 + 64
    assert len(res["sus"]) < 2752
