"""The case table of tests/k1h_variant_cases.py, checked without a GPU: its GPU cases and its emulator cases each run every K1h body the generator is
asked for (so a variant added to gen_k1h.VARIANTS without a case fails here), and no case is vacuous — by the models alone, both samples of the plane
are hit, the three strands give three different sketches, a case with non-base bytes holds a window over one, and the planted windows sample."""
import numpy as np
import pytest

import k1h_variant_cases as vc
import strand_model as sm
from support import gap_mask, nt_comp, oracle_counts

gen_k1h = vc.gen_k1h


def test_the_generator_is_asked_for_138_bodies():
    assert len(gen_k1h.VARIANTS) == 23 and len(set(gen_k1h.VARIANTS)) == 23 and len(set(gen_k1h.STRAND_VARIANTS)) == 46
    bodies = vc.all_bodies()
    assert len(bodies) == 138 and sum(1 for b in bodies if b[2] == sm.CANONICAL) == 46


@pytest.mark.parametrize("name", ["GPU_BODY_CASES", "EMU_CASES"])
def test_the_cases_run_every_body_and_no_other(name):
    cases = getattr(vc, name)
    assert {vc.body_of(c) for c in cases} == vc.all_bodies()
    for body in sorted(vc.all_bodies()):  # (the proof has teeth: without the cases of one body the sets differ)
        assert {vc.body_of(c) for c in cases if vc.body_of(c) != body} != vc.all_bodies()
    assert len({vc.case_id(c) for c in cases}) == len(cases)
    assert all(vc.tiled_supports(c) for c in cases)


def test_the_issue_shapes():
    """per (k, gap, strand): class 7 with a partial last tile at k + 29 bases and, on the GPU, reads of exactly k bases; class 8 at sBits 8 and 11"""
    for k, gap, st in gen_k1h.STRAND_VARIANTS:
        mine = {(c.s_bits, c.n, c.L, c.p_bad) for c in vc.GPU_BODY_CASES if (c.k, c.gap, c.strand) == (k, gap, st)}
        assert mine == {(7, 2049, k + 29, 0.01), (7, 2100, k, 0.0), (8, 2500, k + 29 if gap else k + 1, 0.01), (11, 2049, 97, 0.0)}
        mine = {(c.s_bits, c.r_bits, c.n, c.L, c.p_bad) for c in vc.EMU_CASES if (c.k, c.gap, c.strand) == (k, gap, st)}
        assert mine == {(7, 14, 2049, k + 29, 0.01), (8, 12, 2500, k + 29, 0.01)}
    assert {(c.s_bits, c.L) for c in vc.GPU_BODY_CASES if (c.k, c.gap, c.strand) == (32, 8, sm.CANONICAL)} == {(7, 61), (8, 61), (11, 97)}
    assert {(c.s_bits, c.r_bits) for c in vc.RANGE_CASES} == {(13, 14), (16, 14), (20, 18)} and {c.k for c in vc.RANGE_CASES} == {32, 23}
    assert all(c.r_bits + 1 + c.s_bits - 7 == 32 for c in vc.PLANT_CASES + [c for c in vc.RANGE_CASES if c.s_bits == 20])
    assert all(c.r_bits + 1 + c.s_bits - 7 == 33 and not vc.tiled_supports(c) for c in vc.REFUSE_CASES)
    for group in (vc.RAGGED_CASES, vc.SHORT_READ_CASES, vc.RANGE_CASES, vc.PLANT_CASES, vc.REFUSE_CASES):
        assert {c.strand for c in group} >= {sm.FORWARD, sm.REVERSE}


def check_not_vacuous(c):
    sk = vc.model_sketches(c)
    tc, f1 = sk[c.strand]
    per_sample = tc[0].astype(np.int64).sum(axis=1)
    assert per_sample.min() >= vc.MIN_PER_SAMPLE, (vc.case_id(c), per_sample)
    assert int(f1[0]) > 0
    if c.strand != sm.CANONICAL:
        for a, b in ((sm.CANONICAL, sm.FORWARD), (sm.CANONICAL, sm.REVERSE), (sm.FORWARD, sm.REVERSE)):
            assert not np.array_equal(sk[a][0], sk[b][0]), (vc.case_id(c), a, b)
    else:  # the array model's canonical sketch is the C oracle's
        oc, of1 = vc.want(c)
        assert np.array_equal(oc, tc) and np.array_equal(of1, f1), vc.case_id(c)
    arr = vc.reads_of(c)
    if c.p_bad > 0:
        nwin = np.maximum((arr != ord("#")).sum(axis=1) - c.k + 1, 0).sum()  # (behind a ragged read's end: '#')
        assert int(f1[0]) < nwin, vc.case_id(c)
    if c.kind == "ragged":
        lens = (arr != ord("#")).sum(axis=1)
        assert lens.min() == c.L - 15 and lens.max() == c.L and [len(r) for r in vc.ragged_list(arr)] == lens.tolist()
    assert np.array_equal(sk[sm.FORWARD][1], f1) and np.array_equal(sk[sm.REVERSE][1], f1)
    return sk


@pytest.mark.parametrize("c", list(dict.fromkeys(vc.GPU_BODY_CASES + vc.RAGGED_CASES + vc.EMU_CASES)), ids=vc.case_id)  # (the class-7 case serves both)
def test_a_body_case_is_not_vacuous(c):
    check_not_vacuous(c)


@pytest.mark.parametrize("c", vc.SHORT_READ_CASES + vc.RANGE_CASES, ids=vc.case_id)
def test_a_large_case_is_not_vacuous(c):
    check_not_vacuous(c)


@pytest.mark.parametrize("c", vc.PLANT_CASES + vc.REFUSE_CASES, ids=vc.case_id)
def test_planted_windows_sample_as_planned(c):
    """every planted window without an N inside counts in its sample under the case's strand, the ones with an N inside are no windows, and both
    samples hold at least 8 planted hits"""
    check_not_vacuous(c)
    arr, plants = vc.planted_reads(c)
    assert np.array_equal(arr, vc.reads_of(c))
    assert len({r for r, _, _, _ in plants}) == len(plants) == 2 * sum(n for _, n in vc.PLANTS)
    fs, rs, ok = sm.array_window_values(arr, gap_mask(c.k, c.gap))
    hits = {0: 0, 1: 0}
    for r, w, sample, what in plants:
        row = arr[r]
        n_at = np.flatnonzero((row == ord("N")) | (row == ord("n")))
        if what == "n_inside":
            assert not ok[r, w] and len(n_at) == 1 and w <= n_at[0] < w + c.k
            continue
        assert ok[r, w]
        got, _ = nt_comp(sm.pick(fs[r, w:w + 1], rs[r, w:w + 1], c.strand), c.r_bits, c.s_bits)
        assert got[0] == sample, (r, w, sample, what)
        hits[sample] += 1
        if what == "clean":
            assert len(n_at) == 0
        else:  # the N lies outside the window, in a 16-byte chunk the window touches
            assert len(n_at) == 1 and not w <= n_at[0] < w + c.k and w // 16 <= n_at[0] // 16 <= (w + c.k - 1) // 16, (r, w, what, n_at)
    assert min(hits.values()) >= vc.MIN_PER_SAMPLE


def test_long_sequences_are_not_vacuous():
    seqs = vc.long_seqs()
    for k in vc.LONG_KLIST:
        sk = sm.array_sketches(sm.pad_reads(seqs), "1" * k, [(s, vc.LONG_R_BITS, vc.LONG_S_BITS) for s in vc.ALL_STRANDS])
        tcs = [sk[s, vc.LONG_R_BITS, vc.LONG_S_BITS][0] for s in vc.ALL_STRANDS]
        assert all(t[0].astype(np.int64).sum(axis=1).min() >= vc.MIN_PER_SAMPLE for t in tcs)
        assert not any(np.array_equal(tcs[a], tcs[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
        oc, of1 = oracle_counts(list(seqs), [k], 0, vc.LONG_R_BITS, vc.LONG_S_BITS)
        assert np.array_equal(oc, tcs[0]) and np.array_equal(of1, sk[sm.CANONICAL, vc.LONG_R_BITS, vc.LONG_S_BITS][1])
    assert any(len(s) >= vc.LONG_PIECE for s in seqs) and any(len(s) < vc.LONG_PIECE for s in seqs) and any(b"N" in s for s in seqs)
