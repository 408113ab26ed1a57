"""Host tests of the forge (tests/hash_forge.py) and of the case tables built with it (tests/forged_cases.py): every forged k-mer's values, asked of the
oracle, have exactly the prescribed bits; every case's planned effect is what the models compute; the cases tell the errors they are meant for apart.
No case is skipped: a prescription that cannot be forged is a wrong table entry."""
import numpy as np
import pytest

import forged_cases as fc
import hash_forge as hf
import hll_model as hm
import orc
import strand_model as sm
from support import key_of


def oracle_values(kmer, mask=None):
    """(fh, rh) of the one window of a k-mer by the oracle's primitives (tests/strand_model.py: window_values)"""
    fs, rs, pos = sm.window_values(kmer, "1" * len(kmer) if mask is None else mask)
    assert fs.size == 1 and pos[0] == 0
    return int(fs[0]), int(rs[0])


def has(value, want):
    return value & want[1] == want[0]


# ---- 1. the forge against the oracle ----
def test_the_restated_primitives_are_the_oracle_s():
    L = orc.lib()
    for b, s in hf.SEED.items():
        assert L.orc_seed(ord(b)) == s and L.orc_seed_comp(ord(b)) == hf.SEED[hf.COMP[b]]
        for n in (0, 1, 30, 31, 32, 33, 34, 95, 159, 1022, 1023):
            assert L.orc_srol(s, n) == hf.srol(s, n)


PRESCRIPTIONS = ([(96, hf.lz(r, n, 5), hf.NONE, None) for n in (4, 16, 24) for r in (0, 1, 30, 31, 32, 33, 40, 48, 63 - n, 64 - n) if r <= 64 - n]
                 + [(96, hf.NONE, hf.lz_only_lowest(n, 3), None) for n in (4, 16, 24)]
                 + [(70, (0x0123456789ABCDEF, hf.M64), hf.NONE, None), (70, hf.NONE, (0xFEDCBA9876543210, hf.M64), None)]
                 + [(96, hf.sampled(t, s, 77, 14, below=1), hf.NONE, fc.SPACED96) for t in (0, 1) for s in (2, 7, 16, 24)]
                 + [(96,) + hf.smaller(hf.sampled(0, 24, 16383, 14)) + (None,), (96,) + hf.smaller(hf.lz(0, 16, 9))[::-1] + (fc.SPACED96,)]
                 + [(160,) + hf.tie32(0x00012345, "0", "1", 16, 7, 8) + (None,), (160,) + hf.tie32(0xFFFFFFFF, "1", "0", 24, 1, 2) + (None,)]
                 + [(160, (0x0000000100000000 | 5, hf.M64), hf.both(hf.top("0" * 31 + "1"), hf.low(24, 6)), None)]
                 + [(32, hf.sampled(0, 24), hf.NONE, None), (32, hf.NONE, hf.sampled(1, 24, below=0), None), (32, hf.top("0" * 15 + "1"), hf.top("0" * 16), None),
                    (20, hf.sampled(1, 12, 5, 3, below=1), hf.top("1"), None)])


@pytest.mark.parametrize("i", range(len(PRESCRIPTIONS)))
def test_forged_kmers_have_the_prescribed_bits(i):
    k, wf, wr, mask = PRESCRIPTIONS[i]
    kmer = hf.forge(k, wf, wr, mask=mask, seed=100 + i)
    assert len(kmer) == k and set(kmer) <= set(b"ACGT") and kmer == hf.forge(k, wf, wr, mask=mask, seed=100 + i)
    f, r = oracle_values(kmer, mask)
    assert has(f, wf) and has(r, wr), (hex(f), hex(r))
    assert (f, r) == hf.values(kmer, mask)
    if mask is None:  # the canonical value as the oracle's iterator gives it
        h, _ = orc.hash_read(kmer, k)
        assert h.tolist() == [min(f, r)]


def test_an_unsolvable_prescription_raises():
    with pytest.raises(hf.ForgeError):
        hf.forge(32, hf.top("0" * 24), hf.top("0" * 24), seed=1)  # 48 bits against rank 32
    with pytest.raises(hf.ForgeError):
        hf.forge(16, (0, hf.M64), seed=1)


def oracle_rank(k, bits_f, bits_r, seed):
    """the rank of (fh, rh) & (bits_f, bits_r) over random base pairs, from the oracle's srol and seeds alone"""
    import random
    L, rng = orc.lib(), random.Random(seed)
    vec = []
    for i in range(k):
        a, b = rng.sample(b"ACGT", 2)
        f = L.orc_srol(L.orc_seed(a), k - 1 - i) ^ L.orc_srol(L.orc_seed(b), k - 1 - i)
        r = L.orc_srol(L.orc_seed_comp(a), i) ^ L.orc_srol(L.orc_seed_comp(b), i)
        vec.append((f & bits_f) | ((r & bits_r) << 64))
    return hf.solve(vec, 0)[1]


def test_the_rank_limits():
    """what the case tables rely on, measured with the oracle's primitives: one strand reaches 64 from k = 70 on, both strands 124 of 128; k = 32 gives 32
    (25 bits of one strand and 16 of each are reachable, 24 of each are not)"""
    top = lambda n: ((1 << n) - 1) << (64 - n)  # noqa: E731
    for seed in range(3):
        assert [oracle_rank(k, hf.M64, 0, seed) for k in (20, 32, 70, 96)] == [20, 32, 64, 64]
        assert [oracle_rank(k, 0, hf.M64, seed) for k in (70, 96)] == [64, 64]
        assert [oracle_rank(k, hf.M64, hf.M64, seed) for k in (96, 128, 136, 160, 300, 600)] == [96, 124, 124, 124, 124, 124]
        # (one random choice of pairs may fall one short of the full rank: that is what the forge's retries are for)
        assert oracle_rank(32, top(25), 0, seed) >= 24 and oracle_rank(32, top(16), top(16), seed) >= 31 and oracle_rank(32, top(24), top(24), seed) <= 32 < 48
        assert oracle_rank(k=160, bits_f=hf.M64, bits_r=hf.M64, seed=seed) == hf.rank(160, seed=seed)


def test_the_parity_invariant():
    """srol keeps the parity of either part, a base and its complement differ in the low parity and agree in the high one: parity_low(fh) ^ parity_low(rh)
    is k mod 2 and parity_high(fh) ^ parity_high(rh) is 0 for every window (the oracle's values over random reads)"""
    import random
    rng = random.Random(5)
    par = lambda x: bin(x).count("1") & 1  # noqa: E731
    for k in (1, 20, 33, 96, 161):
        fs, rs, _ = sm.window_values(bytes(rng.choice(b"ACGT") for _ in range(k + 20)), "1" * k)
        for f, r in zip(fs.tolist(), rs.tolist()):
            assert par(f & hf.M33) ^ par(r & hf.M33) == k & 1 and par(f >> 33) ^ par(r >> 33) == 0


# ---- 2. nthll: the planned effect is the model's ----
HLL = {c.name: c for c in fc.hll_cases()}


def test_the_hll_case_names_are_unique():
    assert len(HLL) == len(fc.hll_cases()) == 6 + 3 + 12 + 5 + 2 + 1


@pytest.mark.parametrize("name", list(HLL))
def test_hll_cases_do_what_they_plan(name):
    c = HLL[name]
    regs, f1 = fc.hll_model(c)
    for (plane, bucket), value in c.plan.items():
        assert regs[plane, bucket] == value, (name, plane, bucket)
    assert len(c.plan) >= 3 and max(c.plan.values()) > 0
    if c.complete:
        assert int(np.count_nonzero(regs)) == sum(1 for v in c.plan.values() if v) and f1.tolist() == list(c.f1)
    if len(c.masks) == 1 and c.strand == sm.CANONICAL and not c.seeded:  # the oracle's own nthll over the same reads
        want, _ = orc.hll_reads(fc.all_reads(c), len(c.masks[0]), c.n_bits)
        assert np.array_equal(want, regs[0])


@pytest.mark.parametrize("n_bits", [4, 16, 24])
def test_the_ladder_reaches_every_branch(n_bits):
    """by the oracle's values: run0 0, 1, 30, 31 (the high word decides), 32, 33 and 63 - n_bits (hi == 0: 32 or more leading zeros), rest == 0, and the
    picked value is the forward one for some and the reverse one for others"""
    seen, holders = set(), set()
    for what, kmer, bucket, run0 in fc.ladder(n_bits):
        f, r = oracle_values(kmer)
        h = min(f, r)
        holders.add(h == f)
        assert h & ((1 << n_bits) - 1) == bucket
        rest = h >> n_bits << n_bits
        assert (run0 is None and rest == 0) or 64 - rest.bit_length() == run0, what
        seen.add(run0)
        if what == "lowest":
            assert rest == 1 << n_bits
    assert seen == {0, 1, 30, 31, 32, 33, min(40, 62 - n_bits), 63 - n_bits, None} and holders == {True, False}


def test_ladder_order_cases_differ_in_their_first_submit():
    for n_bits in (4, 16, 24):
        up, down = fc.hll_model_after(f"ladder_b{n_bits}_up", 1), fc.hll_model_after(f"ladder_b{n_bits}_down", 1)
        b = fc.bucket_of(8, n_bits)
        assert (up[0][0, b], down[0][0, b]) == (31, 32)
        assert np.array_equal(fc.hll_model(HLL[f"ladder_b{n_bits}_up"])[0], fc.hll_model(HLL[f"ladder_b{n_bits}_down"])[0])


def test_strand_cases_tell_the_strands_apart():
    """each strand's registers differ from the others'; a canonical choice made on the top 32 bits alone (ties go to the forward value) gives other registers"""
    regs = {s: fc.hll_model(HLL[f"strands_{fc.NAMES[s]}"])[0] for s in (sm.CANONICAL, sm.FORWARD, sm.REVERSE)}
    assert not np.array_equal(regs[sm.CANONICAL], regs[sm.FORWARD]) and not np.array_equal(regs[sm.CANONICAL], regs[sm.REVERSE])
    fs, rs = sm.values_of(list(HLL["strands_canonical"].submits[0]), ["1" * fc.STRAND_K])[0]
    ties = (fs >> np.uint64(32)) == (rs >> np.uint64(32))
    assert ties.sum() == 2 and (fs[ties] < rs[ties]).tolist() == [True, False]
    wrong = np.where((rs >> np.uint64(32)) < (fs >> np.uint64(32)), rs, fs)
    assert not np.array_equal(hm.registers(wrong, 16), regs[sm.CANONICAL][0])
    for (f, r), row in zip(zip(fs.tolist(), rs.tolist()), fc.strand_kmers()):
        assert (f & 0xFFFF, r & 0xFFFF) == (row[1][0], row[2][0]) and (f < r) == (row[3] == sm.FORWARD)


@pytest.mark.parametrize("name", [c.name for c in fc.threshold_cases()] + ["planes_96_160"])
def test_threshold_cases_second_submit_changes_the_registers(name):
    c = HLL[name]
    before, after = fc.hll_model_after(name, 1)[0], fc.hll_model(c)[0]
    plane = len(c.masks) - 1
    assert int(before[plane].min()) == int(before[plane].max()) == (1 if name.startswith("planes") else int(name.split("_")[1][1:]))
    changed = np.flatnonzero(after[plane] != before[plane]).tolist()
    if name.startswith("planes"):
        assert changed == [5] and int(before[0].min()) == 30 and np.array_equal(before[0], after[0])  # plane 0's threshold would hide the window
    else:
        m = int(before[plane].min())
        assert changed == ([1, 2, 3, 4] if c.strand == sm.CANONICAL else [1, 2]) and after[0, 0] == m
    if c.strand == sm.CANONICAL:  # the qualifying value is one strand's while the other starts with a 1
        fs, rs = sm.values_of(list(c.submits[1][3:]), list(c.masks))[0]
        assert (fs >> np.uint64(63)).tolist() == [1, 0] and (rs >> np.uint64(63)).tolist() == [0, 1]


def test_one_submit_case_crosses_the_sub_batch():
    c = HLL["one_submit"]
    reads = c.submits[0]
    assert len(reads) == fc.SUB_BATCH + 64 and all(len(r) == 96 for r in reads)
    first = hm.model(list(reads[:fc.SUB_BATCH]), list(c.masks), c.strand, 4)[0]
    assert first.min() == first.max() == 7 and all(r == b"N" * 96 for r in reads[16:fc.SUB_BATCH])
    assert np.flatnonzero(fc.hll_model(c)[0][0] != first[0]).tolist() == [1, 2]


def test_other_ways_in_hold_the_ladder():
    for name in ("ladder_ragged", "ladder_offsets", "ladder_tiled", "ladder_spaced_forward", "ladder_spaced_reverse", "ladder_cli"):
        assert max(HLL[name].plan.values()) == 63 - HLL[name].n_bits
    assert len({len(r) for r in HLL["ladder_ragged"].submits[0]}) > 4
    assert {len(r) for r in HLL["ladder_offsets"].submits[0]} == {fc.LADDER_K + 37}
    f = fc.hll_model(HLL["ladder_spaced_forward"])[0]
    plain = hm.model(list(HLL["ladder_spaced_forward"].submits[0]), ["1" * 96], sm.FORWARD, 16)[0]
    rev = hm.model(list(HLL["ladder_spaced_forward"].submits[0]), [fc.SPACED96], sm.REVERSE, 16)[0]
    assert not np.array_equal(f, plain) and not np.array_equal(f, rev)  # the mask and the strand matter
    a, b = fc.merge_parts()
    ra, rb = (hm.model([r[1] for r in part], ["1" * 96], sm.CANONICAL, 16)[0][0] for part in (a, b))
    assert ra.max() > 32 and rb.max() > 32 and (ra[fc.bucket_of(5, 16)], rb[fc.bucket_of(5, 16)]) == (33, 40)


# ---- 3. ntcard: the planned effect is the model's ----
FAMILIES = {f.name: f for f in fc.sketch_families()}


def test_the_family_names_are_unique():
    assert len(FAMILIES) == len(fc.sketch_families()) == 18 + 18 + 9 + 11 + 2


@pytest.mark.parametrize("name", list(FAMILIES))
def test_families_do_what_they_plan(name):
    fam = FAMILIES[name]
    tc, f1 = fc.model_sketch(fc.family_reads(fam), fam.mask, fam.strand, fam.r_bits, fam.s_bits)
    keys, hits = set(), 0
    for e in fam.entries:
        f, r = oracle_values(e.kmer, fam.mask)
        v = int(sm.pick(np.array([f], dtype=np.uint64), np.array([r], dtype=np.uint64), fam.strand)[0])
        key = key_of(v, fam.r_bits, fam.s_bits)
        if e.sample is None:
            assert key is None, e.what
            continue
        assert key is not None and key >> fam.r_bits == e.sample, e.what
        if e.index_bits:
            assert key & ((1 << e.index_bits) - 1) == e.index, e.what
        assert key not in keys, e.what  # a counter of its own
        keys.add(key)
        hits += e.count
        assert tc[0, key >> fam.r_bits, key & ((1 << fam.r_bits) - 1)] == e.count, e.what
    assert int(tc.sum()) == hits and int(f1[0]) == sum(e.count for e in fam.entries)
    whats = {e.what for e in fam.entries}
    assert {"hit0", "hit1", "hit0_below0", "hit0_below1", "hit1_below0", "hit1_below1", "hit0_index0", "hit1_index_top", "miss0_first", "miss0_last",
            "miss1_first", "miss1_last"} <= whats
    if fam.strand == sm.CANONICAL and fam.k >= 96:
        assert {"superset_f", "superset_r", "both_match_f", "both_match_r", "tie_f", "tie_r"} <= whats


@pytest.mark.parametrize("name", [n for n, f in FAMILIES.items() if f.strand == sm.CANONICAL])
def test_canonical_families_need_the_right_strand(name):
    """the picked value is the forward one for some entries and the reverse one for others; the superset entries hold one strand 0^s 1.. and the other
    0^(s+1)..; in the both-match entries either strand is sampled, into different counters"""
    fam = FAMILIES[name]
    picked = set()
    for e in fam.entries:
        f, r = oracle_values(e.kmer, fam.mask)
        picked.add(f < r)
        if e.what.startswith("superset"):
            lo, hi = min(f, r), max(f, r)
            assert lo >> (63 - fam.s_bits) == 0 and hi >> (63 - fam.s_bits) == 1 and key_of(hi, fam.r_bits, fam.s_bits) is not None
        if e.what.startswith("both_match"):
            kf, kr = key_of(f, fam.r_bits, fam.s_bits), key_of(r, fam.r_bits, fam.s_bits)
            assert None not in (kf, kr) and kf != kr and (f < r) == e.what.endswith("_f")
        if e.what.startswith("tie"):  # equal top halves: only the low words order the strands
            kf, kr = key_of(f, fam.r_bits, fam.s_bits), key_of(r, fam.r_bits, fam.s_bits)
            assert f >> 32 == r >> 32 and None not in (kf, kr) and kf != kr and (f < r) == e.what.endswith("_f")
    assert picked == {True, False}


def test_near_misses_sit_one_bit_from_a_hit():
    for fam in FAMILIES.values():
        by = {e.what: e for e in fam.entries}
        for sample in (0, 1):
            n = fam.s_bits + 1 if sample == 0 else fam.s_bits
            vals = {}
            for what in (f"hit{sample}", f"miss{sample}_first", f"miss{sample}_last"):
                f, r = oracle_values(by[what].kmer, fam.mask)
                v = int(sm.pick(np.array([f], dtype=np.uint64), np.array([r], dtype=np.uint64), fam.strand)[0])
                if what == "miss1_first" and fam.k < 96 and fam.strand == sm.CANONICAL and v >> 62 == 2:
                    v = max(f, r)  # (tests/forged_cases.py: family — where the rank of a short k leaves no room to make 1^s 0.. the smaller strand)
                vals[what] = v >> (64 - n)
            assert vals[f"hit{sample}"] ^ vals[f"miss{sample}_first"] == 1 << (n - 1) and vals[f"hit{sample}"] ^ vals[f"miss{sample}_last"] == 1


def test_the_packing_boundary_families():
    """r_bits + 1 + (s_bits - 7) == 32 for the two tiled families at the limit of K1h's table word"""
    assert [(f.r_bits, f.s_bits) for f in (FAMILIES["k32_canonical_s24r14"], FAMILIES["k32_canonical_s18r20"])] == [(14, 24), (20, 18)]
    for r_bits, s_bits in ((14, 24), (20, 18)):
        assert r_bits + 1 + (s_bits - 7) == 32
