"""What tests/test_k1_cases_gpu.py covers, checked on the CPU so that the GPU file cannot quietly test less than it claims: every row of K1's table of
instantiations (enumerated through ntc_k1_variant_stats, which needs no device) in every regime it has, every path label a family can reach, and no
case whose reference is too thin to notice a wrong kernel.  The launch plan is the port in tests/k1_cases.py with the MI355X's 256 CUs; the GPU file
pins that port, launch for launch, to what the library reports."""
import numpy as np
import pytest

import k1_cases as kc

FAMILIES = ("plain", "tiled", "spaced", "hll", "sig", "dump")

# (row, regime) pairs of the requirement table that no case has to claim, each with its reason
REGIME_EXEMPT = {
    **{(dump_row, "MULTI"): "a dump buffer of two wave-batches per wave (600 k reads x 120 windows x 8 B) is out of proportion for a validation build"
       for dump_row in [(False, 1, 10, True, False, o, False) for o in (False, True)] + [(False, 0, 10, True, False, o, False) for o in (False, True)]},
}

LABELS = {
    "class": ("CLEAN", "DIRTY", "RAGGED_LEN", "RAGGED_PARTIAL", "RAGGED_MASK", "NOTHING"),
    "start": tuple("START_K%d%s" % (r, m) for r in range(4) for m in ("", "_MARK")),
    "tail": ("SHORT", "TAIL_STEPS", "FULL_BLOCK_TAIL"),
    "ragged": ("RAGGED_ONE_BLOCK", "RAGGED_BLOCKS", "RAGGED_END_IN_GROUP", "RAGGED_MARK_FILL", "RAGGED_MARK_MAIN", "RAGGED_ZERO_LEN"),
    "resolve": ("RESOLVE_FULL", "RESOLVE_REST", "NO_HIT"),
    "log": ("REGION_ROLL", "LOG_EXHAUSTED"),
    "sig": ("CHUNK_ROLL", "SIG_FUSED_CARRY"),
    "batches": ("WAVE_BATCHES_2",),
}
ALL_LABELS = frozenset(x for v in LABELS.values() for x in v)

# labels a family does not have to reach, each with its reason ("cannot": the code path does not exist there; "left out": it does, see the reason)
NOT_REACHED = {
    "plain": {"RAGGED_MASK": "cannot: only a spaced seed has toggle pairs", "CHUNK_ROLL": "cannot: signature rows only",
              "SIG_FUSED_CARRY": "cannot: signature rows only"},
    "tiled": {"RAGGED_MASK": "cannot: tiled staging is for plain k", "CHUNK_ROLL": "cannot: signature rows only", "SIG_FUSED_CARRY": "cannot: signature rows only",
              "RAGGED_ZERO_LEN": "cannot: a ragged tiled batch holds reads of one piece count", "NOTHING": "cannot: a tiled batch that K1 cannot count from is refused",
              "RAGGED_ONE_BLOCK": "cannot: K1 stages tiles for k > 32 of reads of 150 bases and more — several blocks of 32 steps",
              "SHORT": "left out: K1 takes tiles only beside K1h (k <= 32), and a batch of reads of k bases for K1's k > 32 leaves K1h's k nothing to share",
              "NO_HIT": "left out: at sBits 7 a wave-batch of 64 x 87 windows samples ~100; the plain rows reach it in the same code",
              "REGION_ROLL": "left out: beside K1h (sBits >= 7) a wave logs ~100 keys per wave-batch and a region holds 256",
              "LOG_EXHAUSTED": "left out: as REGION_ROLL",
              **{"START_K%d%s" % (r, m): "left out: the tiled rows differ from the row-slot rows in staging only; the start is the plain rows'"
                 for r in (1, 2, 3) for m in ("", "_MARK")}},
    "spaced": {"CHUNK_ROLL": "cannot: signature rows only", "SIG_FUSED_CARRY": "cannot: signature rows only"},
    "hll": {"RESOLVE_FULL": "cannot be told: the candidates depend on the moving threshold, not on the reference", "RESOLVE_REST": "as RESOLVE_FULL",
            "NO_HIT": "as RESOLVE_FULL", "REGION_ROLL": "cannot: nthll has no hit log", "LOG_EXHAUSTED": "cannot: nthll has no hit log",
            "CHUNK_ROLL": "cannot: signature rows only", "SIG_FUSED_CARRY": "cannot: signature rows only"},
    "sig": {},
    "dump": {"RAGGED_MASK": "left out: tests/test_strand_gpu.py and tests/test_seeds_gpu.py dump every mask kind; these cases add the staging regimes only",
             "RESOLVE_REST": "cannot: the dump filter lets every window through", "NO_HIT": "cannot: the dump filter lets every window through",
             "REGION_ROLL": "cannot: no hit log", "LOG_EXHAUSTED": "cannot: no hit log", "CHUNK_ROLL": "cannot: signature rows only",
             "SIG_FUSED_CARRY": "cannot: signature rows only", "WAVE_BATCHES_2": "left out: see REGIME_EXEMPT",
             **{x: "left out: the dump tests cover (k, L) widely; these cases add the staging regimes only"
                for x in ("RAGGED_LEN", "NOTHING", "SHORT", "RAGGED_ONE_BLOCK", "RAGGED_END_IN_GROUP", "RAGGED_ZERO_LEN", "START_K0", "START_K0_MARK", "START_K2",
                          "START_K2_MARK")}},
}


def table_rows():
    import ntcard_amd
    return [s["row"] for s in ntcard_amd.k1_variant_stats()]


def test_the_diagnostic_enumerates_the_table_without_a_device():
    from ntcard_amd import _abi
    rows = table_rows()
    assert len(rows) == len(set(rows)) >= 28
    info = _abi.NtcK1VariantInfo()
    assert _abi.lib().ntc_k1_variant_stats(len(rows), info) == -1 and b"row" in _abi.lib().ntc_last_error()
    assert _abi.lib().ntc_k1_variant_stats(0, None) == -1
    assert all(mode in (0, 1, 2, 3) and pref in (10, 16) for _, mode, pref, *_ in rows)


def requirement(row):
    """the regimes a row must be launched in"""
    multi, mode, pref, dump, tiled, one, sig = row
    need = {"PARTIAL", "IDLE", "MULTI", "PREFETCH"}
    if pref == 10:
        need.add("BLOCKING")  # (a 16-chunk row exists for the strides its prefetch covers)
    if not dump:
        need.add("META")  # (every engine takes ragged batches; the dumps take none)
    if not multi and mode == 0 and pref == 10 and not dump and not tiled and not sig:
        need.add("SMALL_BLOCK")  # (strides 700 and 1000 of the plain single rows; the 16-chunk rows' strides always fit four waves)
    return need


def test_every_row_is_launched_in_every_regime_it_has():
    got = {}
    for c in kc.CASES:
        for x in kc.launches(c):
            got.setdefault(x["row"], set()).update(x["regimes"])
        assert kc.expected_row(c) in kc.expected_rows(c)
    rows = table_rows()
    assert set(got) == set(rows), set(rows) ^ set(got)
    missing = [(row, r) for row in rows for r in sorted(requirement(row) - got[row]) if (row, r) not in REGIME_EXEMPT]
    assert not missing, missing
    stale = [key for key in REGIME_EXEMPT if key[1] in got[key[0]]]
    assert not stale, stale
    # the hit log: every non-nthll family at row slots
    for fam in ("plain", "spaced", "sig"):
        assert any("LOG" in kc.claims(c) for c in kc.CASES if c.family == fam), fam


def test_one_strand_cases_come_in_both_strands():
    names = {c.name for c in kc.CASES}
    for c in kc.CASES:
        if c.strand == "forward":
            assert c.name[:-len("forward")] + "reverse" in names and c.name[:-len("forward")] + "canonical" in names


@pytest.mark.parametrize("family", FAMILIES)
def test_every_reachable_path_is_reached(family):
    reached = frozenset().union(*[kc.paths(c) for c in kc.CASES if c.family == family])
    assert reached <= ALL_LABELS, reached - ALL_LABELS
    assert set(NOT_REACHED[family]) <= ALL_LABELS
    missing = ALL_LABELS - reached - set(NOT_REACHED[family])
    assert not missing, (family, sorted(missing))
    stale = reached & set(NOT_REACHED[family])
    assert not stale, (family, sorted(stale))
    if family in ("plain", "spaced", "hll", "sig"):  # the strands of a family reach the same paths: they run the same reads
        for s in kc.ONE:
            assert frozenset().union(*[kc.paths(c) for c in kc.CASES if c.family == family and c.strand == s]) >= reached - {"RESOLVE_REST", "NO_HIT"}, s


def test_no_case_is_vacuous():
    """by the reference alone: >= 40 increments in each sample of every plane, >= 40 distinct signature values per plane, >= 40 raised registers per
    nthll plane (all 16 of them at n_bits = 4), dumps of >= 40 windows"""
    for c in kc.CASES:
        if c.kind == "dump":
            assert sum(w.size for w in kc.expected_dump(c)) >= 40, c.name
        elif c.kind == "hll":
            regs, f1 = kc.expected_hll(c, kc.batch_of(c, kc.CUS)[0])
            assert ((regs > 0).sum(axis=1) >= min(40, 1 << c.n_bits)).all() and f1.all(), (c.name, (regs > 0).sum(axis=1))
        else:
            per_sample = kc.sketch_of(c)[0].astype(np.int64).sum(axis=2)
            assert (per_sample >= 40).all(), (c.name, per_sample.tolist())
            if c.kind == "sig":
                for i in range(len(c.masks)):
                    assert kc.expected_signature(c, i, kc.batch_of(c, kc.CUS)[0])[0].size >= 40, (c.name, i)


def test_the_strands_differ():
    for c in kc.CASES:
        if not c.one or c.kind == "dump":
            continue
        other = "reverse" if c.strand == "forward" else "forward"
        for i in range(len(c.masks)):
            mine = kc.picked(c, i)
            assert not np.array_equal(mine, kc.picked(c, i, "canonical")) and not np.array_equal(mine, kc.picked(c, i, other)), (c.name, i)
        if c.kind in ("sketch", "sig"):
            assert not np.array_equal(kc.sketch_of(c)[0], kc.sketch_of(c, "canonical")[0]) and not np.array_equal(kc.sketch_of(c)[0], kc.sketch_of(c, other)[0]), c.name
        else:
            regs = [np.stack([kc.hll_model.registers(kc.picked(c, i, s), c.n_bits) for i in range(len(c.masks))]) for s in (c.strand, "canonical", other)]
            if c.n_bits >= 8:  # (16 registers of 64-bit maxima can coincide)
                assert not np.array_equal(regs[0], regs[1]) and not np.array_equal(regs[0], regs[2]), c.name


def test_replication_arithmetic():
    """a replicated case: whole copies of the base set and the head of one more, planned from the device's CUs, at least two wave-batches per wave"""
    for c in kc.CASES:
        if not c.rep:
            continue
        for cus in (64, 256, 304):
            n, stride, _, _ = kc.batch_of(c, cus)
            m, extra = kc.copies(c, n)
            assert m >= 1 and extra == (37 if c.rep == 2 else 0)
            x = kc.launches(c, cus)[-1]
            assert "MULTI" in x["regimes"] and ("PARTIAL" in x["regimes"] or c.rep != 2), (c.name, cus)
            assert n * stride <= 120 << 20, (c.name, n * stride)
