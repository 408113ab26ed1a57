"""GPU tests of one-strand counting on the tiled kernels (include/ntcard_hip.h: NTC_FLAG_STRAND_TILED; Engine(..., strand_tiled=True); `ntcard --strand`):
the one-strand K1h kernels + K1f through every tiled route, exact against tests/strand_model.py — the oracle's fh / rh pushed through ntComp.  Every engine
that is meant to run on the tiled pair is created with NTC_FLAG_REQUIRE_TILED, so a quiet fall-back to the general kernel fails the test."""
import functools
import os
import random

import numpy as np
import pytest

import k1f_cases as kc
import strand_model as sm
from gpu_support import nt, on_device  # noqa: F401
from support import GOLD, NTCARD, assert_same_sketch, gap_mask, run_cli

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ONE = [("forward", sm.FORWARD), ("reverse", sm.REVERSE)]
BOTH = pytest.mark.parametrize("sname,strand", ONE, ids=[s for s, _ in ONE])
R_BITS = sm.R_BITS
KS = [12, 17, 25, 32]


# ---- read sets (fixed seeds) and the model's per-read values, computed once per (set, mask) ----
@functools.lru_cache(maxsize=None)
def equal_reads(L, n=2049, seed=31):
    """n reads of L bases, a non-base byte or two in about 0.4 % of them"""
    rng = random.Random(seed + L)
    return tuple(sm.rseq(rng, L, pn=2.0 / L if rng.random() < 0.004 else 0.0) for _ in range(n))


@functools.lru_cache(maxsize=None)
def ragged_reads(n=2100, seed=32):
    rng = random.Random(seed)
    return tuple(sm.rseq(rng, rng.randint(145, 160), pn=rng.choice([0.0, 0.0, 0.004])) for _ in range(n))


@functools.lru_cache(maxsize=None)
def per_read(reads, mask):
    """[(fs, rs)] per read"""
    return tuple(sm.window_values(r, mask)[:2] for r in reads)


def want(reads, masks, strand, s_bits=7, r_bits=R_BITS, upto=None):
    vals = []
    for m in masks:
        pr = per_read(tuple(reads), m)[:upto]
        vals.append((np.concatenate([p[0] for p in pr]), np.concatenate([p[1] for p in pr])))
    return sm.sketch_of(vals, strand, r_bits, s_bits)


def flags_of(nt, sname, extra=0, require=True):
    return (nt.FLAG_STRAND_FORWARD if sname == "forward" else nt.FLAG_STRAND_REVERSE) | nt.FLAG_STRAND_TILED | (nt.FLAG_REQUIRE_TILED if require else 0) | extra


def tiled(e, reads, L, keep):
    t = torch.from_numpy(__import__("ntcard_amd").tile_reads(list(reads), L)).cuda()
    keep.append(t)
    e.submit_tiled_device(t.data_ptr(), len(reads), L)


# ---- 1: fails without the feature ----
def test_require_tiled_accepts_a_strand_engine_with_the_flag(nt):
    reads = equal_reads(150)
    assert any(b"N" in r or b"n" in r or b"R" in r or b"Y" in r or b"-" in r for r in reads)
    t = torch.from_numpy(nt.tile_reads(list(reads), 150)).cuda()
    for sname, strand in ONE:
        sflag = nt.FLAG_STRAND_FORWARD if sname == "forward" else nt.FLAG_STRAND_REVERSE
        with nt.Engine([32], r_bits=18, s_bits=7, flags=nt.FLAG_REQUIRE_TILED | sflag | nt.FLAG_STRAND_TILED) as e:
            e.submit_tiled_device(t.data_ptr(), len(reads), 150)
            assert_same_sketch(e.finish(counters=True), want(reads, ["1" * 32], strand, r_bits=18), sname)
        with nt.Engine([32], r_bits=18, s_bits=7, flags=nt.FLAG_REQUIRE_TILED | sflag) as e:  # without the flag: as before
            with pytest.raises(nt.NtcError, match="REQUIRE_TILED") as ei:
                e.submit_tiled_device(t.data_ptr(), len(reads), 150)
            assert ei.value.code == -1
            tc, _, f1 = e.finish(counters=True)
            assert not f1.any() and not tc.any()


# ---- 2: routes ----
@BOTH
@pytest.mark.parametrize("k", KS)
def test_equal_length_batches(nt, k, sname, strand):
    for L in (k + 8, 47, 150, 160):
        reads = equal_reads(L)
        keep = []
        with nt.Engine([k], r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname)) as e:
            tiled(e, reads, L, keep)
            assert_same_sketch(e.finish(counters=True), want(reads, ["1" * k], strand), (k, L, sname))


@BOTH
@pytest.mark.parametrize("n", [1, 2048, 2049, 4100])
def test_batch_sizes(nt, n, sname, strand):
    reads = equal_reads(47, 4100)[:n]
    keep = []
    with nt.Engine([32], r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname)) as e:
        tiled(e, reads, 47, keep)
        assert_same_sketch(e.finish(counters=True), want(equal_reads(47, 4100), ["1" * 32], strand, upto=n), (n, sname))


def all_routes(nt, e, equal, ragged, keep):
    """equal-length tiles, ragged tiles, both as two bins of one call, host reads of equal and of mixed lengths: 3 x equal + 3 x ragged"""
    L = len(equal[0])
    t = torch.from_numpy(nt.tile_reads(list(equal), L)).cuda()
    rt, tails, _ = nt.tile_reads_ragged(list(ragged), 10)
    drt, dtl = torch.from_numpy(rt).cuda(), torch.from_numpy(tails).cuda()
    keep += [t, drt, dtl]
    e.submit_tiled_device(t.data_ptr(), len(equal), L)
    e.submit_tiled_ragged_device(drt.data_ptr(), len(ragged), 10, dtl.data_ptr())
    e.submit_tiled_bins_device([(t.data_ptr(), len(equal), L, 0), (drt.data_ptr(), len(ragged), 160, dtl.data_ptr())])
    e.submit_reads(list(equal))
    e.submit_reads(list(ragged))
    e.sync()


@BOTH
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("mode", ["default", "defer", "direct", "partition"])
def test_every_tiled_route_and_update_mode(nt, mode, k, sname, strand):
    extra = {"default": 0, "defer": nt.FLAG_DEFER_REDO, "direct": nt.FLAG_DIRECT_ATOMICS, "partition": nt.FLAG_ALWAYS_LOG | nt.FLAG_PARTITION_ALWAYS}[mode]
    equal, ragged = equal_reads(150), ragged_reads()
    we, wr = want(equal, ["1" * k], strand), want(ragged, ["1" * k], strand)
    keep = []
    with nt.Engine([k], r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname, extra)) as e:
        all_routes(nt, e, equal, ragged, keep)
        assert_same_sketch(e.finish(counters=True), (3 * we[0] + 3 * wr[0], 3 * we[1] + 3 * wr[1]), (mode, k, sname))


# ---- 3: sBits and gaps ----
@BOTH
@pytest.mark.parametrize("s_bits", [8, 11])
def test_larger_s_bits(nt, s_bits, sname, strand):
    reads = equal_reads(150)
    keep = []
    with nt.Engine([32], r_bits=12, s_bits=s_bits, flags=flags_of(nt, sname)) as e:
        tiled(e, reads, 150, keep)
        assert_same_sketch(e.finish(counters=True), want(reads, ["1" * 32], strand, s_bits=s_bits, r_bits=12), (s_bits, sname))


@BOTH
@pytest.mark.parametrize("k,gap", [(12, 2), (32, 8)])
def test_gap_seeds(nt, k, gap, sname, strand):
    equal, ragged = equal_reads(150), ragged_reads()
    m = gap_mask(k, gap)
    we, wr = want(equal, [m], strand), want(ragged, [m], strand)
    keep = []
    with nt.Engine([k], gap=gap, r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname)) as e:
        all_routes(nt, e, equal, ragged, keep)
        assert_same_sketch(e.finish(counters=True), (3 * we[0] + 3 * wr[0], 3 * we[1] + 3 * wr[1]), (k, gap, sname))


# ---- 4: K1f's slow path ----
@BOTH
@pytest.mark.parametrize("v", kc.SLOT_BYTES)
def test_slow_path_by_a_table_slot_byte(nt, v, sname, strand):
    case = kc.slot_bytes(v)
    exp = want(case.reads, ["1" * case.k], strand, s_bits=case.s_bits)
    t = torch.from_numpy(kc.tile(case.reads, case.read_len)).cuda()
    with nt.Engine([case.k], r_bits=R_BITS, s_bits=case.s_bits, flags=flags_of(nt, sname)) as e:
        e.submit_tiled_device(t.data_ptr(), len(case.reads), case.read_len)
        assert_same_sketch(e.finish(counters=True), exp, (v, sname))


@BOTH
@pytest.mark.parametrize("sus_cap", [None, "7"], ids=["dense", "dense-overflow"])
def test_dense_suspects(nt, monkeypatch, sus_cap, sname, strand):
    """kc.dense: 1500 suspects that end in one block; with NTC_K1H_SUS_CAP = 7 the suspect regions overflow and k1h_slow_kernel re-derives every window near a
    dirty piece with the strand's own value"""
    if sus_cap:
        monkeypatch.setenv("NTC_K1H_SUS_CAP", sus_cap)
    case = kc.dense()
    exp = want(case.reads, ["1" * case.k], strand, s_bits=case.s_bits)
    t = torch.from_numpy(kc.tile(case.reads, case.read_len)).cuda()
    for log_entries in (0, 1 << 18):
        with nt.Engine([case.k], r_bits=R_BITS, s_bits=case.s_bits, flags=flags_of(nt, sname), log_entries=log_entries) as e:
            e.submit_tiled_device(t.data_ptr(), len(case.reads), case.read_len)
            assert_same_sketch(e.finish(counters=True), exp, (sus_cap, log_entries, sname))


# ---- 5: identities ----
def test_reverse_is_forward_over_the_reverse_complements(nt):
    reads = equal_reads(150)
    rc = tuple(sm.revcomp(r) for r in reads)
    res = {}
    for sname, rs in (("reverse", reads), ("forward", rc)):
        keep = []
        with nt.Engine([17, 32], r_bits=16, s_bits=7, flags=flags_of(nt, sname)) as e:
            tiled(e, rs, 150, keep)
            res[sname] = e.finish(counters=True)
    assert all(np.array_equal(a, b) for a, b in zip(res["reverse"], res["forward"]))
    assert res["reverse"][0].any()


@BOTH
def test_tiled_route_equals_the_general_kernel_and_f1_the_canonical_engine(nt, sname, strand):
    rng = random.Random(8)
    reads = [sm.rseq(rng, 150, pn=rng.choice([0.0, 0.0, 0.004])) for _ in range(3000)]
    t = torch.from_numpy(nt.tile_reads(reads, 150)).cuda()
    out = {}
    for name, kw in (("tiled", dict(strand=sname, strand_tiled=True, flags=nt.FLAG_REQUIRE_TILED)), ("general", dict(strand=sname, strand_tiled=False)), ("canonical", {})):
        with nt.Engine([21, 25, 31], r_bits=16, s_bits=7, **kw) as e:
            e.submit_tiled_device(t.data_ptr(), len(reads), 150)
            e.submit_reads(reads)
            out[name] = e.finish(counters=True)
    assert all(np.array_equal(a, b) for a, b in zip(out["tiled"], out["general"]))
    assert np.array_equal(out["tiled"][2], out["canonical"][2]) and out["tiled"][2].all()
    assert not np.array_equal(out["tiled"][0], out["canonical"][0])


def test_merge_devices_ignores_the_flag(nt):
    reads = equal_reads(150)
    exp = want(reads, ["1" * 32], sm.FORWARD)
    es = [nt.Engine([32], r_bits=R_BITS, s_bits=7, strand="forward", strand_tiled=True), nt.Engine([32], r_bits=R_BITS, s_bits=7, strand="forward")]
    try:
        es[0].submit_reads(list(reads[0::2]))
        es[1].submit_reads(list(reads[1::2]))
        nt.merge_devices(es)
        assert_same_sketch(es[0].finish(counters=True), exp, "merge")
    finally:
        for e in es:
            e.close()


# ---- 6: a partly qualifying list ----
@BOTH
def test_partly_qualifying_list_stays_on_the_general_kernel(nt, sname, strand):
    reads = equal_reads(150)
    exp = want(reads, ["1" * 32, "1" * 64], strand)
    keep = []
    with nt.Engine([32, 64], r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname, require=False)) as e:
        tiled(e, reads, 150, keep)
        assert_same_sketch(e.finish(counters=True), exp, sname)
    with nt.Engine([32, 64], r_bits=R_BITS, s_bits=7, flags=flags_of(nt, sname)) as e:
        with pytest.raises(nt.NtcError, match="REQUIRE_TILED"):
            tiled(e, reads, 150, keep)
        tc, _, f1 = e.finish(counters=True)
        assert not f1.any() and not tc.any()


# ---- 7: long sequences ----
@functools.lru_cache(maxsize=None)
def long_seqs():
    rng = random.Random(17)
    seqs = []
    for n in (2000, 3100, 4097, 5000, 2500):
        s = bytearray(sm.rseq(rng, n))
        for _ in range(3):  # runs of N
            p = rng.randrange(0, n - 40)
            s[p:p + rng.choice([1, 7, 33])] = b"N" * rng.choice([1, 7, 33])
        seqs.append(bytes(s[:n]))
    return tuple(seqs)


@pytest.mark.parametrize("kl", [(32,), (21, 25, 31)], ids=str)
def test_long_sequences_are_cut_for_a_strand_engine_with_the_flag(nt, kl):
    seqs = long_seqs()
    PL = 48 + 16
    d, offs = on_device(seqs)
    exp = want(seqs, ["1" * k for k in kl], sm.FORWARD)
    with nt.Engine(list(kl), r_bits=R_BITS, s_bits=7, flags=flags_of(nt, "forward")) as e:
        e.submit_long_device(d.data_ptr(), offs, PL)
        assert_same_sketch(e.finish(counters=True), exp, kl)
        assert e.long_stats() == (sum(nt.long_plan(max(kl), PL, len(s))[0] for s in seqs), len(seqs))
    with nt.Engine(list(kl), r_bits=R_BITS, s_bits=7, strand="forward") as e:  # without the flag: gathered whole, as before
        e.submit_long_device(d.data_ptr(), offs, PL)
        assert_same_sketch(e.finish(counters=True), exp, kl)
        assert e.long_stats() == (0, 0)


# ---- 8: CLI ----
def test_cli_strand_kernels_write_the_same_bytes(tmp_path):
    src = os.path.join(GOLD, "reads_small.fq.gz")
    out = {}
    for kern in ("tiled", "general"):
        r = run_cli(NTCARD, ["-k", "32", "--strand=forward", "--strand-kernel=" + kern, "-p", kern, src], cwd=tmp_path, timeout=600)
        assert r.returncode == 0, r.stderr
        out[kern] = (tmp_path / (kern + "_k32.hist")).read_bytes()
    assert out["tiled"] == out["general"] and len(out["tiled"]) > 1000
    r = run_cli(NTCARD, ["-k", "32", "--strand=forward", "-p", "dflt", src], cwd=tmp_path, timeout=600)  # the default is tiled
    assert r.returncode == 0 and (tmp_path / "dflt_k32.hist").read_bytes() == out["tiled"]
    r = run_cli(NTCARD, ["-k", "32", "--strand-kernel=sideways", "-p", "x", src], cwd=tmp_path, timeout=60)
    assert r.returncode == 1 and b"--strand-kernel" in r.stderr
