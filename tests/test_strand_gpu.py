"""GPU tests of one-strand counting (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE, ntc_hash_dump_strand_device; `ntcard --strand`):
hashes window for window and sketches exactly against tests/strand_model.py (tests/test_strand_host.py anchors that model and shows that its
inputs tell the strands apart), through every submit path and update mode, plus identities that need no model.  Every comparison is exact."""
import functools
import os
import random

import numpy as np
import pytest

import orc
import strand_model as sm
from gpu_support import nt  # noqa: F401
from support import GOLD, NTCARD, run_cli, to_slots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ONE = [("forward", sm.FORWARD), ("reverse", sm.REVERSE)]


def make(nt, masks, gap, **kw):
    """the engine of a SKETCH_CONFIGS row: a k list, a -g seed, or a list of masks"""
    if gap < 0:
        return nt.Engine.from_seeds(masks, **kw)
    return nt.Engine([len(m) for m in masks], gap=gap, **kw)


@functools.lru_cache(maxsize=None)
def model_values(name, which):
    masks = next(c[1] for c in sm.SKETCH_CONFIGS if c[0] == name)
    return sm.values_of(sm.sketch_reads_equal() if which == "equal" else sm.sketch_reads_ragged(), masks)


SPANS = [1, 12, 31, 32, 33, 64, 97, 200]


@pytest.mark.parametrize("k", SPANS)
def test_hash_dump_matches_the_model(nt, k):
    rng = random.Random(13 * k)
    for L in sorted({max(1, k - 1), k, k + 5, 150, 151}):
        for n in (128, 64 + 37):  # full waves; a partial last wave
            reads = [sm.rseq(rng, L, pn=rng.choice([0.0, 0.0, 0.02])) for _ in range(n)]
            stride = (L + 3) & ~3
            d = torch.from_numpy(to_slots(reads, stride)).cuda()
            maxw = max(L - k + 1, 1)
            for m in sm.masks_for(k):
                vals = [sm.window_values(r, m) for r in reads]
                out = {}
                for strand in (0, 1, 2):
                    dh = torch.zeros(n * maxw, dtype=torch.int64, device="cuda")
                    dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                    nt.hash_dump_strand_device(d.data_ptr(), n, L, stride, m, strand, maxw, dh.data_ptr(), dc.data_ptr())
                    torch.cuda.synchronize()
                    out[strand] = (dh.cpu().numpy().view(np.uint64).reshape(n, maxw), dc.cpu().numpy())
                for strand in (1, 2):
                    hh, cc = out[strand]
                    for i, (fs, rs, _) in enumerate(vals):
                        want = sm.pick(fs, rs, strand)
                        assert cc[i] == len(want), (k, L, m, strand, i)
                        assert np.array_equal(hh[i, :len(want)], want), (k, L, m, strand, i)
                # strand 0 is ntc_hash_dump_seed_device bit for bit
                dh = torch.zeros(n * maxw, dtype=torch.int64, device="cuda")
                dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                nt.hash_dump_seed_device(d.data_ptr(), n, L, stride, m, maxw, dh.data_ptr(), dc.data_ptr())
                torch.cuda.synchronize()
                assert np.array_equal(out[0][0], dh.cpu().numpy().view(np.uint64).reshape(n, maxw)) and np.array_equal(out[0][1], dc.cpu().numpy())


def run_paths(nt, e_factory, equal, ragged):
    """-> {path: (t_counter, f1)} of the equal-length set (row slots, tiles, host) and the ragged set (host, spans, ragged tiles, bins)"""
    res = {}
    L = len(equal[0])
    stride = (L + 3) & ~3
    d = torch.from_numpy(to_slots(equal, stride)).cuda()
    tiles = torch.from_numpy(np.ascontiguousarray(__import__("ntcard_amd").tile_reads(equal, L))).cuda()
    with e_factory() as e:
        e.submit_device(d.data_ptr(), len(equal), L, stride)
        res["submit_device"] = e.finish(counters=True)
    with e_factory() as e:
        e.submit_tiled_device(tiles.data_ptr(), len(equal), L)
        res["submit_tiled_device"] = e.finish(counters=True)
    with e_factory() as e:
        e.submit_reads(equal)
        res["submit_equal"] = e.finish(counters=True)
    with e_factory() as e:
        e.submit_reads(ragged)
        res["submit_ragged"] = e.finish(counters=True)
    with e_factory() as e:
        buf = b"@".join(ragged)
        starts = np.cumsum([0] + [len(r) + 1 for r in ragged[:-1]]).astype(np.uint64)
        e.submit_spans(buf, starts, np.array([len(r) for r in ragged], dtype=np.uint32))
        res["submit_spans"] = e.finish(counters=True)
    t, tails, _ = nt.tile_reads_ragged(ragged, 10)
    dt, dtl = torch.from_numpy(t).cuda(), torch.from_numpy(tails).cuda()
    with e_factory() as e:
        e.submit_tiled_ragged_device(dt.data_ptr(), len(ragged), 10, dtl.data_ptr())
        res["submit_tiled_ragged_device"] = e.finish(counters=True)
    with e_factory() as e:  # both sets as two bins of one call: an equal-length one and a ragged one
        e.submit_tiled_bins_device([(tiles.data_ptr(), len(equal), L, 0), (dt.data_ptr(), len(ragged), 160, dtl.data_ptr())])
        res["submit_tiled_bins_device"] = e.finish(counters=True)
    return res


@pytest.mark.parametrize("name,masks,gap,s_bits", sm.SKETCH_CONFIGS, ids=[c[0] for c in sm.SKETCH_CONFIGS])
def test_sketches_match_the_model_on_every_submit_path(nt, name, masks, gap, s_bits):
    equal, ragged = sm.sketch_reads_equal(), sm.sketch_reads_ragged()
    for sname, strand in ONE:
        want_e = sm.sketch_of(model_values(name, "equal"), strand, sm.R_BITS, s_bits)
        want_r = sm.sketch_of(model_values(name, "ragged"), strand, sm.R_BITS, s_bits)
        res = run_paths(nt, lambda: make(nt, masks, gap, r_bits=sm.R_BITS, s_bits=s_bits, strand=sname), equal, ragged)
        for path, (tc, _, f1) in res.items():
            if path == "submit_tiled_bins_device":
                assert np.array_equal(f1, want_e[1] + want_r[1]), (name, sname, path)
                assert np.array_equal(tc, want_e[0] + want_r[0]), (name, sname, path)
                continue
            want = want_e if path in ("submit_device", "submit_tiled_device", "submit_equal") else want_r
            assert np.array_equal(f1, want[1]), (name, sname, path)
            assert np.array_equal(tc, want[0]), (name, sname, path)


@pytest.mark.parametrize("name", ["k32", "klist", "seeds"])
def test_sketches_match_the_model_in_every_update_mode(nt, name):
    _, masks, gap, s_bits = next(c for c in sm.SKETCH_CONFIGS if c[0] == name)
    equal, ragged = sm.sketch_reads_equal(), sm.sketch_reads_ragged()
    modes = [nt.FLAG_DIRECT_ATOMICS, nt.FLAG_ALWAYS_LOG | nt.FLAG_PARTITION_ALWAYS, nt.FLAG_DEFER_REDO]
    if gap == 0 and name != "seeds":
        modes.append(nt.FLAG_SIMPLE_KERNEL)  # (plain k: the independent device cross-check)
    for sname, strand in ONE:
        we = sm.sketch_of(model_values(name, "equal"), strand, sm.R_BITS, s_bits)
        wr = sm.sketch_of(model_values(name, "ragged"), strand, sm.R_BITS, s_bits)
        L = len(equal[0])
        d = torch.from_numpy(to_slots(equal, 152)).cuda()
        tiles = torch.from_numpy(nt.tile_reads(equal, L)).cuda()
        for flags in modes:
            with make(nt, masks, gap, r_bits=sm.R_BITS, s_bits=s_bits, strand=sname, flags=flags) as e:
                e.submit_device(d.data_ptr(), len(equal), L, 152)
                e.submit_reads(ragged)
                if not flags & nt.FLAG_SIMPLE_KERNEL:
                    e.submit_tiled_device(tiles.data_ptr(), len(equal), L)
                e.sync()
                tc, _, f1 = e.finish(counters=True)
            mult = 1 if flags & nt.FLAG_SIMPLE_KERNEL else 2
            assert np.array_equal(f1, mult * we[1] + wr[1]), (name, sname, flags)
            assert np.array_equal(tc, mult * we[0] + wr[0]), (name, sname, flags)


def test_a_long_read_is_chunked_by_submit(nt):
    rng = random.Random(5)
    reads = [sm.rseq(rng, 30000, pn=0.0005), sm.rseq(rng, 151), sm.rseq(rng, 7)]
    masks = ["1" * 32, "1" * 64]
    for sname, strand in ONE:
        want = sm.model_sketch(reads, masks, strand, sm.R_BITS, 3)
        with nt.Engine([32, 64], r_bits=sm.R_BITS, s_bits=3, strand=sname) as e:
            e.submit_reads(reads)
            tc, _, f1 = e.finish(counters=True)
        assert np.array_equal(f1, want[1]) and np.array_equal(tc, want[0]), sname


def sketch(nt, reads, masks=None, klist=None, gap=0, s_bits=5, r_bits=16, **kw):
    e = nt.Engine.from_seeds(masks, r_bits=r_bits, s_bits=s_bits, **kw) if masks else nt.Engine(klist, gap=gap, r_bits=r_bits, s_bits=s_bits, **kw)
    with e:
        e.submit_reads(reads)
        return e.finish(counters=True)


def test_reverse_is_forward_over_the_reverse_complements(nt):
    rng = random.Random(6)
    reads = [sm.rseq(rng, rng.choice([40, 150, 151]), pn=rng.choice([0.0, 0.01])) for _ in range(3000)]
    rc = [sm.revcomp(r) for r in reads]
    for klist in ([32], [16, 24, 32, 48], [97]):
        tr, pr, fr = sketch(nt, reads, klist=klist, strand="reverse")
        tf, pf, ff = sketch(nt, rc, klist=klist, strand="forward")
        assert np.array_equal(fr, ff) and np.array_equal(tr, tf) and np.array_equal(pr, pf), klist
    for mask in ("1110011100111", "0" + "1" * 30, "1" * 20 + "0" * 9 + "1" * 35):  # a mask: with the mask reversed
        tr, _, fr = sketch(nt, reads, masks=[mask], strand="reverse")
        tf, _, ff = sketch(nt, rc, masks=[mask[::-1]], strand="forward")
        assert np.array_equal(fr, ff) and np.array_equal(tr, tf), mask


def test_f1_is_strand_blind_and_canonical_is_unchanged(nt):
    reads = sm.small_reads()[:6000]
    klist = [16, 32, 48]
    oc, of1 = orc.sketch_reads(reads, klist, 0, 18, 7)
    base = sketch(nt, reads, klist=klist, r_bits=18, s_bits=7)
    canon = sketch(nt, reads, klist=klist, r_bits=18, s_bits=7, strand="canonical")
    assert np.array_equal(base[2], of1) and np.array_equal(base[0], oc)
    assert all(np.array_equal(a, b) for a, b in zip(base, canon))
    fwd = sketch(nt, reads, klist=klist, r_bits=18, s_bits=7, strand="forward")
    rev = sketch(nt, reads, klist=klist, r_bits=18, s_bits=7, flags=nt.FLAG_STRAND_REVERSE)
    assert np.array_equal(fwd[2], of1) and np.array_equal(rev[2], of1)
    assert not np.array_equal(fwd[0], oc) and not np.array_equal(rev[0], oc) and not np.array_equal(fwd[0], rev[0])


def test_require_tiled_refuses_a_strand_engine(nt):
    n, L = 2048, 150
    rng = random.Random(3)
    tiles = torch.from_numpy(nt.tile_reads([sm.rseq(rng, L) for _ in range(n)], L)).cuda()
    with nt.Engine([32], r_bits=18, s_bits=7, flags=nt.FLAG_REQUIRE_TILED | nt.FLAG_STRAND_FORWARD) as e:
        with pytest.raises(nt.NtcError, match="REQUIRE_TILED") as ei:
            e.submit_tiled_device(tiles.data_ptr(), n, L)
        assert ei.value.code == -1  # NTC_ERR_ARG
        tc, _, f1 = e.finish(counters=True)
    assert not f1.any() and not tc.any()


def test_merges_and_log_round_trips(nt):
    equal = sm.sketch_reads_equal()
    name, masks, gap, s_bits = sm.SKETCH_CONFIGS[0]
    want = sm.sketch_of(model_values(name, "equal"), sm.FORWARD, sm.R_BITS, s_bits)
    kw = dict(r_bits=sm.R_BITS, s_bits=s_bits)
    es = [nt.Engine([32], strand="forward", **kw) for _ in range(2)]
    try:
        es[0].submit_reads(equal[0::2])
        es[1].submit_reads(equal[1::2])
        nt.merge_devices(es)
        tc, _, f1 = es[0].finish(counters=True)
        assert np.array_equal(f1, want[1]) and np.array_equal(tc, want[0])
        with nt.Engine([32], **kw) as canon:  # a forward and a canonical engine: refused, both unchanged
            canon.submit_reads(equal)
            before = canon.finish(counters=True)
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], canon])
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([canon, es[0]])
            after = canon.finish(counters=True)
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
        with nt.Engine([32], strand="reverse", **kw) as rev:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], rev])
        tc2, _, f12 = es[0].finish(counters=True)
        assert np.array_equal(f12, want[1]) and np.array_equal(tc2, want[0])
    finally:
        for e in es:
            e.close()
    # merge_counters: a dumped image added into a fresh forward engine, twice
    with nt.Engine([32], strand="forward", **kw) as e:
        e.merge_counters(want[0], want[1])
        e.submit_reads(equal)
        tc, _, f1 = e.finish(counters=True)
    assert np.array_equal(f1, 2 * want[1]) and np.array_equal(tc, 2 * want[0])
    # log_export / log_replace: the pending log of a forward engine moved into another one
    with nt.Engine([32], strand="forward", flags=nt.FLAG_ALWAYS_LOG, **kw) as a, nt.Engine([32], strand="forward", flags=nt.FLAG_ALWAYS_LOG, **kw) as b:
        a.submit_reads(equal)
        a.sync()
        counts = a.log_export(2)
        offs = [0, counts[0]]
        keys = torch.zeros(max(1, sum(counts)), dtype=torch.int32, device="cuda")
        assert a.log_export(2, keys.data_ptr(), offs) == counts
        b.log_replace(keys.data_ptr(), sum(counts))
        tc, _, _ = b.finish(counters=True)
        assert sum(counts) == int(want[0].astype(np.int64).sum()) and np.array_equal(tc, want[0])


def test_cli_strand_outputs_match_the_model(tmp_path):
    src = os.path.join(GOLD, "reads_small.fq.gz")
    reads = sm.small_reads()
    cases = [(["-k", "32"], ["1" * 32], ["x_k32.hist"]), (["-k", "16,48"], ["1" * 16, "1" * 48], ["x_k16.hist", "x_k48.hist"]),
             (["-k", "12", "-g", "2"], [sm.gap_mask(12, 2)], ["x_k12.hist"]), (["--seed=1110011100111"], ["1110011100111"], ["x_seed1_k13.hist"])]
    for args, masks, files in cases:
        vals = sm.values_of(reads, masks)
        for sname, strand in ONE:
            for f in tmp_path.glob("x_*"):
                f.unlink()
            r = run_cli(NTCARD, args + ["--strand=" + sname, "-p", "x", src], cwd=tmp_path, timeout=600)
            assert r.returncode == 0, r.stderr
            tc, f1 = sm.sketch_of(vals, strand, 27, 7)
            for mi, fn in enumerate(files):
                assert (tmp_path / fn).read_bytes() == orc.hist_from_counters(tc[mi], int(f1[mi]), 27, 7), (args, sname, fn)


def test_cli_strand_canonical_is_the_committed_reference_output(tmp_path):
    src = os.path.join(GOLD, "reads_small.fq.gz")
    for args, gold in ((["-k", "12", "-g", "2"], {"out_k12.hist": "ref_k12_g2__out_k12.hist"}), (["-k", "32"], {"out_k32.hist": "ref_k32__out_k32.hist"}),
                       (["-k", "16,24,32,48"], {"out_k%d.hist" % k: "ref_multi__out_k%d.hist" % k for k in (16, 24, 32, 48)})):
        r = run_cli(NTCARD, args + ["--strand=canonical", "-p", "out", src], cwd=tmp_path, timeout=600)
        assert r.returncode == 0, r.stderr
        for fn, g in gold.items():
            assert (tmp_path / fn).read_bytes() == open(os.path.join(GOLD, g), "rb").read(), (args, fn)
