"""GPU tests of nthll engines with planes, spaced seeds and a strand (include/ntcard_hip.h: ntc_hll_create_ex; `nthll --strand / --seed / -k K,K`):
registers and F1 of every plane exactly against tests/hll_model.py (tests/test_nthll_ext_host.py pins that model to the oracle and shows that its
inputs tell the strands and the masks apart), under a moving threshold, through the other submit paths, merge and reset, and the command line."""
import functools
import gzip
import json
import os
import random

import numpy as np
import pytest

import hll_model as hm
import orc
import strand_model as sm
from gpu_support import nt, on_device  # noqa: F401
from support import GOLD, NTHLL, rseq_acgt, run_cli, to_slots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STRANDS = [("canonical", sm.CANONICAL), ("forward", sm.FORWARD), ("reverse", sm.REVERSE)]


def goldens():
    with open(os.path.join(GOLD, "nthll_goldens.json")) as f:
        return json.load(f)


def make(nt, masks, seeded, n_bits, strand):
    if seeded:
        return nt.HllEngine.from_seeds(masks, n_bits=n_bits, strand=strand)
    return nt.HllEngine([len(m) for m in masks], n_bits=n_bits, strand=strand)


def same(got, want):
    regs, f1 = got
    return regs.shape == want[0].shape and np.array_equal(f1, want[1]) and np.array_equal(regs, want[0])


# ---- 1. registers and F1 of every plane against the model ----
@pytest.mark.parametrize("name,masks,seeded,n_bits", hm.CONFIGS, ids=[c[0] for c in hm.CONFIGS])
def test_registers_match_the_model(nt, name, masks, seeded, n_bits):
    equal, ragged = sm.sketch_reads_equal(), sm.sketch_reads_ragged()
    L, stride = len(equal[0]), 152
    d = torch.from_numpy(to_slots(equal, stride)).cuda()
    for sname, strand in STRANDS:
        with make(nt, masks, seeded, n_bits, sname) as e:
            e.submit_device(d.data_ptr(), len(equal), L, stride)
            got = e.finish()
        assert same(got, hm.planes_of(hm.config_values(name, "equal"), strand, n_bits)), (name, sname, "submit_device")
        with make(nt, masks, seeded, n_bits, sname) as e:
            e.submit_reads(ragged)
            got = e.finish()
        assert same(got, hm.planes_of(hm.config_values(name, "ragged"), strand, n_bits)), (name, sname, "submit_reads")


# ---- 2. the old and the new constructor ----
def test_old_and_new_constructors_agree(nt):
    reads = sm.small_reads()
    with nt.HllEngine(32) as e:
        e.submit_reads(reads)
        regs, f1 = e.finish()
    assert regs.shape == (1 << 16,) and isinstance(f1, int)
    with nt.HllEngine([32]) as e:
        e.submit_reads(reads)
        regs2, f12 = e.finish()
    assert regs2.shape == (1, 1 << 16) and f12.shape == (1,) and f12.dtype == np.uint64
    assert np.array_equal(regs2[0], regs) and int(f12[0]) == f1
    c = next(c for c in goldens()["cases"] if c["k"] == 32 and c["n_bits"] == 16)
    assert "%016x" % orc.fnv1a64(regs) == c["fnv1a64"]
    with nt.HllEngine(32, strand="canonical") as e:  # the keyword spelled out: the same engine
        e.submit_reads(reads)
        regs3, f13 = e.finish()
    assert np.array_equal(regs3, regs) and f13 == f1


# ---- 3. the moving threshold ----
@functools.lru_cache(maxsize=None)
def short_reads():
    rng = random.Random(31)
    return tuple(sm.rseq(rng, 24, pn=0.002) for _ in range(20000))


@pytest.mark.parametrize("mask,seeded,sname,strand", [("1" * 16, False, "forward", sm.FORWARD), ("1111111101111111", True, "reverse", sm.REVERSE)],
                         ids=["k16_forward", "mask16_reverse"])
def test_the_threshold_never_drops_a_window_that_raises_a_register(nt, mask, seeded, sname, strand):
    """20 000 reads in one submit: more than the first sub-batch of 16384, so the second one runs under a threshold from 256 warm registers; the second
    submit (the reverse complements) runs under one from the start"""
    reads = list(short_reads())
    rc = [sm.revcomp(r) for r in reads]
    with make(nt, [mask], seeded, 8, sname) as e:
        e.submit_reads(reads)
        e.submit_reads(rc)
        got = e.finish()
    want = hm.model(reads + rc, [mask], strand, 8)
    assert int(want[0].min()) > 0  # every register is warm: the threshold has moved
    assert same(got, want)


# ---- 4. other ways into the engine ----
def test_a_tiled_batch_counts_like_submit_reads(nt):
    rng = random.Random(41)
    reads = [sm.rseq(rng, 40, pn=rng.choice([0.0, 0.01])) for _ in range(2048 + 5)]
    tiles = torch.from_numpy(nt.tile_reads(reads, 40)).cuda()
    with nt.HllEngine([20, 32], n_bits=10, strand="forward") as e:
        e.submit_reads(reads)
        want = e.finish()
    with nt.HllEngine([20, 32], n_bits=10, strand="forward") as e:
        e.submit_tiled_device(tiles.data_ptr(), len(reads), 40)
        got = e.finish()
    assert want[1].all() and same(got, want)


K, PL = 32, 48  # (the shape of tests/test_long_gpu.py: mixed)
STEP = PL - K + 1


def mixed():
    """about 40 sequences: every boundary length of the plan, dirty bytes, a few of several thousand bases"""
    rng = random.Random(11)
    lens = [0, K - 1, K, PL - 1, PL, PL + STEP - 1, PL + STEP, 5 * STEP + K - 1, 3001, 5003, 7777, 2222] + [rng.randrange(1, 400) for _ in range(28)]
    seqs = [bytearray(rseq_acgt(rng, n)) for n in lens]
    big = seqs[8]
    big[100] = ord("N")
    big[500:505] = b"acgtn"
    big[900] = ord("U")
    big[1200] = ord("R")
    big[2000:2000 + PL + 12] = b"N" * (PL + 12)
    seqs[9][47] = ord("N")
    seqs[9][48 + 16] = ord("n")
    seqs[10][7776] = ord("N")
    for s in seqs[12:20]:
        if len(s) > 40:
            s[len(s) // 2] = ord("N")
    return [bytes(s) for s in seqs]


def test_long_sequences_count_like_submit_reads(nt):
    seqs = mixed()
    d, offs = on_device(seqs)
    with nt.HllEngine([20, 32], n_bits=10, strand="forward") as e:
        e.submit_reads(seqs)
        want = e.finish()
    with nt.HllEngine([20, 32], n_bits=10, strand="forward") as e:
        e.submit_long_device(d.data_ptr(), offs)
        got = e.finish()
    assert want[1].all() and same(got, want)


# ---- 5. an identity that needs no model ----
def test_reverse_is_forward_over_the_reverse_complements(nt):
    reads = sm.sketch_reads_ragged()
    rc = [sm.revcomp(r) for r in reads]

    def run(e, rs):
        with e:
            e.submit_reads(rs)
            return e.finish()
    rev = run(nt.HllEngine([16, 32], n_bits=10, strand="reverse"), reads)
    fwd = run(nt.HllEngine([16, 32], n_bits=10, strand="forward"), rc)
    assert rev[1].all() and same(rev, fwd)
    mask = "1110011100111"  # a mask: with the mask reversed
    rev = run(nt.HllEngine.from_seeds([mask], n_bits=10, strand="reverse"), reads)
    fwd = run(nt.HllEngine.from_seeds([mask[::-1]], n_bits=10, strand="forward"), rc)
    assert rev[1].all() and same(rev, fwd)


# ---- 6. merge_devices ----
def test_merge_devices_folds_every_plane(nt):
    reads = sm.sketch_reads_equal()
    masks = ["1" * 16, "1" * 32]
    want = hm.model(reads, masks, sm.FORWARD, 10)
    es = [nt.HllEngine([16, 32], n_bits=10, strand="forward") for _ in range(2)]
    try:
        es[0].submit_reads(reads[0::2])
        es[1].submit_reads(reads[1::2])
        halves = [e.finish() for e in es]
        assert not np.array_equal(halves[0][0], want[0]) and not np.array_equal(halves[1][0], want[0])
        nt.merge_devices(es)
        assert same(es[0].finish(), want)  # the per-plane max and the summed F1
        regs1, f11 = es[1].finish()
        assert not regs1.any() and not f11.any()
        with nt.HllEngine([16, 32], n_bits=10, strand="reverse") as rev:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], rev])
        with nt.HllEngine([16, 32], n_bits=11, strand="forward") as other:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], other])
        with nt.HllEngine.from_seeds(["1" * 15 + "0", "1" * 32], n_bits=10, strand="forward") as other:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], other])
        assert same(es[0].finish(), want)
    finally:
        for e in es:
            e.close()


# ---- 7. reset ----
def test_reset_zeroes_every_plane(nt):
    first, second = sm.sketch_reads_equal(), sm.sketch_reads_ragged()
    with nt.HllEngine.from_seeds(["1" * 24, "1110011100111"], n_bits=9, strand="reverse") as e:
        e.submit_reads(first)
        e.reset()
        regs, f1 = e.finish()
        assert not regs.any() and not f1.any()
        e.submit_reads(second)
        got = e.finish()
    assert same(got, hm.model(second, ["1" * 24, "1110011100111"], sm.REVERSE, 9))


# ---- 8. the command line ----
def write_reads(tmp_path):
    with gzip.open(os.path.join(GOLD, "reads_small.fq.gz"), "rb") as f:
        (tmp_path / "reads.fq").write_bytes(f.read())
    return "reads.fq"


def test_cli_prints_one_line_per_plane(nt, tmp_path):
    src = write_reads(tmp_path)
    cases = [(["--strand=forward", "-k", "20,32"], ("1" * 20, "1" * 32), "forward", ["k=20", "k=32"]),
             (["--seed=111110011111"], ("111110011111",), "canonical", ["seed=111110011111"]),
             (["--strand=reverse", "--seed=111110011111"], ("111110011111",), "reverse", ["seed=111110011111"]),
             (["--strand=reverse", "-k", "32"], ("1" * 32,), "reverse", ["k=32"])]
    for args, masks, sname, labels in cases:
        regs, _ = hm.planes_of(hm.small_values(masks), sm.STRANDS[sname], 16)
        want = "".join("F0, Exp# of distnt kmers(%s): %d\n" % (lab, int(nt.hll_estimate(regs[i], 16, strand=sname))) for i, lab in enumerate(labels))
        r = run_cli(NTHLL, args + [src], cwd=tmp_path, timeout=300)
        assert r.returncode == 0 and r.stdout.decode() == want, (args, r.stdout, r.stderr)


def test_cli_canonical_is_the_reference_line(tmp_path):
    src = write_reads(tmp_path)
    r = run_cli(NTHLL, ["--strand=canonical", "-k", "32", src], cwd=tmp_path, timeout=300)
    assert r.returncode == 0 and r.stdout.decode() == goldens()["cli_k32"], r.stderr
