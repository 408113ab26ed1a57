"""GPU tests of nthll engines on forged k-mers (tests/hash_forge.py, tests/forged_cases.py): the decisions an engine takes on a k-mer's 64-bit value — the
canonical strand, the register its low n_bits select, the leading zeros of the rest (sink_hll's hi == 0 branch and rest == 0 skip), and whether the walk's
moving threshold lets the window through (hll_threshold_kernel: exact up to a minimum register of 29, clamped from 30 on; one threshold word per plane) —
on values chosen to sit on each decision's edge.  Registers and F1 must equal tests/hll_model.py exactly; tests/test_hash_forge_host.py pins every case
to the oracle and shows what it plans."""
import numpy as np
import pytest

import forged_cases as fc
import hll_model as hm
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401
from support import NTHLL, run_cli, to_slots

pytestmark = pytest.mark.gpu

HLL = {c.name: c for c in fc.hll_cases()}


def make(nt, c):
    if c.seeded:
        return nt.HllEngine.from_seeds(list(c.masks), n_bits=c.n_bits, strand=fc.NAMES[c.strand])
    return nt.HllEngine([len(m) for m in c.masks], n_bits=c.n_bits, strand=fc.NAMES[c.strand])


def by_reads(e, reads):
    e.submit_reads(reads)


def by_slots(e, reads):
    """equal-length reads as row slots on the device (the order of the reads is the order of the slots)"""
    L = len(reads[0])
    stride = (L + 3) // 4 * 4
    d = dev(to_slots(reads, stride))
    e.submit_device(d.data_ptr(), len(reads), L, stride)
    e.sync()  # (d is released behind this call)


def by_tiles(nt):
    def submit(e, reads):
        d = dev(nt.tile_reads(reads, len(reads[0])))
        e.submit_tiled_device(d.data_ptr(), len(reads), len(reads[0]))
        e.sync()
    return submit


def run(nt, c, submit=by_reads):
    with make(nt, c) as e:
        for s in c.submits:
            submit(e, list(s))
        return e.finish()


def assert_same(got, want, what):
    regs, f1 = got
    off = np.argwhere(regs != want[0]).tolist()
    print(what, "F1", f1.tolist(), "model", want[1].tolist(), "registers off", [(p, b, int(regs[p, b]), int(want[0][p, b])) for p, b in off[:8]])
    assert np.array_equal(f1, want[1]) and not off, what


def check(nt, name, submit=by_reads):
    c = HLL[name]
    assert_same(run(nt, c, submit), fc.hll_model(c), name)


# ---- 1. the leading-zero ladder ----
@pytest.mark.parametrize("name", [c.name for c in fc.ladder_cases()])
def test_ladder(nt, name):
    """run0 0, 1, 30, 31, 32, 33 and 63 - n_bits, a value with rest == 0, two of one bucket in either order; n_bits at both ends of the range and 16"""
    check(nt, name)


# ---- 2. strands ----
@pytest.mark.parametrize("name", [c.name for c in fc.strand_cases()])
def test_strands(nt, name):
    """either strand the smaller one by the bit under the leading one, by the number of leading zeros, and behind equal top halves (bits 63 .. 32) by bit 31;
    every strand's value selects a register of its own"""
    check(nt, name)
    check(nt, name, by_slots)


# ---- 3. the threshold between two submits, exact and clamped ----
@pytest.mark.parametrize("name", [c.name for c in fc.threshold_cases()])
def test_threshold_between_submits(nt, name):
    check(nt, name)


def test_threshold_inside_one_submit(nt):
    """16384 + 64 slots: run_hll launches the last 64 under the threshold of the registers the first 16 reads warmed"""
    check(nt, "one_submit", by_slots)


def test_every_plane_has_its_own_threshold(nt):
    check(nt, "planes_96_160")


# ---- 4. other ways in ----
def test_ragged_host_reads(nt):
    check(nt, "ladder_ragged")


def test_device_slots_window_at_the_first_a_middle_and_the_last_offset(nt):
    check(nt, "ladder_offsets", by_slots)


def test_tiled_batch_is_re_laid_out(nt):
    check(nt, "ladder_tiled", by_tiles(nt))


@pytest.mark.parametrize("name", [c.name for c in fc.spaced_cases()])
def test_spaced_seed_one_strand(nt, name):
    check(nt, name)
    check(nt, name, by_slots)


def test_merge_devices_and_reset_above_32(nt):
    a, b = ([r[1] for r in part] for part in fc.merge_parts())
    mask = ["1" * fc.LADDER_K]
    es = [nt.HllEngine([fc.LADDER_K], n_bits=16) for _ in range(2)]
    try:
        es[0].submit_reads(a)
        es[1].submit_reads(b)
        for e, part in zip(es, (a, b)):
            assert_same(e.finish(), hm.model(part, mask, sm.CANONICAL, 16), "half")
        nt.merge_devices(es)
        assert_same(es[0].finish(), hm.model(a + b, mask, sm.CANONICAL, 16), "merged")
        regs1, f11 = es[1].finish()
        assert not regs1.any() and not f11.any()
        es[0].reset()
        regs0, f10 = es[0].finish()
        assert not regs0.any() and not f10.any()
        es[0].submit_reads(b)  # after the reset the threshold starts from empty registers again
        assert_same(es[0].finish(), hm.model(b, mask, sm.CANONICAL, 16), "after reset")
    finally:
        for e in es:
            e.close()


# ---- 5. the command line ----
def test_cli_prints_the_estimate_of_the_model_s_registers(nt, tmp_path):
    c = HLL["ladder_cli"]
    (tmp_path / "ladder.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(c.submits[0])))
    regs, _ = fc.hll_model(c)
    assert int(regs.max()) == 59
    want = "F0, Exp# of distnt kmers(k=%d): %d\n" % (fc.LADDER_K, int(nt.hll_estimate(regs[0], c.n_bits)))
    r = run_cli(NTHLL, ["-k", fc.LADDER_K, "-b", c.n_bits, "ladder.fa"], cwd=tmp_path, timeout=120)
    assert r.returncode == 0 and r.stdout.decode() == want, (r.stdout, r.stderr)
