"""CPU tests of nthll engines with planes, spaced seeds and a strand (include/ntcard_hip.h: ntc_hll_create_ex, ntc_hll_estimate_strand; `nthll --strand
/ --seed / -k K,K`): the model the GPU tests compare against (tests/hll_model.py) is pinned to the oracle, its inputs tell the strands and the masks
apart, the strand estimate is the reference's with the alpha not halved, and every malformed argument is refused before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

import hll_model as hm
import orc
import strand_model as sm
from ntcard_amd import _abi
from support import NTHLL, hll_create_ex, run_cli

ERR_ARG = -1
FWD, REV = 512, 1024


# ---- the model ----
@pytest.mark.parametrize("k,b", [(32, 16), (20, 12)])
def test_model_registers_are_the_oracles(k, b):
    reads = sm.small_reads()
    regs, f1 = hm.planes_of(hm.small_values(("1" * k,)), sm.CANONICAL, b)
    want, _ = orc.hll_reads(reads, k, b)
    assert np.array_equal(regs[0], want)
    assert int(f1[0]) == sum(len(orc.hash_read(r, k)[0]) for r in reads)


def test_clz64():
    x = np.array([1, 2, 3, 1 << 31, 1 << 32, (1 << 63) | 1, (1 << 64) - 1, 0x00f0000000000000], dtype=np.uint64)
    assert hm.clz64(x).tolist() == [63, 62, 62, 32, 31, 0, 0, 8]


def test_the_inputs_tell_the_strands_and_the_masks_apart():
    """a GPU test that passes on these reads cannot pass with the strand or the mask ignored"""
    reads = sm.sketch_reads_equal()
    vals = sm.values_of(reads, ["1" * 32])
    c, f, r = (hm.planes_of(vals, s, 10)[0][0] for s in (sm.CANONICAL, sm.FORWARD, sm.REVERSE))
    assert not np.array_equal(c, f) and not np.array_equal(c, r) and not np.array_equal(f, r)
    plain = hm.planes_of(sm.values_of(reads, ["1" * 13]), sm.CANONICAL, 10)[0][0]
    masked = hm.planes_of(sm.values_of(reads, ["1110011100111"]), sm.CANONICAL, 10)[0][0]
    assert not np.array_equal(plain, masked)


def test_reverse_registers_are_the_forward_registers_of_the_reverse_complements():
    reads = sm.sketch_reads_ragged()
    rc = [sm.revcomp(r) for r in reads]
    for mask in ("1" * 32, "1" * 16):
        rev = hm.model(reads, [mask], sm.REVERSE, 10)
        fwd = hm.model(rc, [mask], sm.FORWARD, 10)
        assert np.array_equal(rev[0], fwd[0]) and np.array_equal(rev[1], fwd[1])
    rev = hm.model(reads, ["1110011100111"], sm.REVERSE, 10)  # a mask: with the mask reversed
    fwd = hm.model(rc, ["1110011100111"[::-1]], sm.FORWARD, 10)
    assert np.array_equal(rev[0], fwd[0]) and np.array_equal(rev[1], fwd[1])


# ---- ntc_hll_estimate_strand ----
@pytest.mark.parametrize("b", [8, 12, 16])
def test_estimate_strand(b):
    import ntcard_amd as nt
    L = _abi.lib()
    rng = np.random.default_rng(b)
    regs = rng.integers(0, 40, size=1 << b, dtype=np.uint8)
    base, est = C.c_double(), C.c_double()
    assert L.ntc_hll_estimate(regs.ctypes.data, b, C.byref(base)) == 0
    assert base.value == orc.lib().orc_hll_estimate(regs.ctypes.data, b)
    assert L.ntc_hll_estimate_strand(regs.ctypes.data, b, 0, C.byref(est)) == 0
    assert est.value == base.value  # bit for bit
    for strand in (1, 2):  # the alpha is not halved, and halving is exact in IEEE double
        assert L.ntc_hll_estimate_strand(regs.ctypes.data, b, strand, C.byref(est)) == 0
        assert est.value == 2.0 * base.value
    assert L.ntc_hll_estimate_strand(regs.ctypes.data, b, 3, C.byref(est)) == ERR_ARG
    assert b"strand" in L.ntc_last_error()
    assert nt.hll_estimate(regs, b) == base.value and nt.hll_estimate(regs, b, strand="canonical") == base.value
    assert nt.hll_estimate(regs, b, strand="forward") == 2.0 * base.value == nt.hll_estimate(regs, b, strand="reverse")
    with pytest.raises(ValueError):
        nt.hll_estimate(regs, b, strand="both")


# ---- ntc_hll_create_ex: every argument error comes before the device (this test runs where there is none) ----
def create_ex(**kw):
    rc, h, L = hll_create_ex(**kw)
    if h:
        L.ntc_destroy(h)
    return rc, L.ntc_last_error().decode()


BAD_CONFIGS = {
    "both strand flags": dict(k=[32], flags=FWD | REV),
    "another flag": dict(k=[32], flags=1),
    "another flag beside a strand": dict(k=[32], flags=FWD | 64),
    "both lists": dict(k=[32], seeds=[b"1101"]),
    "neither list": dict(),
    "mask with another character": dict(seeds=[b"11a1"]),
    "mask without a 1": dict(seeds=[b"0000"]),
    "empty mask": dict(seeds=[b"1101", b""]),
    "null mask": dict(seeds=[None]),
    "mask too long": dict(seeds=[b"1" * 601]),
    "too many masks": dict(seeds=[b"101"] * 33),
    "too many k": dict(k=[20] * 33),
    "k = 0": dict(k=[32, 0]),
    "k too large": dict(k=[601]),
    "n_bits too small": dict(k=[32], n_bits=3),
    "n_bits too large": dict(k=[32], n_bits=25),
    "n_bits too large, seeds": dict(seeds=[b"1101"], n_bits=25, flags=REV),
}


@pytest.mark.parametrize("name", sorted(BAD_CONFIGS))
def test_create_ex_argument_errors(name):
    rc, msg = create_ex(**BAD_CONFIGS[name])
    assert rc == ERR_ARG, (name, rc, msg)
    assert msg.startswith("ntc_hll_create_ex: ") and len(msg) > len("ntc_hll_create_ex: "), (name, msg)


def test_create_ex_null_arguments():
    L = _abi.lib()
    h = C.c_void_p()
    assert L.ntc_hll_create_ex(None, C.byref(h)) == ERR_ARG
    cfg = _abi.NtcHllConfig()
    assert L.ntc_hll_create_ex(C.byref(cfg), None) == ERR_ARG


def test_python_constructors_check_the_strand_first():
    import ntcard_amd as nt
    with pytest.raises(ValueError):
        nt.HllEngine([32], strand="both")
    with pytest.raises(ValueError):
        nt.HllEngine.from_seeds(["1101"], strand="sideways")
    with pytest.raises(nt.NtcError) as ei:
        nt.HllEngine.from_seeds(["1121"])
    assert ei.value.code == ERR_ARG


# ---- the command line ----
@pytest.mark.parametrize("args,needle", [
    (["--strand=sideways", "-k", "32", "reads.fq"], b"--strand"),
    (["--seed=1101", "-k", "20", "reads.fq"], b"--seed cannot be combined with -k"),
    (["-k", "20", "--seed=1101", "reads.fq"], b"--seed cannot be combined with -k"),
    (["--seed=11a1", "reads.fq"], b"--seed"),
    (["--seed=1101,000", "reads.fq"], b"--seed"),
    (["--seed=1101,", "reads.fq"], b"--seed"),
])
def test_cli_argument_errors(args, needle, tmp_path):
    r = run_cli(NTHLL, args, cwd=tmp_path, timeout=60)  # (reads.fq does not exist: never opened)
    assert r.returncode == 1 and r.stdout == b"", (args, r.stdout, r.stderr)
    assert r.stderr.startswith(b"nthll: ") and needle in r.stderr, (args, r.stderr)
