"""The one-strand K1h kernels on the CPU: the GENERATED instruction list of gen_k1h.Gen(..., strand=1 | 2) runs on the wave emulator and, together with a
Python model of what K1f does for a strand launch (tests/k1h_strand_model.py), must reproduce strand_model.model_sketch — the oracle's fh / rh pushed through
ntComp — exactly.  Also here: strand=0 renders the canonical kernels unchanged, the budgets of every strand variant the library is built with, and the
argument checks of NTC_FLAG_STRAND_TILED, which come before a device is looked for."""
import ctypes as C
import re

import pytest

import k1h_strand_model as ksm
import k1h_variant_cases as vc
import strand_model as sm
from ntcard_amd import _abi
from support import abi_config

gen_k1h = ksm.gen_k1h
BOTH = pytest.mark.parametrize("strand", [sm.FORWARD, sm.REVERSE], ids=["forward", "reverse"])
ERR_ARG = -1
FWD, REV, STRAND_TILED = 512, 1024, 4096


@BOTH
@pytest.mark.parametrize("n,L,k,p_bad,n_waves", [
    (2048, 40, 32, 0.0, 2),       # one tile shared by two waves (the second one fills its window with two masked blocks)
    (4097, 47, 32, 0.02, 3),      # a partial last tile of one read
    (2100, 64, 25, 0.01, 2), (2049, 33, 20, 0.0, 2), (2500, 20, 12, 0.02, 2),  # other k: window start chunk, phase, table groups
    (2048, 160, 32, 0.001, 2),    # a virtual chunk behind the read (blocks = chunks + 1)
])
def test_strand_k1h_emulated_matches_model(strand, n, L, k, p_bad, n_waves):
    res = ksm.run(strand, n, L, k, p_bad, n_waves=n_waves)
    assert not res["sus_overflow"]
    if p_bad:
        assert len(res["sus"]) > 0


@BOTH
@pytest.mark.parametrize("s_bits", [8, 11])
def test_strand_k1h_emulated_larger_s_bits(strand, s_bits):
    """sBits >= 8: the walk tests the 8-bit prefixes 0x7f / 0x00 of the strand's top bits, the resolve pass the rest"""
    ksm.run(strand, 3000, 150, 32, 0.002, s_bits=s_bits, r_bits=12)


@BOTH
@pytest.mark.parametrize("k,gap,L", [(12, 2, 40), (32, 8, 100)])
def test_strand_k1h_emulated_spaced_seeds(strand, k, gap, L):
    ksm.run(strand, 3000, L, k, 0.004, gap=gap, r_bits=12)


@BOTH
@pytest.mark.parametrize("n,C,k,p_bad", [(2100, 4, 25, 0.01), (2300, 1, 12, 0.0)])
def test_strand_k1h_emulated_ragged_batches(strand, n, C, k, p_bad):
    ksm.run_ragged(strand, n, C, k, p_bad, seed=n + C)


@BOTH
def test_strand_k1h_emulated_suspect_overflow(strand):
    res = ksm.run(strand, 4097, 47, 32, 0.02, n_waves=3, sus_cap=16)
    assert res["sus_overflow"]    # K1f's slow path (the model's): every window of a dirty-affected block from the bytes, the strand's own value


@BOTH
def test_strand_k1h_emulated_direct_atomics(strand):
    res = ksm.run(strand, 2048, 80, 32, use_log=False)
    assert res["sketch"].any() and res["sk_dirty"] == 1 and res["keys"].size == 0


@BOTH
@pytest.mark.parametrize("k", [13, 17, 29])
def test_strand_k1h_emulated_odd_k(strand, k):
    """phases (k - 1) mod 16 the cases above do not touch, and the parity of the bit that wraps around in a walk step"""
    ksm.run(strand, 2100, k + 29, k, 0.01, seed=k)


@pytest.mark.parametrize("c", [c for c in vc.EMU_CASES + vc.PLANT_CASES if c.strand != sm.CANONICAL], ids=vc.case_id)
def test_strand_k1h_emulated_every_body(c):
    """every one-strand body the library is built with, both sBits classes (the case table of tests/k1h_variant_cases.py; tests/test_k1h_variant_cases_host.py
    proves the coverage): what depends on k — start chunk, phase, table groups, the wrap bit's parity in the reverse walk — at each k it belongs to; and the planted windows of sBits 24 at r_bits 14 (17 extra hash bits in the table word)"""
    arr = vc.reads_of(c)
    res = ksm.check(c.strand, [arr[i].tobytes() for i in range(c.n)], arr, c.n, c.L, c.k, c.r_bits, c.s_bits, c.gap, 2)
    assert len(res["sus"]) > 0 and not res["sus_overflow"]
    if c.kind == "plant":  # the windows planted beside an N are suspects: K1f's verdict on the extra hash bits decides them
        sus = {(int(t) * 2048 + (int(rw) & 2047), int(rw) >> 11) for _, t, rw, _ in res["sus"]}
        beside = [(r, w) for r, w, _, what in vc.planted_reads(c)[1] if what in ("n_before", "n_behind")]
        assert len(beside) == 12 and all(p in sus for p in beside)


@pytest.mark.parametrize("k,sb,gap", [(32, 7, 0), (12, 8, 2), (21, 8, 0)])
def test_strand_zero_is_the_canonical_generator(k, sb, gap):
    a = gen_k1h.Gen(k, sb, gap).build().render(label_fmt=".L{}")
    b = gen_k1h.Gen(k, sb, gap, strand=0).build().render(label_fmt=".L{}")
    assert a == b
    one = gen_k1h.Gen(k, sb, gap, strand=1).build()
    assert one.n_insts() < gen_k1h.Gen(k, sb, gap).build().n_insts()


def test_strand_variants_budgets():
    """every one-strand variant the library is built with: (k, gap) of VARIANTS x forward, reverse x both sBits classes; the register map is the canonical
    kernels' (checked there), the table is the unchanged [2 strands][groups][64] one, and a strand walk is shorter than the canonical one"""
    assert set(gen_k1h.STRAND_VARIANTS) == {(k, g, st) for k, g in gen_k1h.VARIANTS for st in (1, 2)}
    assert len(gen_k1h.STRAND_VARIANTS) == len(set(gen_k1h.STRAND_VARIANTS))
    assert {gen_k1h.strand_part(k, st) for k, _g, st in gen_k1h.STRAND_VARIANTS} == set(range(gen_k1h.STRAND_PARTS))
    gen_k1h.check_register_map()
    assert gen_k1h.S_END <= 100
    canonical = {(k, gap, sb): gen_k1h.Gen(k, sb, gap).build().n_insts() for k, gap in gen_k1h.VARIANTS for sb in (7, 8)}
    for k, gap, st in gen_k1h.STRAND_VARIANTS:
        assert gen_k1h.TABLE_OFF + gen_k1h.table_bytes(k) <= gen_k1h.LDS_BYTES
        for sb in (7, 8):
            prog = gen_k1h.Gen(k, sb, gap, strand=st).build()
            assert 2000 < prog.n_insts() < canonical[k, gap, sb]
            regs = set()
            for ins in prog.render(label_fmt=".L{}"):
                regs.update(int(x) for x in re.findall(r"\bv(\d+)\b", ins))
                for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", ins):  # register tuples: loads, 64-bit items, the suspect entry
                    regs.update(range(int(lo), int(hi) + 1))
            assert max(regs) <= 254
            other = range(gen_k1h.V_R, gen_k1h.V_R + 31) if st == 1 else range(gen_k1h.V_F, gen_k1h.V_F + 31)
            assert not regs & set(other), "the other strand's state planes are never touched"


# ---- ABI: NTC_FLAG_STRAND_TILED is valid only beside exactly one strand flag; checked before a device is looked for ----
def test_header_library_and_package_carry_the_flag():
    import os
    import ntcard_amd as nt
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntcard_hip.h")
    text = open(header).read()
    assert re.search(r"#define\s+NTC_FLAG_STRAND_TILED\s+4096u", text) and re.search(r"#define\s+NTC_ABI_VERSION\s+6\b", text)
    assert nt.FLAG_STRAND_TILED == STRAND_TILED and _abi.lib().ntc_abi_version() == 6


@pytest.mark.parametrize("flags", [STRAND_TILED, STRAND_TILED | FWD | REV, STRAND_TILED | 64])
@pytest.mark.parametrize("seeded", [False, True])
def test_strand_tiled_needs_exactly_one_strand_flag(flags, seeded):
    L = _abi.lib()
    h = C.c_void_p()
    if seeded:
        c = _abi.NtcConfig(r_bits=20, s_bits=7, device=0, flags=flags)
        arr = (C.c_char_p * 1)(b"1" * 32)
        rc = L.ntc_create_seeded(C.byref(c), 1, arr, C.byref(h))
    else:
        rc = L.ntc_create(C.byref(abi_config(r_bits=20, flags=flags)), C.byref(h))
    assert rc == ERR_ARG and not h.value
    assert b"device" not in L.ntc_last_error() and b"STRAND" in L.ntc_last_error()


def test_nthll_engines_refuse_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    arr = (C.c_uint32 * 1)(32)
    c = _abi.NtcHllConfig(n_bits=12, device=0, flags=FWD | STRAND_TILED)
    c.n_k = 1
    c.k = C.cast(arr, C.POINTER(C.c_uint32))
    assert L.ntc_hll_create_ex(C.byref(c), C.byref(h)) == ERR_ARG and not h.value
    assert b"unknown flag" in L.ntc_last_error()


def test_python_strand_tiled_keyword():
    import ntcard_amd as nt
    with pytest.raises(ValueError, match="strand_tiled"):
        nt.Engine([32], strand_tiled=True)                       # no strand to count
    with pytest.raises(ValueError, match="strand_tiled"):
        nt.Engine([32], strand="canonical", strand_tiled=True)
