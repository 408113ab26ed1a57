"""GPU tests of ntcard engines on forged k-mers (tests/hash_forge.py, tests/forged_cases.py): ntComp's two sample patterns at every sBits class up to 24,
where no random read of a feasible test is ever sampled — hits of both samples, the bit under the pattern both ways, the lowest and the highest counter
index, near misses by the first and by the last pattern bit, K1's superset case (one strand 0^s 1.., the other 0^(s+1)..) and both strands matching —
on the general kernel K1 (plain, one strand, spaced seed, signatures) and on the tiled pair K1h + K1f up to its packing limit
r_bits + 1 + (s_bits - 7) == 32.  t_Counter, F1 and the value histograms must equal tests/strand_model.py exactly (signatures: the values and their counts
too); tests/test_hash_forge_host.py pins every family to the oracle and shows that every hit has a counter of its own with a count of its own."""
import numpy as np
import pytest

import forged_cases as fc
import strand_model as sm
from gpu_support import dev, nt  # noqa: F401
from support import assert_same_sketch, to_slots

pytestmark = pytest.mark.gpu


def engine(nt, fam, flags=0, **kw):
    if "0" in fam.mask:
        return nt.Engine.from_seeds([fam.mask], r_bits=fam.r_bits, s_bits=fam.s_bits, flags=flags, strand=fc.NAMES[fam.strand], **kw)
    return nt.Engine([fam.k], r_bits=fam.r_bits, s_bits=fam.s_bits, flags=flags, strand=fc.NAMES[fam.strand], **kw)


def by_reads(e, reads):
    e.submit_reads(reads)


def by_slots(e, reads):
    L = len(reads[0])
    stride = (L + 3) // 4 * 4
    d = dev(to_slots(reads, stride))
    e.submit_device(d.data_ptr(), len(reads), L, stride)
    e.sync()  # (d is released behind this call)


def check(nt, fam, reads, submit, what, flags=0, **kw):
    want = fc.model_sketch(reads, fam.mask, fam.strand, fam.r_bits, fam.s_bits)
    assert want[0].any() and int(want[1][0]) == len(reads)
    with engine(nt, fam, flags, **kw) as e:
        submit(e, reads)
        got = e.finish(counters=True)
    assert_same_sketch(got, want, f"{fam.name} {what}", nonempty=True, hist_r_bits=fam.r_bits)


# ---- 1. the general kernel K1 ----
@pytest.mark.parametrize("k,s_bits", fc.K1_FAMILIES, ids=[f"k{k}_s{s}" for k, s in fc.K1_FAMILIES])
def test_k1_plain(nt, k, s_bits):
    fam = fc.family(k, s_bits)
    reads = fc.family_reads(fam)
    check(nt, fam, reads, by_slots, "submit_device")
    check(nt, fam, reads, by_reads, "submit_reads")
    check(nt, fam, reads, by_slots, "submit_device, direct atomics", nt.FLAG_DIRECT_ATOMICS)
    check(nt, fam, reads, by_reads, "submit_reads, direct atomics", nt.FLAG_DIRECT_ATOMICS)


@pytest.mark.parametrize("s_bits", fc.S_BITS)
def test_k1_one_strand(nt, s_bits):
    """the forward and the reverse engine over the same reads: the k-mers forged for either strand"""
    fams = [fc.family(96, s_bits, strand=st) for st in (sm.FORWARD, sm.REVERSE)]
    reads = fc.family_reads(fams[0]) + fc.family_reads(fams[1])
    for fam in fams:
        check(nt, fam, reads, by_slots, "submit_device")
        check(nt, fam, reads, by_reads, "submit_reads")


@pytest.mark.parametrize("s_bits", fc.S_BITS)
def test_k1_spaced_seed(nt, s_bits):
    fam = fc.family(96, s_bits, mask=fc.SPACED96)
    reads = fc.family_reads(fam)
    check(nt, fam, reads, by_slots, "submit_device")
    check(nt, fam, reads, by_reads, "submit_reads")


@pytest.mark.parametrize("s_bits", [16, 24])
def test_signature_engine(nt, s_bits):
    fam = fc.family(96, s_bits)
    reads = fc.family_reads(fam)
    want = fc.model_sketch(reads, fam.mask, fam.strand, fam.r_bits, fam.s_bits)
    hashes, counts = fc.model_signature(reads, fam.mask, fam.strand, s_bits)
    assert hashes.size == sum(1 for e in fam.entries if e.sample is not None) and sorted(counts.tolist()) == list(range(1, hashes.size + 1))
    with engine(nt, fam, signature=True) as e:
        e.submit_reads(reads)
        got = e.finish(counters=True)
        h, c = e.signature(0)
    assert_same_sketch(got, want, f"{fam.name} signature", nonempty=True, hist_r_bits=fam.r_bits)
    assert np.array_equal(h, hashes) and np.array_equal(c, counts)


# ---- 2. the tiled kernels K1h + K1f ----
def by_tiles(nt):
    def submit(e, reads):
        d = dev(nt.tile_reads(reads, len(reads[0])))
        e.submit_tiled_device(d.data_ptr(), len(reads), len(reads[0]))
        e.sync()
    return submit


def tiled_reads(fam):
    """(the windows clean, the windows directly beside an N: in front of one half, behind the other)"""
    clean = fc.family_reads(fam)
    dirty = [b"N" + r if j % 2 else r + b"N" for j, r in enumerate(clean)]
    return clean, dirty


@pytest.mark.parametrize("k,s_bits,r_bits", fc.TILED_FAMILIES, ids=[f"k{k}_s{s}r{r}" for k, s, r in fc.TILED_FAMILIES])
def test_tiled(nt, k, s_bits, r_bits):
    """K1h samples the clean windows; a window beside an N is K1f's to re-derive.  (14, 24) and (20, 18) fill K1h's table word to its last bit"""
    fam = fc.family(k, s_bits, r_bits)
    clean, dirty = tiled_reads(fam)
    check(nt, fam, clean, by_tiles(nt), "tiled, clean", nt.FLAG_REQUIRE_TILED)
    check(nt, fam, dirty, by_tiles(nt), "tiled, beside an N", nt.FLAG_REQUIRE_TILED)


@pytest.mark.parametrize("strand", [sm.FORWARD, sm.REVERSE], ids=["forward", "reverse"])
def test_tiled_one_strand(nt, strand):
    fam = fc.family(32, 16, strand=strand)
    clean, dirty = tiled_reads(fam)
    check(nt, fam, clean, by_tiles(nt), "tiled, clean", nt.FLAG_REQUIRE_TILED, strand_tiled=True)
    check(nt, fam, dirty, by_tiles(nt), "tiled, beside an N", nt.FLAG_REQUIRE_TILED, strand_tiled=True)
