"""Host tests of signatures (include/ntcard_hip.h: NTC_FLAG_SIGNATURE): the flag's validation before a device is looked for, ntc_signature_compare against
np.intersect1d, the signature file's write / read round trip, bin/ntsig, and the model of tests/sig_model.py against the real reference's hashes."""
import ctypes as C

import numpy as np
import pytest

import orc
import sig_model
import strand_model as sm
from ntcard_amd import _abi
import ntcard_amd as nt
from support import NTSIG, abi_config, created, run_cli, sampled

ERR_ARG = -1
SIG, FWD, REV, STRAND_TILED, HPC = 16384, 512, 1024, 4096, 8192


# ---- the flag ----
def test_the_constant():
    assert nt.FLAG_SIGNATURE == SIG
    assert all(s in _abi.ABI_SYMBOLS for s in ("ntc_signature", "ntc_signature_size", "ntc_signature_inject", "ntc_signature_inject_device",
                                               "ntc_signature_compare", "ntc_signature_stats", "ntc_signature_time"))


@pytest.mark.parametrize("beside", [0, 2, 8, 16, 32, 128, FWD, REV, FWD | STRAND_TILED, HPC, 64])
def test_create_takes_the_flag_beside_every_compatible_one(beside):
    L = _abi.lib()
    h = C.c_void_p()
    assert created(L.ntc_create(C.byref(abi_config(flags=SIG | beside)), C.byref(h)), h, L)


def test_create_seeded_takes_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    c = _abi.NtcConfig(n_k=0, k=None, gap=0, r_bits=14, s_bits=7, device=0, flags=SIG)
    seeds = (C.c_char_p * 1)(b"1110111")
    assert created(L.ntc_create_seeded(C.byref(c), 1, seeds, C.byref(h)), h, L)


def test_the_simple_kernel_is_refused_beside_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    assert L.ntc_create(C.byref(abi_config(flags=SIG | 1)), C.byref(h)) == ERR_ARG and not h
    assert b"NTC_FLAG_SIGNATURE" in L.ntc_last_error()
    c = _abi.NtcConfig(n_k=0, k=None, gap=0, r_bits=14, s_bits=7, device=0, flags=SIG | 1)
    seeds = (C.c_char_p * 1)(b"1111111")
    assert L.ntc_create_seeded(C.byref(c), 1, seeds, C.byref(h)) == ERR_ARG and not h


def test_the_retired_bits_stay_refused_beside_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    for bit in (4, 256, 2048, 1 << 20):
        assert L.ntc_create(C.byref(abi_config(flags=SIG | bit)), C.byref(h)) == ERR_ARG and b"unknown flag" in L.ntc_last_error()
    assert L.ntc_create(C.byref(abi_config(flags=SIG | FWD | REV)), C.byref(h)) == ERR_ARG
    assert L.ntc_create(C.byref(abi_config(flags=SIG | STRAND_TILED)), C.byref(h)) == ERR_ARG


@pytest.mark.parametrize("flags", [SIG, SIG | FWD, SIG | HPC])
def test_hll_create_refuses_the_flag(flags):
    L = _abi.lib()
    k = (C.c_uint32 * 1)(32)
    c = _abi.NtcHllConfig()
    c.n_k, c.k, c.n_bits, c.device, c.flags = 1, C.cast(k, C.POINTER(C.c_uint32)), 12, 0, flags
    h = C.c_void_p()
    assert L.ntc_hll_create_ex(C.byref(c), C.byref(h)) == ERR_ARG and not h
    assert b"unknown flag" in L.ntc_last_error()


def test_python_keyword_sets_the_bit(monkeypatch):
    seen = []
    L = _abi.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name in ("ntc_create", "ntc_create_seeded"):
                def wrapped(cfg_ref, *rest):
                    seen.append(cfg_ref._obj.flags)
                    return ERR_ARG
                return wrapped
            return fn

    monkeypatch.setattr(_abi, "lib", lambda: Spy())
    for make in (lambda: nt.Engine([32], signature=True), lambda: nt.Engine.from_seeds(["1101"], signature=True, hpc=True),
                 lambda: nt.Engine([32], strand="forward")):
        with pytest.raises(nt.NtcError):
            make()
    assert seen == [SIG, SIG | HPC, FWD]


# ---- ntc_signature_compare ----
def u64(x):
    return np.array(x, dtype=np.uint64)


RNG = np.random.default_rng(5)
POOL = np.unique(RNG.integers(1, 1 << 63, size=4000, dtype=np.uint64) * np.uint64(2) + np.uint64(1))
COMPARE_CASES = {
    "empty_empty": (u64([]), u64([])),
    "empty_some": (u64([]), POOL[:10]),
    "some_empty": (POOL[:10], u64([])),
    "disjoint": (POOL[0:200:2], POOL[1:200:2]),
    "identical": (POOL[:777], POOL[:777]),
    "interleaved": (POOL[::2], np.union1d(POOL[::3], POOL[1::7])),
    "one_at_the_low_end": (POOL[:1], POOL[:500]),
    "one_at_the_high_end": (POOL[:500], POOL[499:500]),
    "one_past_the_high_end": (POOL[:500], POOL[500:501]),
    "extremes": (u64([1, 2**64 - 1]), u64([1, 5, 2**64 - 1])),
}


@pytest.mark.parametrize("name", sorted(COMPARE_CASES))
def test_compare_matches_intersect1d(name):
    a, b = COMPARE_CASES[name]
    want = np.intersect1d(a, b).size
    if name in ("disjoint", "empty_some", "one_past_the_high_end"):
        assert want == 0
    if name in ("identical", "interleaved", "one_at_the_low_end", "one_at_the_high_end", "extremes"):
        assert want > 0
    common, jac, cab, cba = nt.signature_compare(a, b)
    assert common == want
    union = a.size + b.size - want
    assert jac == (want / union if union else 0.0)
    assert cab == (want / a.size if a.size else 0.0) and cba == (want / b.size if b.size else 0.0)
    assert nt.signature_compare(b, a)[0] == want


@pytest.mark.parametrize("bad", [u64([3, 2, 5]), u64([2, 2, 5]), u64([1, 2, 5, 5]), u64([9, 1])])
def test_compare_refuses_unsorted_and_duplicated_input(bad):
    good = u64([1, 2, 3])
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(nt.NtcError) as ei:
            nt.signature_compare(a, b)
        assert ei.value.code == ERR_ARG and "ascending" in str(ei.value)


def test_compare_null_arguments():
    L = _abi.lib()
    n = C.c_uint64()
    a = u64([1, 2])
    assert L.ntc_signature_compare(None, 2, a.ctypes.data_as(C.c_void_p), 2, C.byref(n)) == ERR_ARG
    assert L.ntc_signature_compare(a.ctypes.data_as(C.c_void_p), 2, a.ctypes.data_as(C.c_void_p), 2, None) == ERR_ARG
    assert L.ntc_signature_compare(None, 0, None, 0, C.byref(n)) == 0 and n.value == 0


# ---- files ----
HEADER = dict(k=25, gap=0, strand=1, hpc=1, s_bits=7, mask="1111111101111111100111111")


def test_file_round_trip(tmp_path):
    h = POOL[:1000]
    c = RNG.integers(1, 2**32, size=h.size, dtype=np.uint64).astype(np.uint32)
    c[0], c[-1] = 2**32 - 1, 1
    p = tmp_path / "a.sig"
    nt.signature_write(p, HEADER, h, c)
    raw = p.read_bytes()
    assert raw[:8] == b"NTCSIG1\0" and len(raw) == 8 + 24 + 8 + 32 + 12 * h.size  # magic, six uint32, n, the mask padded to 8, the pairs
    assert raw[8 + 24 + 8 + 32:][:8] == int(h[0]).to_bytes(8, "little")
    got, gh, gc = nt.signature_read(p)
    assert got == dict(HEADER, n=h.size) and np.array_equal(gh, h) and np.array_equal(gc, c)
    nt.signature_write(p, dict(HEADER, mask="1" * 32, k=32), u64([]), np.zeros(0, np.uint32))
    got, gh, gc = nt.signature_read(p)
    assert got["n"] == 0 and gh.size == 0 and gc.size == 0 and got["mask"] == "1" * 32


def test_file_errors(tmp_path):
    p = tmp_path / "a.sig"
    for bad in (dict(HEADER, k=24), dict(HEADER, mask="1" * 24 + "2"), dict(HEADER, strand=3), dict(HEADER, s_bits=1)):
        with pytest.raises(nt.NtcError):
            nt.signature_write(p, bad, u64([1]), np.ones(1, np.uint32))
    with pytest.raises(nt.NtcError):
        nt.signature_write(p, HEADER, u64([2, 1]), np.ones(2, np.uint32))
    nt.signature_write(p, HEADER, u64([1, 2, 3]), np.ones(3, np.uint32))
    raw = p.read_bytes()
    (tmp_path / "cut.sig").write_bytes(raw[:-3])
    (tmp_path / "magic.sig").write_bytes(b"NTCSIG2\0" + raw[8:])
    for name in ("cut.sig", "magic.sig", "absent.sig"):
        with pytest.raises(nt.NtcError):
            nt.signature_read(tmp_path / name)
    # a pair count the file's length does not bear out is refused before anything is sized or sought by it
    lying = bytearray(raw)
    lying[32:40] = (2**61).to_bytes(8, "little")
    (tmp_path / "lying.sig").write_bytes(bytes(lying))
    L = _abi.lib()
    hd = _abi.NtcSigHeader()
    cnt = np.zeros(4, np.uint32)
    assert L.ntc_signature_read(str(tmp_path / "lying.sig").encode(), C.byref(hd), None, cnt.ctypes.data_as(C.c_void_p), 2**62) == ERR_ARG
    assert L.ntc_signature_read(str(tmp_path / "lying.sig").encode(), C.byref(hd), None, None, 0) == ERR_ARG
    assert L.ntc_signature_read(str(tmp_path / "a.sig").encode(), C.byref(hd), None, cnt.ctypes.data_as(C.c_void_p), 4) == 0 and cnt.tolist() == [1, 1, 1, 0]
    (tmp_path / "long.sig").write_bytes(raw + b"\0" * 12)
    with pytest.raises(nt.NtcError):
        nt.signature_read(tmp_path / "long.sig")


def ntsig(*args):
    return run_cli(NTSIG, args, timeout=60)


def test_ntsig_info_and_compare(tmp_path):
    a, b = POOL[:600], POOL[300:1000]
    nt.signature_write(tmp_path / "a.sig", HEADER, a, np.ones(a.size, np.uint32))
    nt.signature_write(tmp_path / "b.sig", HEADER, b, np.ones(b.size, np.uint32))
    r = ntsig("info", tmp_path / "a.sig")
    assert r.returncode == 0, r.stderr
    fields = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert fields["k"] == "25" and fields["mask"] == HEADER["mask"] and fields["strand"] == "forward" and fields["hpc"] == "1" and fields["sBits"] == "7" and fields["n"] == "600"
    r = ntsig("compare", tmp_path / "a.sig", tmp_path / "b.sig")
    assert r.returncode == 0, r.stderr
    fields = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert fields["common"] == "300" and fields["n_a"] == "600" and fields["n_b"] == "700"
    assert fields["jaccard"] == "%.6f" % (300 / 1000) and fields["containment_a_in_b"] == "%.6f" % 0.5 and fields["containment_b_in_a"] == "%.6f" % (300 / 700)
    r = ntsig("compare", tmp_path / "a.sig", tmp_path / "a.sig")
    assert r.returncode == 0 and b"jaccard\t1.000000" in r.stdout


@pytest.mark.parametrize("field,other", [("sBits", dict(HEADER, s_bits=11)), ("mask", dict(HEADER, mask="1" * 25)), ("strand", dict(HEADER, strand=0)),
                                         ("hpc", dict(HEADER, hpc=0)), ("k", dict(HEADER, k=24, mask=HEADER["mask"][:24])), ("gap", dict(HEADER, gap=2))])
def test_ntsig_refuses_files_counted_differently(tmp_path, field, other):
    nt.signature_write(tmp_path / "a.sig", HEADER, POOL[:10], np.ones(10, np.uint32))
    nt.signature_write(tmp_path / "b.sig", other, POOL[:10], np.ones(10, np.uint32))
    r = ntsig("compare", tmp_path / "a.sig", tmp_path / "b.sig")
    assert r.returncode != 0 and r.stdout == b""
    assert ("(%s differs)" % field).encode() in r.stderr


def test_ntsig_usage_and_bad_files(tmp_path):
    assert ntsig().returncode != 0 and ntsig("compare", "x").returncode != 0
    (tmp_path / "junk.sig").write_bytes(b"not a signature")
    r = ntsig("info", tmp_path / "junk.sig")
    assert r.returncode != 0 and b"not a signature file" in r.stderr


# ---- the model ----
def test_sampled_is_ntcomp():
    s = 7
    yes0, yes1 = np.uint64(1 << 56), np.uint64(63 << 57)  # s = 7: the top bits 0000 0001 and 0111 111
    h = u64([int(yes0), int(yes0) | 12345, int(yes1), int(yes1) | 99, 0, 1, 2**64 - 1, int(yes0) << 1, int(yes0) >> 1])
    assert sampled(h, s).tolist() == [True, True, True, True, False, False, False, False, False]
    # against ntComp as the oracle runs it: a value is sampled iff it lands in t_Counter
    v = sig_model.values(list(sig_model.equal_reads())[:40], 32)
    tc, f1 = sm.sketch_of([(v, v)], sm.FORWARD, 14, s)
    assert int(tc.sum()) == int(sampled(v, s).sum()) > 0 and f1[0] == v.size


def test_the_tables_of_the_issue():
    """the generator's figures the GPU tests rely on (a changed generator cannot empty a test)"""
    assert sum(orc.hash_read(r, 32)[0].size for r in sig_model.equal_reads()) == 36451
    for k, s, total, distinct, top in ((32, 7, 593, 593, 1), (32, 2, 18636, 18636, 1), (12, 2, 22622, 22482, 3)):
        h, c = sig_model.equal_model(k, "canonical", s)
        assert (int(c.sum()), h.size, int(c.max())) == (total, distinct, top)
        assert np.all(h[1:] > h[:-1]) and h[0] != 0


def test_plain_and_mask_paths_of_the_model_agree():
    reads = list(sig_model.equal_reads())[:30]
    a = sig_model.values(reads, 32)
    (fs, rs), = sm.values_of(reads, ["1" * 32])
    assert np.array_equal(a, np.minimum(fs, rs)) and a.size > 0


@pytest.mark.skipif(not orc.have_ref(), reason="the reference's hash tool is built only where its sources are")
def test_model_values_are_the_references():
    reads = [r for r in sig_model.equal_reads()][:60]
    rows = orc.ref_hash(reads, 32)
    ref = np.concatenate([np.asarray(h, dtype=np.uint64).reshape(-1) for _, h in rows])
    assert np.array_equal(np.sort(ref), np.sort(sig_model.values(reads, 32))) and ref.size > 5000
