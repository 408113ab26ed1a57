"""CPU tests of one-strand counting (include/ntcard_hip.h: NTC_FLAG_STRAND_FORWARD / _REVERSE, ntc_hash_dump_strand_device; `ntcard --strand`):
the model the GPU tests compare against (tests/strand_model.py) is anchored to what is already pinned against the reference, its inputs
tell the three strands apart, and every malformed argument is refused before a device is looked for."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import orc
import strand_model as sm
from ntcard_amd import _abi
from support import ALPHA, NTCARD, ROOT, abi_config, gap_mask, random_reads, run_cli
HEADER = os.path.join(ROOT, "include", "ntcard_hip.h")
ERR_ARG = -1
FWD, REV = 512, 1024


# ---- the model ----
@pytest.mark.parametrize("k", [1, 5, 12, 31, 32, 33, 64, 97])
def test_min_of_the_two_strands_is_the_pinned_canonical_hash(k):
    rng = random.Random(k)
    for _ in range(12):
        seq = sm.rseq(rng, rng.choice([max(1, k - 1), k, k + 7, 150]), pn=rng.choice([0.0, 0.02]))
        fs, rs, pos = sm.window_values(seq, "1" * k)
        oh, opos = orc.hash_read(seq, k)
        assert np.array_equal(pos, opos) and np.array_equal(np.minimum(fs, rs), oh), (k, seq)


@pytest.mark.parametrize("k", [2, 12, 31, 32, 33, 64])
def test_min_of_the_two_strands_is_the_pinned_spaced_seed_hash(k):
    L = orc.lib()
    rng = random.Random(100 + k)
    for mask in sm.masks_for(k):  # (asymmetric masks included)
        if "0" not in mask:
            continue
        dc = np.array([i for i, c in enumerate(mask) if c == "0"], dtype=np.uint32)
        for _ in range(4):
            seq = sm.rseq(rng, rng.choice([k, k + 7, 150]), pn=rng.choice([0.0, 0.02]))
            fs, rs, pos = sm.window_values(seq, mask)
            cap = max(len(seq), 1)
            h = np.zeros(cap, dtype=np.uint64)
            p = np.zeros(cap, dtype=np.uint32)
            n = L.orc_sthash_read(seq, len(seq), k, orc._ptr(dc), len(dc), orc._ptr(h), orc._ptr(p), cap)
            assert n == len(pos) and np.array_equal(pos, p[:n]) and np.array_equal(np.minimum(fs, rs), h[:n]), (mask, seq)


@pytest.mark.parametrize("k", [1, 2, 12, 31, 33, 64, 200])
def test_forward_and_reverse_are_the_closed_forms(k):
    """fh: the FIRST base rotated k-1 times (which of the two is "forward"); rh likewise from the complement; rh(w) == fh(revcomp(w))"""
    L = orc.lib()
    rng = random.Random(200 + k)
    for _ in range(8):
        w = sm.rseq(rng, k)
        fh, rh, bad = C.c_uint64(), C.c_uint64(), C.c_uint()
        assert L.orc_window_hash(w, k, C.byref(fh), C.byref(rh), C.byref(bad)) == 1
        f = r = 0
        for i in range(k):
            f ^= L.orc_srol(L.orc_seed(w[i]), k - 1 - i)
            r ^= L.orc_srol(L.orc_seed_comp(w[i]), i)
        assert fh.value == f and rh.value == r
        wc = sm.revcomp(w)
        fc, rc = C.c_uint64(), C.c_uint64()
        assert L.orc_window_hash(wc, k, C.byref(fc), C.byref(rc), C.byref(bad)) == 1
        assert rh.value == fc.value and fh.value == rc.value
    if k > 1:  # the two are different functions: a window that is not its own reverse complement
        w = b"A" * (k - 1) + b"C"
        assert sm.strand_hash(w, "1" * k, sm.FORWARD)[0] != sm.strand_hash(w, "1" * k, sm.REVERSE)[0]


@pytest.mark.parametrize("name,masks,gap,s_bits", sm.SKETCH_CONFIGS, ids=[c[0] for c in sm.SKETCH_CONFIGS])
def test_the_gpu_tests_inputs_tell_the_strands_apart(name, masks, gap, s_bits):
    """a kernel that ignores the flag, or swaps the strands, cannot pass tests/test_strand_gpu.py on these inputs"""
    for reads in (sm.sketch_reads_equal(), sm.sketch_reads_ragged()):
        vals = sm.values_of(reads, masks)
        sk = {s: sm.sketch_of(vals, s, sm.R_BITS, s_bits) for s in (sm.CANONICAL, sm.FORWARD, sm.REVERSE)}
        assert np.array_equal(sk[sm.FORWARD][1], sk[sm.CANONICAL][1]) and np.array_equal(sk[sm.REVERSE][1], sk[sm.CANONICAL][1])  # F1
        for mi in range(len(masks)):
            for s in sk:
                assert sk[s][0][mi, 0].any() and sk[s][0][mi, 1].any(), (name, mi, s)
            for a, b in ((sm.CANONICAL, sm.FORWARD), (sm.CANONICAL, sm.REVERSE), (sm.FORWARD, sm.REVERSE)):
                assert not np.array_equal(sk[a][0][mi], sk[b][0][mi]), (name, mi, a, b)


@pytest.mark.parametrize("k", list(range(12, 33)))
def test_array_form_is_window_values_window_by_window(k):
    """strand_model.window_blocks (table look-ups over arr[n, L]) against window_values (one oracle call per window): which windows exist, and fs and rs
    of each, for plain k and both -g masks; reads with lower case, U / u, N and every other byte of support.ALPHA, and the reference's table-slot bytes"""
    rng = np.random.default_rng(k)
    masks = ["1" * k] + [gap_mask(kk, g) for kk, g in ((12, 2), (32, 8)) if kk == k]
    other = np.concatenate([ALPHA[10:], np.array([0, 1, 3, 4, 5, 7, 255], dtype=np.uint8)])  # NnRYKM.-* and bytes that are no letters
    for mask in masks:
        for L, p_bad in ((k, 0.02), (k + 1, 0.0), (k + 29, 0.05), (97, 0.01)):
            arr = ALPHA[rng.integers(0, 10, size=(40, L))]  # ACGTacgtUu
            arr = np.where(rng.random(arr.shape) < p_bad, other[rng.integers(0, len(other), size=arr.shape)], arr).astype(np.uint8)
            fs, rs, ok = sm.array_window_values(arr, mask)
            assert fs.shape == rs.shape == ok.shape == (40, L - k + 1)
            for i in range(arr.shape[0]):
                wf, wr, pos = sm.window_values(arr[i].tobytes(), mask)
                assert np.array_equal(np.flatnonzero(ok[i]), pos), (mask, L, i)
                assert np.array_equal(fs[i][ok[i]], wf) and np.array_equal(rs[i][ok[i]], wr), (mask, L, i)
            assert p_bad == 0.0 or not ok.all()
    # row blocks, reads shorter than k, reads padded to one length, and the sketches of all three strands in one pass
    arr = random_reads(rng, 300, k + 5, 0.02)
    whole = sm.array_window_values(arr, "1" * k)
    parts = list(sm.window_blocks(arr, "1" * k, rows=64))
    assert len(parts) == 5 and all(np.array_equal(np.concatenate([p[j] for p in parts]), whole[j]) for j in range(3))
    assert sm.array_window_values(arr[:, :k - 1], "1" * k)[0].shape == (300, 0)
    reads = [arr[i, :k + 5 - (i % 9)].tobytes() for i in range(300)]
    for strand in (sm.CANONICAL, sm.FORWARD, sm.REVERSE):
        got = sm.array_sketches(sm.pad_reads(reads), "1" * k, [(strand, 10, 7)])[strand, 10, 7]
        want = sm.model_sketch(reads, ["1" * k], strand, 10, 7)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and want[0].any()


# ---- ABI ----
def test_header_and_library_carry_the_strand_additions():
    text = open(HEADER).read()
    assert re.search(r"#define\s+NTC_FLAG_STRAND_FORWARD\s+512u", text) and re.search(r"#define\s+NTC_FLAG_STRAND_REVERSE\s+1024u", text)
    assert re.search(r"#define\s+NTC_ABI_VERSION\s+6\b", text)
    assert "ntc_hash_dump_strand_device" in text
    L = _abi.lib()
    assert hasattr(L, "ntc_hash_dump_strand_device") and "ntc_hash_dump_strand_device" in _abi.ABI_SYMBOLS
    assert L.ntc_abi_version() == 6
    import ntcard_amd as nt
    assert nt.FLAG_STRAND_FORWARD == FWD and nt.FLAG_STRAND_REVERSE == REV and callable(nt.hash_dump_strand_device)


@pytest.mark.parametrize("seeded", [False, True])
def test_both_strand_flags_are_refused_before_the_device(seeded):
    L = _abi.lib()
    h = C.c_void_p()
    if seeded:
        c = _abi.NtcConfig(r_bits=20, s_bits=7, device=0, flags=FWD | REV)
        arr = (C.c_char_p * 1)(b"110011")
        rc = L.ntc_create_seeded(C.byref(c), 1, arr, C.byref(h))
    else:
        rc = L.ntc_create(C.byref(abi_config(r_bits=20, flags=FWD | REV)), C.byref(h))
    assert rc == ERR_ARG and not h.value
    assert b"device" not in L.ntc_last_error() and b"STRAND" in L.ntc_last_error()


def test_hash_dump_strand_rejects_a_bad_strand_before_the_device():
    L = _abi.lib()
    buf = (C.c_uint8 * 64)()
    out = (C.c_uint64 * 64)()
    cnt = (C.c_uint32 * 4)()
    addr = (C.addressof(buf) + 15) & ~15
    for strand, seed in ((3, b"1111"), (7, b"1101"), (1, b"11x1"), (2, b"000")):
        rc = L.ntc_hash_dump_strand_device(0, None, C.c_void_p(addr), 1, 8, 8, seed, strand, 8, C.cast(out, C.c_void_p), C.cast(cnt, C.c_void_p))
        assert rc == ERR_ARG and b"device" not in L.ntc_last_error().replace(b"ntc_hash_dump_strand_device", b"")


@pytest.mark.parametrize("flags,k,gap", [(FWD, (32,), 0), (REV, (16, 24, 32, 48), 0), (FWD, (12,), 2), (REV | 1, (32,), 0), (FWD | 64 | 128, (32,), 0)])
def test_a_single_strand_flag_reaches_the_device_probe(flags, k, gap):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present (the GPU tests create strand engines)")
    L = _abi.lib()
    h = C.c_void_p()
    assert L.ntc_create(C.byref(abi_config(r_bits=20, k=k, gap=gap, flags=flags)), C.byref(h)) == -2 and not h.value
    c = _abi.NtcConfig(r_bits=20, s_bits=7, device=0, flags=flags & ~1)
    arr = (C.c_char_p * 2)(b"110011", b"1111")
    assert L.ntc_create_seeded(C.byref(c), 2, arr, C.byref(h)) == -2 and not h.value


def test_the_retired_flag_bits_stay_refused():
    L = _abi.lib()
    h = C.c_void_p()
    for bit in (4, 256, 1 << 20, 2048):
        assert L.ntc_create(C.byref(abi_config(r_bits=20, flags=FWD | bit)), C.byref(h)) == ERR_ARG and b"unknown flag" in L.ntc_last_error()


def test_python_strand_keyword_is_checked_before_the_library():
    import ntcard_amd as nt
    with pytest.raises(ValueError, match="strand"):
        nt.Engine([32], strand="sideways")
    with pytest.raises(ValueError, match="strand"):
        nt.Engine.from_seeds(["1101"], strand="both")
    with pytest.raises(ValueError, match="contradicts"):
        nt.Engine([32], strand="forward", flags=nt.FLAG_STRAND_REVERSE)
    with pytest.raises(ValueError, match="contradicts"):
        nt.Engine.from_seeds(["1101"], strand="canonical", flags=nt.FLAG_STRAND_FORWARD)


# ---- CLI ----
@pytest.mark.parametrize("args", [["--strand=sideways", "-k", "32"], ["--strand=", "-k", "32"], ["--strand=Forward", "--seed=1101"],
                                  ["-k", "12", "-g", "2", "--strand", "both"]])
def test_cli_strand_argument_errors(tmp_path, args):
    r = run_cli(NTCARD, args + ["-p", "x", "x.fq"], cwd=tmp_path, text=True)  # (x.fq does not exist: the usage error comes before any file is opened)
    assert r.returncode == 1
    assert "--strand" in r.stderr and "--help" in r.stderr
    assert not list(tmp_path.glob("x_*"))


def test_cli_help_lists_strand():
    r = run_cli(NTCARD, ["--help"], cwd=ROOT, text=True)
    assert r.returncode == 0 and "--strand=canonical|forward|reverse" in r.stderr
