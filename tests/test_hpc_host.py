"""CPU tests of homopolymer-compressed counting (include/ntcard_hip.h: NTC_FLAG_HPC, ntc_hpc_compress, ntc_hpc_compress_device, ntc_hpc_stats,
ntc_hpc_time): the host compression against the pure-Python model of tests/hpc_model.py, and the flag and argument handling, which comes before a
device is looked for."""
import ctypes as C
import random

import numpy as np
import pytest

import hpc_model as hm
import ntcard_amd as nt
from ntcard_amd import _abi
from support import abi_config, created, hll_create_ex

ERR_ARG = -1
HPC, FWD, REV, STRAND_TILED = 8192, 512, 1024, 4096
NEW_SYMBOLS = ["ntc_hpc_compress", "ntc_hpc_compress_device", "ntc_hpc_stats", "ntc_hpc_time"]


def test_library_exports_the_symbols():
    L = _abi.lib()
    for name in NEW_SYMBOLS:
        assert name in _abi.ABI_SYMBOLS and hasattr(L, name), name
    assert L.ntc_abi_version() == 6  # additive: the ABI version stays
    assert nt.FLAG_HPC == HPC
    assert callable(nt.hpc_compress) and callable(nt.hpc_compress_device) and hasattr(nt.Engine, "hpc_stats") and hasattr(nt.Engine, "hpc_time")


# ---- the model ----
def test_model_forms_agree_and_follow_the_definition():
    rng = random.Random(1)
    for _ in range(200):
        s = bytes(rng.choice(b"ACGTacgtUuNnR\r\x01\x03") for _ in range(rng.randrange(0, 60)))
        assert hm.compress(s) == hm.compress_slow(s)
    assert hm.compress(b"aAAa") == b"a" and hm.compress(b"NNN") == b"NNN" and hm.compress(b"TtUu") == b"T"
    assert hm.compress(b"AANAA") == b"ANA" and hm.compress(b"") == b""
    assert hm.compress(b"\x01\x01\x03\x03\x04\x05\x05\x07\x07") == b"\x01\x01\x03\x03\x04\x05\x05\x07\x07"  # what the seed table takes for bases has no class
    for s in hm.device_set():
        assert hm.compress(s) == hm.compress_slow(s)


def test_the_device_set_holds_what_the_gpu_tests_say():
    seqs = hm.device_set()
    comp = hm.model(seqs)
    assert b"" in seqs and any(len(s) == 1 for s in seqs) and seqs[-1] == b""
    assert any(a and b and hm.CLASS[a[-1]] == hm.CLASS[b[0]] != hm.NONE for a, b in zip(seqs, seqs[1:]))
    assert any(len(s) > 100 and len(c) == 1 for s, c in zip(seqs, comp))
    assert any(len(s) > 70_000 and len(c) == 5 for s, c in zip(seqs, comp))
    assert sum(len(s) for s in seqs) < 600_000 and max(len(s) for s in seqs) == 300_000
    assert 0.3 < sum(len(c) for c in comp) / sum(len(s) for s in seqs) < 0.9
    s0 = seqs[0]  # the straddling runs: for every boundary and lead a run of three begins at each of the four shifts
    for B in hm.STRADDLE:
        for lead in range(4):
            for d in (-2, -1, 0, 1):
                assert any(hm.CLASS[s0[j]] == hm.CLASS[s0[j + 1]] == hm.CLASS[s0[j + 2]] for j in range(3, len(s0) - 3) if (lead + j - d) % B == 0), (B, lead, d)


def test_compress_many_is_compress_per_sequence():
    """the one-pass model of the large GPU inputs against compress() sequence by sequence: on the device set (with and without bytes in front of the first
    offset) and on a sample of the 530 000 short sequences"""
    seqs = hm.device_set()
    want = hm.model(seqs)
    for lead in (0, 3):
        buf = np.frombuffer(b"G" * lead + b"".join(seqs), dtype=np.uint8)
        out, offs = hm.compress_many(buf, hm.offsets_of(seqs, lead))
        assert offs.dtype == np.uint64 and np.array_equal(offs, hm.offsets_of(want)) and out.tobytes() == b"".join(want)
    buf, offs = hm.many_short()
    out, new = hm.compress_many(buf, offs)
    assert len(offs) - 1 == 530_000 and int(np.diff(offs).max()) == 20 and int(np.diff(offs).min()) == 0
    for i in list(range(3000)) + list(range(len(offs) - 3000, len(offs) - 1)):
        assert hm.compress(buf[int(offs[i]):int(offs[i + 1])].tobytes()) == out[int(new[i]):int(new[i + 1])].tobytes(), i
    sub, sub_offs = hm.compress_many(buf, offs[1000:2001])  # a call that starts in the middle of the buffer
    assert np.array_equal(sub_offs, new[1000:2001] - new[1000]) and np.array_equal(sub, out[int(new[1000]):int(new[2000])])
    for total in (4_194_301, 4_194_306):
        a, o = hm.three_seqs(total)
        c, no = hm.compress_many(a, o)
        assert c.tobytes() == b"".join(hm.compress(a[int(o[i]):int(o[i + 1])].tobytes()) for i in range(3))
        assert int(no[3] - no[2]) == 1 and (a[int(o[2]) - 1] | 0x20) == ord("g")  # the run goes on across the join: its first byte behind it is kept, alone


# ---- ntc_hpc_compress ----
def c_compress(seq, in_place=False):
    L = _abi.lib()
    n = C.c_uint64(0xdead)
    src = C.create_string_buffer(bytes(seq), max(len(seq), 1))
    dst = src if in_place else C.create_string_buffer(max(len(seq), 1))
    assert L.ntc_hpc_compress(src, len(seq), dst, C.byref(n)) == 0
    assert n.value <= len(seq)
    return dst.raw[:n.value]


@pytest.mark.parametrize("in_place", [False, True])
def test_compress_matches_the_model(in_place):
    rng = random.Random(5)
    for i in range(300):
        n = rng.randrange(0, 200) if i < 280 else rng.randrange(5000, 20000)
        s = hm.runs_seq(rng, n, p_more=0.6, p_low=0.3, p_other=0.1) if i % 2 else bytes(rng.choice(b"ACGTacgtUuNnR\r\x01\x03") for _ in range(n))
        assert c_compress(s, in_place) == hm.compress(s), s
    for s in (b"", b"A", b"N", b"G" * 1000, b"TtUu", b"NNN", b"aAAa"):
        assert c_compress(s, in_place) == hm.compress(s), s
    assert c_compress(b"G" * 1000, in_place) == b"G" and c_compress(b"TtUu", in_place) == b"T" and c_compress(b"NNN", in_place) == b"NNN"
    assert c_compress(b"aAAa", in_place) == b"a"


def test_every_pair_of_byte_values():
    """ntc_hpc_compress on all 256 byte values in front of and behind every other: one sequence that holds every ordered pair, and every pair as a
    sequence of its own — against the definition, pair by pair"""
    seq, _ = hm.pair_seq()
    pairs = {(int(seq[j]), int(seq[j + 1])) for j in range(0, seq.size, 2)}
    assert len(pairs) == 65536 and seq.size == 131072
    for in_place in (False, True):
        assert c_compress(seq.tobytes(), in_place) == hm.compress(seq.tobytes()) == hm.compress_slow(seq.tobytes())
    want, offs = hm.pair_want()
    assert int(offs[-1]) == 131072 - 28  # (4 + 4 + 4 + 16 ordered pairs of one class)
    raw = seq.tobytes()
    for i in range(65536):
        got = c_compress(raw[2 * i:2 * i + 2])
        assert got == want[int(offs[i]):int(offs[i + 1])].tobytes(), (raw[2 * i], raw[2 * i + 1], got)
    got, got_offs = hm.compress_many(*hm.pair_seqs())
    assert np.array_equal(got, want) and np.array_equal(got_offs, offs)


def test_python_compress():
    for s in hm.device_set()[1:12]:
        assert nt.hpc_compress(s) == hm.compress(s)
    assert nt.hpc_compress(b"") == b"" and nt.hpc_compress(bytearray(b"ccC")) == b"c"


def test_compress_argument_errors():
    L = _abi.lib()
    n = C.c_uint64()
    buf = C.create_string_buffer(b"ACGT")
    assert L.ntc_hpc_compress(buf, 4, buf, None) == ERR_ARG
    assert L.ntc_hpc_compress(None, 4, buf, C.byref(n)) == ERR_ARG and L.ntc_hpc_compress(buf, 4, None, C.byref(n)) == ERR_ARG
    assert L.ntc_hpc_compress(None, 0, None, C.byref(n)) == 0 and n.value == 0


# ---- the flag ----
@pytest.mark.parametrize("beside", [0, 1, 2, 8, 16, 32, 64, 128, FWD, REV, FWD | STRAND_TILED])
def test_create_takes_the_flag_beside_every_other(beside):
    L = _abi.lib()
    h = C.c_void_p()
    assert created(L.ntc_create(C.byref(abi_config(flags=HPC | beside)), C.byref(h)), h, L)


def test_create_seeded_takes_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    c = _abi.NtcConfig(n_k=0, k=None, gap=0, r_bits=14, s_bits=7, device=0, flags=HPC)
    seeds = (C.c_char_p * 1)(b"1110111")
    assert created(L.ntc_create_seeded(C.byref(c), 1, seeds, C.byref(h)), h, L)


def test_the_retired_bits_stay_refused_beside_the_flag():
    L = _abi.lib()
    h = C.c_void_p()
    for bit in (4, 256, 2048, 1 << 20):
        assert L.ntc_create(C.byref(abi_config(flags=HPC | bit)), C.byref(h)) == ERR_ARG and b"unknown flag" in L.ntc_last_error()
    assert L.ntc_create(C.byref(abi_config(flags=HPC | FWD | REV)), C.byref(h)) == ERR_ARG
    assert L.ntc_create(C.byref(abi_config(flags=HPC | STRAND_TILED)), C.byref(h)) == ERR_ARG


def hll_create(flags):
    return hll_create_ex(k=[32], n_bits=12, flags=flags)


@pytest.mark.parametrize("flags", [HPC, HPC | FWD, HPC | REV])
def test_hll_create_takes_the_flag(flags):
    rc, h, L = hll_create(flags)
    assert created(rc, h, L)


@pytest.mark.parametrize("flags", [HPC | STRAND_TILED, HPC | FWD | STRAND_TILED, HPC | FWD | REV, HPC | 64])
def test_hll_create_refuses_what_it_refused(flags):
    rc, h, L = hll_create(flags)
    assert rc == ERR_ARG and not h
    if flags & (STRAND_TILED | 64):
        assert b"unknown flag" in L.ntc_last_error()


def test_python_keyword_sets_the_bit(monkeypatch):
    seen = []
    L = _abi.lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name in ("ntc_create", "ntc_create_seeded", "ntc_hll_create_ex"):
                def wrapped(cfg_ref, *rest):
                    seen.append((name, cfg_ref._obj.flags))
                    return ERR_ARG  # (no engine: the constructor raises)
                return wrapped
            return fn

    monkeypatch.setattr(_abi, "_lib", Spy())
    for make in (lambda **kw: nt.Engine([32], r_bits=14, **kw), lambda **kw: nt.Engine.from_seeds(["1101"], r_bits=14, **kw),
                 lambda **kw: nt.HllEngine(32, **kw), lambda **kw: nt.HllEngine.from_seeds(["1101"], **kw)):
        for kw, want in ((dict(hpc=True), HPC), (dict(), 0), (dict(hpc=True, strand="forward"), HPC | FWD)):
            seen.clear()
            with pytest.raises(nt.NtcError):
                make(**kw)
            assert len(seen) == 1 and seen[0][1] == want, (kw, seen)


# ---- ntc_hpc_compress_device, ntc_hpc_stats, ntc_hpc_time: refused before a device is looked for ----
def test_bad_device_calls_are_rejected_before_touching_the_device():
    L = _abi.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: the argument checks come first
    offs = (C.c_uint64 * 3)(0, 100, 300)
    down = (C.c_uint64 * 3)(0, 200, 100)
    out = (C.c_uint64 * 3)()
    call = lambda d_in, o, d_out, oo: L.ntc_hpc_compress_device(0, None, d_in, o, 2, d_out, oo)
    assert call(fake, None, fake, out) == ERR_ARG and b"null offsets" in L.ntc_last_error()
    assert call(fake, offs, fake, None) == ERR_ARG and b"null offsets" in L.ntc_last_error()
    assert call(fake, down, fake, out) == ERR_ARG and b"monotone" in L.ntc_last_error()
    assert call(None, offs, fake, out) == ERR_ARG and b"null buffer" in L.ntc_last_error()
    assert call(fake, offs, None, out) == ERR_ARG and b"null buffer" in L.ntc_last_error()
    empty = (C.c_uint64 * 3)(7, 7, 7)
    out[:] = [9, 9, 9]
    assert call(None, empty, None, out) == 0 and list(out) == [0, 0, 0]  # nothing to compress: no device needed
    a, b = C.c_uint64(), C.c_uint64()
    assert L.ntc_hpc_stats(None, C.byref(a), C.byref(b)) == ERR_ARG
    assert L.ntc_hpc_time(None, None) == ERR_ARG
    with pytest.raises(nt.NtcError):
        nt.hpc_compress_device(0x1000, [0, 5, 3], 0x2000)
