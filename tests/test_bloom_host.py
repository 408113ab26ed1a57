"""Host tests of the Bloom filters (include/ntcard_hip.h: ntc_bloom_*): the symbols, every refusal that must come before a device is touched, the sizing
formula, the filter file, and the model of tests/bloom_model.py pinned to the oracle's primitives and to the real reference's multi-hash rows.

The model's BIT LAYOUT — bit 7 - loc % 8 of byte loc / 8 — rests on reading vendor/ntHash/lib/BloomFilter.hpp:56-66 of the reference, not on a run of it:
oracle/ builds no program that includes that header.  What IS run of the reference is its ntHashIterator with h hashes per window (the reference tool's
`hash` mode: orc.ref_hash), live where the reference binaries exist and always through the recorded rows of tests/golden/bloom_vectors.json."""
import ctypes as C
import json
import math
import os
import random

import numpy as np
import pytest

import bloom_model as bm
import orc
import strand_model as sm
from ntcard_amd import _abi
from support import ERR_ARG, FAKE, GOLD, L, offs, ptr, rseq

M, H, K = (1 << 20) + 7, 3, 32


def test_symbols_are_declared_and_exported():
    names = ["ntc_bloom_size", "ntc_bloom_insert_device", "ntc_bloom_query_device", "ntc_bloom_insert_hashes_device", "ntc_bloom_query_hashes_device",
             "ntc_bloom_popcount_device", "ntc_bloom_or_device", "ntc_bloom_write", "ntc_bloom_read"]
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "ntcard_hip.h")).read()
    for n in names:
        assert n in _abi.ABI_SYMBOLS and hasattr(L(), n) and n + "(" in text
    assert f"#define NTC_BLOOM_BLOCK {_abi.BLOOM_BLOCK}u" in text
    assert L().ntc_abi_version() == 6
    import ntcard_amd
    assert ntcard_amd.BloomFilter is not None and ntcard_amd.BLOOM_BLOCK == _abi.BLOOM_BLOCK


# (what is wrong, filter, m_bits, n_hash, k): the checks every filter call shares
BAD_FILTER = [
    ("null filter", None, M, H, K),
    ("misaligned filter", FAKE + 2, M, H, K),
    ("m_bits 0", FAKE, 0, H, K),
    ("m_bits 2^40", FAKE, 1 << 40, H, K),
    ("n_hash 0", FAKE, M, 0, K),
    ("n_hash 33", FAKE, M, 33, K),
    ("k 0", FAKE, M, H, 0),
    ("k too large", FAKE, M, H, None),
]


@pytest.mark.parametrize("what,filt,m,h,k", BAD_FILTER, ids=[b[0] for b in BAD_FILTER])
def test_bad_filter_arguments_are_refused_before_the_device(what, filt, m, h, k):
    lib = L()
    k = lib.ntc_max_k() + 1 if k is None else k
    o = offs(0, 40)
    n = C.c_uint64(77)
    assert lib.ntc_bloom_insert_device(0, None, filt, m, h, k, 0, FAKE, ptr(o), 1, C.byref(n)) == ERR_ARG and n.value == 77
    assert lib.ntc_last_error()
    assert lib.ntc_bloom_query_device(0, None, filt, m, h, k, 0, FAKE, ptr(o), 1, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bloom_insert_hashes_device(0, None, filt, m, h, k, FAKE, 4) == ERR_ARG
    assert lib.ntc_bloom_query_hashes_device(0, None, filt, m, h, k, FAKE, 4, FAKE) == ERR_ARG
    if what.split()[0] in ("null", "misaligned", "m_bits"):
        pop = C.c_uint64(5)
        assert lib.ntc_bloom_popcount_device(0, None, filt, m, C.byref(pop)) == ERR_ARG and pop.value == 5
        assert lib.ntc_bloom_or_device(0, None, filt, FAKE, m) == ERR_ARG
        assert lib.ntc_bloom_or_device(0, None, FAKE, filt, m) == ERR_ARG


def test_bad_input_arguments_are_refused_before_the_device():
    lib = L()
    n = C.c_uint64(77)
    good = offs(5, 45, 45, 90)
    for strand in (3, 7, 1 << 31):
        assert lib.ntc_bloom_insert_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG and b"strand" in lib.ntc_last_error()
        assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, None, 3, C.byref(n)) == ERR_ARG and b"offsets" in lib.ntc_last_error()
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, None, 3, FAKE, FAKE) == ERR_ARG
    down = offs(5, 45, 44, 90)
    assert lib.ntc_bloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(down), 3, C.byref(n)) == ERR_ARG and b"sequence 1" in lib.ntc_last_error()
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(down), 3, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bloom_insert_device(0, None, FAKE, M, H, K, 0, None, ptr(good), 3, C.byref(n)) == ERR_ARG and b"bases" in lib.ntc_last_error()
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, None, ptr(good), 3, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, None, FAKE) == ERR_ARG and b"output" in lib.ntc_last_error()
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, FAKE, None) == ERR_ARG
    assert lib.ntc_bloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 4) == ERR_ARG
    assert lib.ntc_bloom_query_hashes_device(0, None, FAKE, M, H, K, None, 4, FAKE) == ERR_ARG
    assert lib.ntc_bloom_query_hashes_device(0, None, FAKE, M, H, K, FAKE, 4, None) == ERR_ARG
    assert lib.ntc_bloom_popcount_device(0, None, FAKE, M, None) == ERR_ARG
    assert n.value == 77


def test_calls_without_work_need_no_device():
    """no window, no hash: NTC_OK with the counts set, on a machine without a GPU too"""
    lib = L()
    n = C.c_uint64(77)
    short = offs(3, 10, 10, 20)  # 17 bytes in all: no window of 32
    assert lib.ntc_bloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(short), 3, C.byref(n)) == 0 and n.value == 0
    assert lib.ntc_bloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 0) == 0
    assert lib.ntc_bloom_query_hashes_device(0, None, FAKE, M, H, K, None, 0, None) == 0
    assert lib.ntc_bloom_query_device(0, None, FAKE, M, H, K, 0, None, ptr(offs(9)), 0, None, None) == 0


def formula(n, h, fpr):
    return math.ceil(-n * h / math.log(1.0 - fpr ** (1.0 / h)))


@pytest.mark.parametrize("n", [1, 1000, 1_190_000_000, 35_000_000_000])
@pytest.mark.parametrize("h", [1, 3, 8, 32])
@pytest.mark.parametrize("fpr", [0.5, 0.01, 1e-4])
def test_size_is_the_formula(n, h, fpr):
    want = (formula(n, h, fpr) + 63) // 64 * 64
    m = C.c_uint64(0)
    rc = L().ntc_bloom_size(n, h, fpr, C.byref(m))
    if want >= 1 << 40:
        assert rc == ERR_ARG and m.value == 0
        return
    assert rc == 0
    assert m.value in (want - 64, want, want + 64) and m.value % 64 == 0  # (the two libms may differ in the last bit)
    assert (1.0 - math.exp(-h * n / m.value)) ** h <= fpr


def test_size_refusals():
    lib = L()
    m = C.c_uint64(9)
    for n, h, fpr in ((0, 3, 0.01), (10, 0, 0.01), (10, 33, 0.01), (10, 3, 0.0), (10, 3, 1.0), (10, 3, -0.5), (10, 3, 1.5), (10, 3, float("nan")),
                      (1 << 40, 1, 0.4), (1 << 62, 3, 0.01), (10**9, 32, 1e-300)):
        assert lib.ntc_bloom_size(n, h, fpr, C.byref(m)) == ERR_ARG and m.value == 9, (n, h, fpr)
    assert lib.ntc_bloom_size(10, 3, 0.01, None) == ERR_ARG
    import ntcard_amd as nt
    assert nt.bloom_size(1000, 0.01, 3) % 64 == 0
    with pytest.raises(nt.NtcError):
        nt.bloom_size(0, 0.01, 3)


def header(k=32, h=3, strand=1, m=77, ins=12345, reserved=0):
    return _abi.NtcBloomHeader(k=k, n_hash=h, strand=strand, reserved=reserved, m_bits=m, n_inserted=ins)


def test_file_round_trip_and_damage(tmp_path):
    lib = L()
    rng = np.random.default_rng(3)
    for m in (1, 8, 77, 4093, (1 << 20) + 7):
        img = rng.integers(0, 256, size=(m + 7) // 8, dtype=np.uint8)
        path = tmp_path / f"f{m}.bf"
        assert lib.ntc_bloom_write(str(path).encode(), C.byref(header(m=m)), ptr(img)) == 0
        assert not os.path.exists(str(path) + ".part")
        raw = path.read_bytes()
        assert raw[:8] == b"NTCBF1\0\0" and len(raw) == 40 + img.size and raw[40:] == img.tobytes()
        assert np.frombuffer(raw[8:24], dtype="<u4").tolist() == [32, 3, 1, 0] and np.frombuffer(raw[24:40], dtype="<u8").tolist() == [m, 12345]
        h = _abi.NtcBloomHeader()
        assert lib.ntc_bloom_read(str(path).encode(), C.byref(h), None, 0) == 0  # the header alone
        assert (h.k, h.n_hash, h.strand, h.reserved, h.m_bits, h.n_inserted) == (32, 3, 1, 0, m, 12345)
        back = np.zeros(img.size + 3, dtype=np.uint8)
        assert lib.ntc_bloom_read(str(path).encode(), C.byref(h), ptr(back), back.size) == 0
        assert np.array_equal(back[: img.size], img) and not back[img.size:].any()
        if img.size > 1:
            small = np.zeros(img.size - 1, dtype=np.uint8)
            h2 = _abi.NtcBloomHeader()
            assert lib.ntc_bloom_read(str(path).encode(), C.byref(h2), ptr(small), small.size) == ERR_ARG and h2.m_bits == m and not small.any()
    # the python mirror
    from ntcard_amd import bloom
    hd, image = bloom.read_file(path)
    assert hd == {"k": 32, "n_hash": 3, "strand": "forward", "m_bits": m, "n_inserted": 12345} and np.array_equal(image, img)
    # damage: cut short, grown, wrong magic, bad header fields, missing
    for name, data in (("cut", raw[:-1]), ("cut_header", raw[:39]), ("cut_magic", raw[:5]), ("grown", raw + b"\0"), ("magic", b"NTCSIG1\0" + raw[8:]),
                       ("empty", b""), ("k0", raw[:8] + b"\0\0\0\0" + raw[12:]), ("hash33", raw[:12] + b"\x21\0\0\0" + raw[16:]),
                       ("strand3", raw[:16] + b"\x03\0\0\0" + raw[20:]), ("reserved", raw[:20] + b"\x01\0\0\0" + raw[24:]),
                       ("m0", raw[:24] + b"\0" * 8 + raw[32:]), ("mhuge", raw[:24] + b"\xff" * 8 + raw[32:])):
        p = tmp_path / f"bad_{name}.bf"
        p.write_bytes(data)
        h = header(k=99)
        assert lib.ntc_bloom_read(str(p).encode(), C.byref(h), None, 0) == ERR_ARG and h.k == 99, name
    assert lib.ntc_bloom_read(str(tmp_path / "none.bf").encode(), C.byref(h), None, 0) == ERR_ARG
    assert lib.ntc_bloom_read(None, C.byref(h), None, 0) == ERR_ARG and lib.ntc_bloom_read(str(path).encode(), None, None, 0) == ERR_ARG


def test_file_write_refusals_leave_nothing_behind(tmp_path):
    lib = L()
    img = np.zeros(16, dtype=np.uint8)
    out = tmp_path / "x.bf"
    for h in (header(k=0), header(k=lib.ntc_max_k() + 1), header(h=0), header(h=33), header(strand=3), header(m=0), header(m=1 << 40), header(reserved=1)):
        assert lib.ntc_bloom_write(str(out).encode(), C.byref(h), ptr(img)) == ERR_ARG
    assert lib.ntc_bloom_write(None, C.byref(header()), ptr(img)) == ERR_ARG
    assert lib.ntc_bloom_write(str(out).encode(), None, ptr(img)) == ERR_ARG
    assert lib.ntc_bloom_write(str(out).encode(), C.byref(header()), None) == ERR_ARG
    assert os.listdir(tmp_path) == []
    # a target that cannot be written (a directory of that name; a directory that does not exist): refused, no .part left
    os.mkdir(out)
    assert lib.ntc_bloom_write(str(out).encode(), C.byref(header()), ptr(img)) == ERR_ARG and b"cannot write" in lib.ntc_last_error()
    assert os.path.isdir(out) and not os.path.exists(str(out) + ".part")
    assert lib.ntc_bloom_write(str(tmp_path / "no" / "x.bf").encode(), C.byref(header()), ptr(img)) == ERR_ARG
    # an existing file is replaced only by a whole one
    good = tmp_path / "y.bf"
    assert lib.ntc_bloom_write(str(good).encode(), C.byref(header(m=128)), ptr(img)) == 0
    first = good.read_bytes()
    assert lib.ntc_bloom_write(str(good).encode(), C.byref(header(m=0)), ptr(img)) == ERR_ARG and good.read_bytes() == first


# ---- the model ----
def test_model_arithmetic_is_the_oracles():
    lib = orc.lib()
    rng = random.Random(5)
    h0 = np.array([0, 1, 2**64 - 1, 2**63, 2**32] + [rng.getrandbits(64) for _ in range(200)], dtype=np.uint64)
    for k in (1, 32, 127, 600):
        mh = bm.multihash(h0, 32, k)
        assert np.array_equal(mh[:, 0], h0)
        for i in (1, 2, 7, 31):
            assert mh[:, i].tolist() == [lib.orc_multihash(int(x), i, k) for x in h0]
    for m in (1, 7, 4093, 2**20 + 7, 2**32 - 5, 2**33 + 9, 2**40 - 1):
        pos = bm.positions(h0, 4, 32, m)
        assert pos.tolist() == [[int(x) % m for x in row] for row in bm.multihash(h0, 4, 32)]


def test_model_bit_rule():
    """bit 7 - loc % 8 of byte loc / 8 (BloomFilter.hpp:56-66): position 0 is the TOP bit of byte 0"""
    assert bm.image_of([0], 16).tolist() == [0x80, 0]
    assert bm.image_of([7, 8], 16).tolist() == [0x01, 0x80]
    assert bm.image_of([9, 9, 15], 16).tolist() == [0, 0x41]
    img = bm.image_of([3, 12], 13)
    assert img.size == 2 and bm.bits_set(img, np.array([[3, 12], [3, 11]])).tolist() == [[True, True], [True, False]]
    assert bm.popcount(img) == 2


def test_model_one_strand_is_the_window_walk():
    rng = random.Random(8)
    seqs = [rseq(rng, n, pn=0.03) for n in (0, 1, 30, 31, 32, 33, 90, 200)] + [b"", b"ACGTUacgtu" * 5]
    for k in (1, 31, 32):
        for strand in (sm.FORWARD, sm.REVERSE, sm.CANONICAL):
            want = [sm.strand_hash(s, "1" * k, strand) for s in seqs]
            got = bm.h0_values(seqs, k, strand)
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (k, strand)


def check_rows(seqs, k, h, m, rows):
    """the reference tool's rows (pos[], hashes[n, h]) per sequence against the model's positions"""
    vals = bm.h0_values(seqs, k, sm.CANONICAL)
    for s, v, (pos, hs) in zip(seqs, vals, rows):
        assert np.array_equal(pos, orc.hash_read(s, k)[1])
        assert np.array_equal(bm.multihash(v, h, k), hs)
        assert bm.positions(v, h, k, m).tolist() == [[int(x) % m for x in row] for row in hs]


def test_model_is_the_recorded_reference():
    with open(os.path.join(GOLD, "bloom_vectors.json")) as f:
        gold = json.load(f)
    seqs = [s.encode() for s in gold["sequences"]]
    assert gold["cases"]
    for c in gold["cases"]:
        rows = [(np.array([r[0] for r in rs], dtype=np.uint32), np.array([[int(x, 16) for x in r[1:]] for r in rs], dtype=np.uint64).reshape(len(rs), c["h"]))
                for rs in c["rows"]]
        assert sum(len(r[0]) for r in rows) > 0
        check_rows(seqs, c["k"], c["h"], c["m"], rows)


@pytest.mark.skipif(not orc.have_ref(), reason="the reference binaries exist only where the reference sources do")
@pytest.mark.parametrize("h", [1, 3, 8])
def test_model_is_the_live_reference(h):
    rng = random.Random(40 + h)
    seqs = [rseq(rng, n, pn=0.02) for n in (40, 64, 65, 150, 300)]
    for k in (12, 32, 33, 64):
        check_rows(seqs, k, h, (1 << 20) + 7, orc.ref_hash(seqs, k, h))
