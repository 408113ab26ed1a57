"""Host tests of the blocked Bloom filters (include/ntcard_hip.h: ntc_bbloom_*): the symbols, every refusal that must come before a device is touched, the
false positive rate formula and the sizing built on it, the filter file, the model of tests/bbloom_model.py pinned to Python integers — and the SCHEME
itself: that blocks and in-block positions taken from one ntHash value and its multi-hashes behave like independent uniform choices, which is what the
formula assumes."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bbloom_model as bb
import bloom_model as bm
from ntcard_amd import _abi
from support import ERR_ARG, FAKE, GOLD, L, offs, ptr

M, H, K = 1000 * 512, 3, 32
CM = (1 << 20) + 7  # a counting filter's counters


NAMES = ["ntc_bbloom_fpr", "ntc_bbloom_size", "ntc_bbloom_insert_device", "ntc_bbloom_query_device", "ntc_bbloom_insert_hashes_device",
         "ntc_bbloom_query_hashes_device", "ntc_bbloom_hist_device", "ntc_bbloom_insert_solid_device", "ntc_bbloom_write", "ntc_bbloom_read"]


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "ntcard_hip.h")).read()
    for n in NAMES:
        assert n in _abi.ABI_SYMBOLS and hasattr(L(), n) and n + "(" in text
    assert f"#define NTC_BBLOOM_BLOCK_BITS {_abi.BBLOOM_BLOCK_BITS}u" in text and _abi.BBLOOM_BLOCK_BITS == bb.BLOCK
    assert L().ntc_abi_version() == 6
    import ntcard_amd
    assert ntcard_amd.BlockedBloomFilter is not None and ntcard_amd.BBLOOM_BLOCK_BITS == 512
    # the header says that the image is an ordinary bit image which the plain popcount and OR serve
    assert "ntc_bloom_popcount_device and ntc_bloom_or_device serve a blocked filter unchanged" in text


# (what is wrong, filter, m_bits, n_hash, k): the checks every blocked-filter call shares
BAD_FILTER = [
    ("null filter", None, M, H, K),
    ("misaligned filter", FAKE + 2, M, H, K),
    ("m_bits 0", FAKE, 0, H, K),
    ("m_bits 511", FAKE, 511, H, K),
    ("m_bits 513", FAKE, 513, H, K),
    ("m_bits 64", FAKE, 64, H, K),
    ("m_bits odd multiple of 64", FAKE, 512 * 1000 + 64, H, K),
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
    assert lib.ntc_bbloom_insert_device(0, None, filt, m, h, k, 0, FAKE, ptr(o), 1, C.byref(n)) == ERR_ARG and n.value == 77
    assert lib.ntc_last_error()
    assert lib.ntc_bbloom_query_device(0, None, filt, m, h, k, 0, FAKE, ptr(o), 1, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bbloom_insert_hashes_device(0, None, filt, m, h, k, FAKE, 4) == ERR_ARG
    assert lib.ntc_bbloom_query_hashes_device(0, None, filt, m, h, k, FAKE, 4, FAKE) == ERR_ARG
    assert lib.ntc_bbloom_insert_solid_device(0, None, filt, m, h, FAKE, CM, 3, 2, k, 0, FAKE, ptr(o), 1, C.byref(n)) == ERR_ARG and n.value == 77
    if what.split()[0] in ("null", "misaligned", "m_bits"):
        hist = np.full(513, 5, dtype=np.uint64)
        assert lib.ntc_bbloom_hist_device(0, None, filt, m, ptr(hist)) == ERR_ARG and (hist == 5).all()
    if what.startswith("m_bits"):
        assert b"512" in lib.ntc_last_error()
        fpr = C.c_double(7.0)
        assert lib.ntc_bbloom_fpr(1000, m, 3, C.byref(fpr)) == ERR_ARG and fpr.value == 7.0


def test_bad_input_arguments_are_refused_before_the_device():
    lib = L()
    n = C.c_uint64(77)
    good = offs(5, 45, 45, 90)
    for strand in (3, 7, 1 << 31):
        assert lib.ntc_bbloom_insert_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG and b"strand" in lib.ntc_last_error()
        assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, FAKE, FAKE) == ERR_ARG
        assert lib.ntc_bbloom_insert_solid_device(0, None, FAKE, M, H, FAKE, CM, 3, 2, K, strand, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG
    assert lib.ntc_bbloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, None, 3, C.byref(n)) == ERR_ARG and b"offsets" in lib.ntc_last_error()
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, None, 3, FAKE, FAKE) == ERR_ARG
    down = offs(5, 45, 44, 90)
    assert lib.ntc_bbloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(down), 3, C.byref(n)) == ERR_ARG and b"sequence 1" in lib.ntc_last_error()
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(down), 3, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bbloom_insert_solid_device(0, None, FAKE, M, H, FAKE, CM, 3, 2, K, 0, FAKE, ptr(down), 3, C.byref(n)) == ERR_ARG
    assert lib.ntc_bbloom_insert_device(0, None, FAKE, M, H, K, 0, None, ptr(good), 3, C.byref(n)) == ERR_ARG and b"bases" in lib.ntc_last_error()
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, None, ptr(good), 3, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, None, FAKE) == ERR_ARG and b"output" in lib.ntc_last_error()
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, FAKE, None) == ERR_ARG
    assert lib.ntc_bbloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 4) == ERR_ARG
    assert lib.ntc_bbloom_insert_hashes_device(0, None, FAKE, M, H, K, FAKE + 4, 4) == ERR_ARG and b"8-byte" in lib.ntc_last_error()
    assert lib.ntc_bbloom_query_hashes_device(0, None, FAKE, M, H, K, None, 4, FAKE) == ERR_ARG
    assert lib.ntc_bbloom_query_hashes_device(0, None, FAKE, M, H, K, FAKE, 4, None) == ERR_ARG
    assert lib.ntc_bbloom_hist_device(0, None, FAKE, M, None) == ERR_ARG
    # the solid insert: its counting filter and its count
    for counters, cm, ch, c in ((None, CM, 3, 2), (FAKE + 1, CM, 3, 2), (FAKE, 0, 3, 2), (FAKE, CM, 0, 2), (FAKE, CM, 33, 2), (FAKE, CM, 3, 0), (FAKE, CM, 3, 256)):
        assert lib.ntc_bbloom_insert_solid_device(0, None, FAKE, M, H, counters, cm, ch, c, K, 0, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG, (counters, cm, ch, c)
    assert n.value == 77


def test_calls_without_work_need_no_device():
    """no window, no hash: NTC_OK with the counts set, on a machine without a GPU too"""
    lib = L()
    n = C.c_uint64(77)
    short = offs(3, 10, 10, 20)  # 17 bytes in all: no window of 32
    assert lib.ntc_bbloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(short), 3, C.byref(n)) == 0 and n.value == 0
    n.value = 77
    assert lib.ntc_bbloom_insert_solid_device(0, None, FAKE, M, H, FAKE, CM, 3, 2, K, 0, FAKE, ptr(short), 3, C.byref(n)) == 0 and n.value == 0
    assert lib.ntc_bbloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 0) == 0
    assert lib.ntc_bbloom_query_hashes_device(0, None, FAKE, M, H, K, None, 0, None) == 0
    assert lib.ntc_bbloom_query_device(0, None, FAKE, M, H, K, 0, None, ptr(offs(9)), 0, None, None) == 0


# ---- the model ----
@pytest.mark.parametrize("n_hash", [1, 3, 4, 5, 8, 9, 32])
def test_model_positions_are_the_definition_in_python_integers(n_hash):
    rng = random.Random(n_hash)
    vals = [0, 1, 2**64 - 1, 2**63, 2**32, 511, 512] + [rng.getrandbits(64) for _ in range(300)]
    h0 = np.array(vals, dtype=np.uint64)
    for k in (1, 32, 600):
        for m in (512, 3 * 512, 8 * 512, 1000 * 512, 2**32 + 3 * 512, 2**40 - 512):
            pos = bb.positions(h0, n_hash, k, m)
            assert pos.tolist() == [bb.positions_scalar(v, n_hash, k, m) for v in vals], (k, m)
            assert (pos < m).all() and ((pos // np.uint64(512)) == (pos[:, :1] // np.uint64(512))).all()  # one block per value
    # positions 4 q .. 4 q + 3 are the four 9-bit fields of the top 36 bits of multi-hash 1 + q, highest first
    mh = bm.multihash(h0, 9, 32)
    pos = bb.positions(h0, n_hash, 32, 512)
    for i in range(n_hash):
        top36 = [int(g) >> 28 for g in mh[:, 1 + i // 4]]
        assert pos[:, i].tolist() == [(t >> (27 - 9 * (i % 4))) & 511 for t in top36]


def test_model_image_and_histogram():
    img = bb.image_of(np.array([0], dtype=np.uint64), 1, 32, 1024)
    assert bm.popcount(img) == 1 and img[:64].any() and not img[64:].any()  # h_0 = 0: block 0
    h0 = np.arange(1, 4000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    img = bb.image_of(h0, 3, 32, 8 * 512)
    assert bb.test_values(img, h0, 3, 32, 8 * 512).all()
    hist = bb.block_hist(img)
    assert hist.size == 513 and int(hist.sum()) == 8 and int((hist * np.arange(513, dtype=np.uint64)).sum()) == bm.popcount(img)
    assert bb.realised_fpr(np.zeros(128, dtype=np.uint8), 3) == 0.0 and bb.realised_fpr(np.full(128, 0xFF, dtype=np.uint8), 3) == 1.0


# ---- the formula and the size ----
@pytest.mark.parametrize("n_hash", [1, 2, 3, 4, 8, 32])
def test_fpr_is_the_models_formula(n_hash):
    """to 1e-9 relative: the sum has a few hundred positive terms, each an exp of an argument of at most a few hundred — an error of about 1e-13; 1e-9
    leaves room for another lgamma"""
    lib = L()
    for n, m in ((1, 512), (1, 2**39), (50_000, 630_784), (50_000, 512), (1000, 512 * 4), (10**6, 512 * 1000), (1_190_000_000, 11_400_000_000 // 512 * 512),
                 (35_000_000_000, 2**40 - 512), (3 * 10**6, 512 * 100), (200_000, 512)):
        fpr = C.c_double(-1.0)
        assert lib.ntc_bbloom_fpr(n, m, n_hash, C.byref(fpr)) == 0
        want = bb.fpr(n, m, n_hash)
        assert 0.0 < want <= 1.0 + 1e-9 and fpr.value == pytest.approx(want, rel=1e-9), (n, m, fpr.value, want)
        assert fpr.value <= 1.0
    fpr = C.c_double(-1.0)
    assert lib.ntc_bbloom_fpr(0, 512, n_hash, C.byref(fpr)) == 0 and fpr.value == 0.0
    assert lib.ntc_bbloom_fpr(10, 512, n_hash, None) == ERR_ARG
    assert lib.ntc_bbloom_fpr(10, 512, 0, C.byref(fpr)) == ERR_ARG and lib.ntc_bbloom_fpr(10, 512, 33, C.byref(fpr)) == ERR_ARG


def test_fpr_at_one_hash_is_the_plain_filters():
    """n_hash = 1: sum_j P(j) (1 - q^j) = 1 - exp(-l / 512) = 1 - exp(-n / m) — blocking costs nothing with one hash"""
    import math
    for n, m in ((1000, 512 * 4), (50_000, 512 * 1000), (10**6, 512 * 100)):
        fpr = C.c_double(0)
        assert L().ntc_bbloom_fpr(n, m, 1, C.byref(fpr)) == 0
        assert fpr.value == pytest.approx(-math.expm1(-n / m), rel=1e-9)


def lib_fpr(n, m, h):
    fpr = C.c_double(-1.0)
    assert L().ntc_bbloom_fpr(n, m, h, C.byref(fpr)) == 0
    return fpr.value


@pytest.mark.parametrize("n", [1, 1000, 1_190_000_000, 35_000_000_000])
@pytest.mark.parametrize("h", [1, 3, 8, 32])
@pytest.mark.parametrize("fpr", [0.5, 0.01, 1e-4])
def test_size_is_the_smallest_that_meets_the_rate(n, h, fpr):
    m = C.c_uint64(0)
    rc = L().ntc_bbloom_size(n, h, fpr, C.byref(m))
    if lib_fpr(n, (1 << 40) - 512, h) > fpr:  # the largest legal filter misses the rate: refused as ntc_bloom_size refuses
        assert rc == ERR_ARG and m.value == 0 and b"2^40 bits or more" in L().ntc_last_error()
        return
    assert rc == 0 and m.value % 512 == 0 and 512 <= m.value < 1 << 40
    assert lib_fpr(n, m.value, h) <= fpr
    if m.value > 512:
        assert fpr < lib_fpr(n, m.value - 512, h)
    if h == 1:  # one hash: the plain filter's size, within a block
        plain = C.c_uint64(0)
        assert L().ntc_bloom_size(n, 1, fpr, C.byref(plain)) == 0 and abs(int(m.value) - int(plain.value)) <= 512


def test_size_refuses_somewhere_on_the_grid():
    """(the grid above holds both outcomes)"""
    m = C.c_uint64(0)
    assert L().ntc_bbloom_size(35_000_000_000, 1, 1e-4, C.byref(m)) == ERR_ARG
    assert L().ntc_bbloom_size(35_000_000_000, 3, 0.01, C.byref(m)) == 0 and m.value > 35_000_000_000 * 9


def test_size_refusals():
    lib = L()
    m = C.c_uint64(9)
    for n, h, fpr in ((0, 3, 0.01), (10, 0, 0.01), (10, 33, 0.01), (10, 3, 0.0), (10, 3, 1.0), (10, 3, -0.5), (10, 3, 1.5), (10, 3, float("nan")),
                      (1 << 40, 1, 0.4), (1 << 62, 3, 0.01), (10**9, 32, 1e-300)):
        assert lib.ntc_bbloom_size(n, h, fpr, C.byref(m)) == ERR_ARG and m.value == 9, (n, h, fpr)
    assert lib.ntc_bbloom_size(10, 3, 0.01, None) == ERR_ARG
    import ntcard_amd as nt
    m3 = nt.bbloom_size(1000, 0.01, 3)
    assert m3 % 512 == 0 and nt.bbloom_fpr(1000, m3, 3) <= 0.01 < nt.bbloom_fpr(1000, m3 - 512, 3)
    # at three hashes and 1 % a blocked filter needs about 2 % more bits than a plain one
    assert 1.01 < nt.bbloom_size(10**8, 0.01, 3) / nt.bloom_size(10**8, 0.01, 3) < 1.03
    with pytest.raises(nt.NtcError):
        nt.bbloom_size(0, 0.01, 3)


# ---- the scheme against the formula: a condition, not a measurement ----
N_KEYS, N_QUERIES, N_SETS = 50_000, 1 << 18, 16


def pooled_rate(m, n_hash, ideal):
    """false positives / queries over 16 key sets of 50 000 uniform 64-bit values and 2^18 absent queries each.  ideal: the block still comes from the
    value, the in-block positions are drawn uniformly in the test itself instead of coming from the multi-hash"""
    fp = 0
    for s in range(N_SETS):
        rng = np.random.default_rng(100 + s)
        keys = rng.integers(0, 2**64, size=N_KEYS, dtype=np.uint64)
        qs = rng.integers(0, 2**64, size=N_QUERIES, dtype=np.uint64)
        if ideal:
            nb = np.uint64(m // 512)
            kp = (keys % nb)[:, None] * np.uint64(512) + rng.integers(0, 512, size=(N_KEYS, n_hash), dtype=np.uint64)
            qp = (qs % nb)[:, None] * np.uint64(512) + rng.integers(0, 512, size=(N_QUERIES, n_hash), dtype=np.uint64)
        else:
            kp, qp = bb.positions(keys, n_hash, 32, m), bb.positions(qs, n_hash, 32, m)
        bits = np.zeros(m, dtype=bool)
        bits[kp.ravel().astype(np.int64)] = True
        fp += int(bits[qp.astype(np.int64)].all(axis=1).sum())
    return fp / (N_SETS * N_QUERIES)


@pytest.mark.parametrize("n_hash", [3, 4, 8])
def test_scheme_meets_the_formula(n_hash):
    """The pooled false positive rate of the model lies within 5 % of the formula, and so does that of ideal uniform in-block positions: with about
    42 000 false positives pooled the counting error is 0.5 %.  A block and position choice that are correlated, or a wrong formula, miss by far more.
    Repeated with m rounded up to a power of two, where the block is the low bits of the value."""
    import ntcard_amd as nt
    m = nt.bbloom_size(N_KEYS, 0.01, n_hash)
    m2 = 1 << (m - 1).bit_length()
    assert m2 > m and m2 & (m2 - 1) == 0
    for mm in (m, m2):
        want = nt.bbloom_fpr(N_KEYS, mm, n_hash)
        got, ideal = pooled_rate(mm, n_hash, False), pooled_rate(mm, n_hash, True)
        print(f"n_hash {n_hash} m {mm}: formula {want:.6f} model {got:.6f} ideal {ideal:.6f}")
        assert abs(got - want) <= 0.05 * want, (mm, got, want)
        assert abs(ideal - want) <= 0.05 * want, (mm, ideal, want)


# ---- the file ----
def header(k=32, h=3, strand=1, m=1024, ins=12345, reserved=512):
    return _abi.NtcBloomHeader(k=k, n_hash=h, strand=strand, reserved=reserved, m_bits=m, n_inserted=ins)


def test_file_round_trip_and_damage(tmp_path):
    lib = L()
    rng = np.random.default_rng(3)
    for m in (512, 3 * 512, 1000 * 512):
        img = rng.integers(0, 256, size=m // 8, dtype=np.uint8)
        path = tmp_path / f"f{m}.bbf"
        assert lib.ntc_bbloom_write(str(path).encode(), C.byref(header(m=m)), ptr(img)) == 0
        assert not os.path.exists(str(path) + ".part")
        raw = path.read_bytes()
        assert raw[:8] == b"NTCBB1\0\0" and len(raw) == 40 + img.size and raw[40:] == img.tobytes()
        assert np.frombuffer(raw[8:24], dtype="<u4").tolist() == [32, 3, 1, 512] and np.frombuffer(raw[24:40], dtype="<u8").tolist() == [m, 12345]
        h = _abi.NtcBloomHeader()
        assert lib.ntc_bbloom_read(str(path).encode(), C.byref(h), None, 0) == 0  # the header alone
        assert (h.k, h.n_hash, h.strand, h.reserved, h.m_bits, h.n_inserted) == (32, 3, 1, 512, m, 12345)
        back = np.zeros(img.size + 3, dtype=np.uint8)
        assert lib.ntc_bbloom_read(str(path).encode(), C.byref(h), ptr(back), back.size) == 0
        assert np.array_equal(back[: img.size], img) and not back[img.size:].any()
        small = np.zeros(img.size - 1, dtype=np.uint8)
        h2 = _abi.NtcBloomHeader()
        assert lib.ntc_bbloom_read(str(path).encode(), C.byref(h2), ptr(small), small.size) == ERR_ARG and h2.m_bits == m and not small.any()
        # the three kinds do not read one another's files
        assert lib.ntc_bloom_read(str(path).encode(), C.byref(h2), None, 0) == ERR_ARG and lib.ntc_cbloom_read(str(path).encode(), C.byref(h2), None, 0) == ERR_ARG
    from ntcard_amd import bloom
    hd, image = bloom.read_blocked_file(path)
    assert hd == {"k": 32, "n_hash": 3, "strand": "forward", "m_bits": m, "n_inserted": 12345, "block_bits": 512} and np.array_equal(image, img)
    # damage: cut short, too long, wrong magic, reserved != 512, m_bits no multiple of 512 (with a body of that many bits: only the header is wrong)
    m520 = b"NTCBB1\0\0" + raw[8:24] + np.array([520, 1], dtype="<u8").tobytes() + b"\0" * 65
    for name, data in (("cut", raw[:-1]), ("cut_header", raw[:39]), ("cut_magic", raw[:5]), ("grown", raw + b"\0"), ("plain_magic", b"NTCBF1\0\0" + raw[8:]),
                       ("counting_magic", b"NTCCB1\0\0" + raw[8:]), ("empty", b""), ("k0", raw[:8] + b"\0\0\0\0" + raw[12:]),
                       ("hash33", raw[:12] + b"\x21\0\0\0" + raw[16:]), ("strand3", raw[:16] + b"\x03\0\0\0" + raw[20:]),
                       ("reserved0", raw[:20] + b"\0\0\0\0" + raw[24:]), ("reserved256", raw[:20] + b"\0\x01\0\0" + raw[24:]),
                       ("reserved1024", raw[:20] + b"\0\x04\0\0" + raw[24:]), ("m0", raw[:24] + b"\0" * 8 + raw[32:]), ("m520", m520),
                       ("mhuge", raw[:24] + b"\xff" * 8 + raw[32:])):
        p = tmp_path / f"bad_{name}.bbf"
        p.write_bytes(data)
        h = header(k=99)
        assert lib.ntc_bbloom_read(str(p).encode(), C.byref(h), None, 0) == ERR_ARG and h.k == 99, name
    # a plain filter's file of a legal blocked size is still no blocked file
    plain = tmp_path / "plain.bf"
    assert lib.ntc_bloom_write(str(plain).encode(), C.byref(header(m=1024, reserved=0)), ptr(np.zeros(128, dtype=np.uint8))) == 0
    assert lib.ntc_bbloom_read(str(plain).encode(), C.byref(h), None, 0) == ERR_ARG and b"is not a blocked filter file" in lib.ntc_last_error()
    assert lib.ntc_bbloom_read(str(tmp_path / "none.bbf").encode(), C.byref(h), None, 0) == ERR_ARG
    assert lib.ntc_bbloom_read(None, C.byref(h), None, 0) == ERR_ARG and lib.ntc_bbloom_read(str(path).encode(), None, None, 0) == ERR_ARG


def test_file_write_refusals_leave_nothing_behind(tmp_path):
    lib = L()
    img = np.zeros(128, dtype=np.uint8)
    out = tmp_path / "x.bbf"
    for h in (header(k=0), header(k=lib.ntc_max_k() + 1), header(h=0), header(h=33), header(strand=3), header(m=0), header(m=1 << 40), header(reserved=0),
              header(reserved=256), header(m=520), header(m=64), header(m=512 + 64)):
        assert lib.ntc_bbloom_write(str(out).encode(), C.byref(h), ptr(img)) == ERR_ARG and b"512" in lib.ntc_last_error()
    assert lib.ntc_bbloom_write(None, C.byref(header()), ptr(img)) == ERR_ARG
    assert lib.ntc_bbloom_write(str(out).encode(), None, ptr(img)) == ERR_ARG
    assert lib.ntc_bbloom_write(str(out).encode(), C.byref(header()), None) == ERR_ARG
    assert os.listdir(tmp_path) == []
    os.mkdir(out)
    assert lib.ntc_bbloom_write(str(out).encode(), C.byref(header()), ptr(img)) == ERR_ARG and b"cannot write" in lib.ntc_last_error()
    assert os.path.isdir(out) and not os.path.exists(str(out) + ".part")
    assert lib.ntc_bbloom_write(str(tmp_path / "no" / "x.bbf").encode(), C.byref(header()), ptr(img)) == ERR_ARG
    # an existing file is replaced only by a whole one
    good = tmp_path / "y.bbf"
    assert lib.ntc_bbloom_write(str(good).encode(), C.byref(header()), ptr(img)) == 0
    first = good.read_bytes()
    assert lib.ntc_bbloom_write(str(good).encode(), C.byref(header(m=520)), ptr(img)) == ERR_ARG and good.read_bytes() == first
    # the plain and the counting writers still insist on reserved == 0
    assert lib.ntc_bloom_write(str(tmp_path / "z.bf").encode(), C.byref(header()), ptr(img)) == ERR_ARG
    assert lib.ntc_cbloom_write(str(tmp_path / "z.cbf").encode(), C.byref(header()), ptr(img)) == ERR_ARG
