"""Host tests of the counting Bloom filters (include/ntcard_hip.h: ntc_cbloom_*, ntc_bloom_insert_solid_device): the symbols, every refusal that comes
before a device is touched, the counting filter file, and the model of tests/cbloom_model.py pinned to tests/bloom_model.py — which is itself pinned to the
oracle and the reference's recorded rows (tests/test_bloom_host.py)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from ntcard_amd import _abi
from support import ERR_ARG, FAKE, GOLD, L, offs, ptr, rseq

M, H, K = (1 << 20) + 7, 3, 32
NAMES = ["ntc_cbloom_insert_device", "ntc_cbloom_query_device", "ntc_cbloom_profile_device", "ntc_cbloom_insert_hashes_device", "ntc_cbloom_query_hashes_device",
         "ntc_cbloom_threshold_device", "ntc_bloom_insert_solid_device", "ntc_cbloom_add_device", "ntc_cbloom_hist_device", "ntc_cbloom_write", "ntc_cbloom_read"]


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(os.path.dirname(GOLD), "..", "include", "ntcard_hip.h")).read()
    for n in NAMES:
        assert n in _abi.ABI_SYMBOLS and hasattr(L(), n) and n + "(" in text
    assert L().ntc_abi_version() == 6  # additive: the version stays
    import ntcard_amd
    from ntcard_amd import bloom
    assert ntcard_amd.CountingBloomFilter is bloom.CountingBloomFilter and callable(bloom.read_counting_file)


# ---- the model ----
def mixed(rng, k):
    return [rseq(rng, n, pn=0.02) for n in (0, 1, k - 1, k, k + 1, 90, 200, 333)] + [b"", b"ACGTUacgtu" * 7]


@pytest.mark.parametrize("strand", [sm.CANONICAL, sm.FORWARD, sm.REVERSE])
def test_model_thresholded_at_one_is_the_pinned_image(strand):
    rng = random.Random(3)
    for k in (1, 31, 32, 33):
        seqs = mixed(rng, k)
        for m in (7, 64, 4099):
            cnt, n = cm.counters(seqs, k, strand, H, m)
            img, n_img = bm.build(seqs, k, strand, H, m)
            assert n == n_img and n > 0 and cnt.dtype == np.uint8 and cnt.size == m
            assert np.array_equal(cm.threshold(cnt, 1), img)
            assert int(cnt.astype(np.int64).sum()) == H * n or (cnt == 255).any()  # every increment is there unless a counter saturated
            w, h = cm.query(cnt, seqs, k, strand, H, 1)
            bw, bh = bm.query(img, seqs, k, strand, H, m)
            assert np.array_equal(w, bw) and np.array_equal(h, bh)


def test_model_counts_a_duplicate_position_twice():
    h0 = np.array([5, 77, 2**63 + 12345], dtype=np.uint64)
    assert cm.counters_of(h0, H, K, 1).tolist() == [9]  # m = 1: all three positions of every value are counter 0
    pos = bm.positions(h0, H, K, 2)
    assert any(len(set(row)) < H for row in pos.tolist())  # m = 2, three positions: two coincide
    cnt = cm.counters_of(h0, H, K, 2)
    assert cnt.tolist() == [int((pos == 0).sum()), int((pos == 1).sum())] and int(cnt.sum()) == 9
    assert cm.counters_of(np.repeat(h0, 100), H, K, 1).tolist() == [255]  # 900 increments saturate
    assert cm.counts(cnt, h0, H, K).tolist() == [min(int(cnt[p]) for p in row) for row in pos.tolist()]


def test_model_merge_is_the_model_of_the_concatenated_input():
    rng = random.Random(4)
    k, m = 32, 61
    a, b = mixed(rng, k), [b"A" * 400] + mixed(rng, k)
    ca, na = cm.counters(a, k, sm.CANONICAL, H, m)
    cb, nb = cm.counters(b, k, sm.CANONICAL, H, m)
    whole, n = cm.counters(a + b, k, sm.CANONICAL, H, m)
    assert n == na + nb and (whole == 255).any() and (whole < 255).any()
    assert np.array_equal(cm.merge(ca, cb), whole)
    assert np.array_equal(cm.counters(b, k, sm.CANONICAL, H, m, into=ca)[0], whole)
    assert np.array_equal(cm.hist(whole), np.bincount(whole, minlength=256)) and int(cm.hist(whole).sum()) == m


def test_model_profile_and_solid_values():
    k, m = 4, 257
    seqs = [b"ACGTACGTNACGTA", b"ACG", b"", b"ACGTAC"]
    cnt, n = cm.counters(seqs, k, sm.FORWARD, H, m)
    assert n == 5 + 2 + 3
    prof = cm.profile(cnt, seqs, k, sm.FORWARD, H)
    assert prof.size == 14 + 3 + 6
    starts = [0, 1, 2, 3, 4, 9, 10, 17, 18, 19]
    assert np.nonzero(prof)[0].tolist() == starts
    # ACGT starts at 0, 4, 9 and 17, CGTA at 1 and 10: counted so often at least
    assert prof[0] == prof[4] == prof[9] == prof[17] >= 4 and prof[1] == prof[10] >= 2 and prof[1] == prof[18]
    v = cm.all_values(seqs, k, sm.FORWARD)
    assert np.array_equal(cm.solid_values(cnt, seqs, k, sm.FORWARD, H, 1), v)
    uniq, true = np.unique(v, return_counts=True)
    s4 = cm.solid_values(cnt, seqs, k, sm.FORWARD, H, 4)
    assert set(uniq[true >= 4].tolist()) <= set(s4.tolist()) and 4 <= s4.size < v.size


# ---- refusals before the device ----
# (what is wrong, counters, m, n_hash, k): the checks every counting-filter call shares
BAD_COUNTERS = [
    ("null counters", None, M, H, K),
    ("misaligned counters", FAKE + 2, M, H, K),
    ("m 0", FAKE, 0, H, K),
    ("m 2^40", FAKE, 1 << 40, H, K),
    ("n_hash 0", FAKE, M, 0, K),
    ("n_hash 33", FAKE, M, 33, K),
    ("k 0", FAKE, M, H, 0),
    ("k too large", FAKE, M, H, None),
]


@pytest.mark.parametrize("what,cnt,m,h,k", BAD_COUNTERS, ids=[b[0] for b in BAD_COUNTERS])
def test_bad_counter_arguments_are_refused_before_the_device(what, cnt, m, h, k):
    lib = L()
    k = lib.ntc_max_k() + 1 if k is None else k
    o = offs(0, 40)
    n = C.c_uint64(77)
    assert lib.ntc_cbloom_insert_device(0, None, cnt, m, h, k, 0, FAKE, ptr(o), 1, C.byref(n)) == ERR_ARG and n.value == 77
    assert lib.ntc_last_error()
    assert lib.ntc_cbloom_query_device(0, None, cnt, m, h, k, 0, FAKE, ptr(o), 1, 1, FAKE, FAKE) == ERR_ARG
    assert lib.ntc_cbloom_profile_device(0, None, cnt, m, h, k, 0, FAKE, ptr(o), 1, FAKE) == ERR_ARG
    assert lib.ntc_cbloom_insert_hashes_device(0, None, cnt, m, h, k, FAKE, 4) == ERR_ARG
    assert lib.ntc_cbloom_query_hashes_device(0, None, cnt, m, h, k, FAKE, 4, FAKE) == ERR_ARG
    assert lib.ntc_bloom_insert_solid_device(0, None, FAKE, M, H, cnt, m, h, 2, k, 0, FAKE, ptr(o), 1, C.byref(n)) == ERR_ARG and n.value == 77
    if what.split()[0] in ("null", "misaligned", "m"):
        hist = np.full(256, 5, dtype=np.uint64)
        assert lib.ntc_cbloom_hist_device(0, None, cnt, m, ptr(hist)) == ERR_ARG and (hist == 5).all()
        assert lib.ntc_cbloom_add_device(0, None, cnt, FAKE + 64, m) == ERR_ARG
        assert lib.ntc_cbloom_add_device(0, None, FAKE + 64, cnt, m) == ERR_ARG
        assert lib.ntc_cbloom_threshold_device(0, None, cnt, m, 1, FAKE + 64) == ERR_ARG


def test_bad_input_and_output_arguments_are_refused_before_the_device():
    lib = L()
    n = C.c_uint64(77)
    good = offs(5, 45, 45, 90)
    down = offs(5, 45, 44, 90)
    for strand in (3, 1 << 31):
        assert lib.ntc_cbloom_insert_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG and b"strand" in lib.ntc_last_error()
        assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, 1, FAKE, FAKE) == ERR_ARG
        assert lib.ntc_cbloom_profile_device(0, None, FAKE, M, H, K, strand, FAKE, ptr(good), 3, FAKE) == ERR_ARG
        assert lib.ntc_bloom_insert_solid_device(0, None, FAKE, M, H, FAKE, M, H, 2, K, strand, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG
    for bases, o, word in ((FAKE, None, b"offsets"), (FAKE, down, b"sequence 1"), (None, good, b"bases")):
        op = ptr(o) if o is not None else None
        assert lib.ntc_cbloom_insert_device(0, None, FAKE, M, H, K, 0, bases, op, 3, C.byref(n)) == ERR_ARG and word in lib.ntc_last_error()
        assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, 0, bases, op, 3, 1, FAKE, FAKE) == ERR_ARG and word in lib.ntc_last_error()
        assert lib.ntc_cbloom_profile_device(0, None, FAKE, M, H, K, 0, bases, op, 3, FAKE) == ERR_ARG and word in lib.ntc_last_error()
        assert lib.ntc_bloom_insert_solid_device(0, None, FAKE, M, H, FAKE, M, H, 2, K, 0, bases, op, 3, C.byref(n)) == ERR_ARG and word in lib.ntc_last_error()
    # min_count is 1 .. 255
    for c in (0, 256, 1 << 31):
        assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, c, FAKE, FAKE) == ERR_ARG and b"min_count" in lib.ntc_last_error()
        assert lib.ntc_cbloom_threshold_device(0, None, FAKE, M, c, FAKE + 64) == ERR_ARG and b"min_count" in lib.ntc_last_error()
        assert lib.ntc_bloom_insert_solid_device(0, None, FAKE, M, H, FAKE, M, H, c, K, 0, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG and b"min_count" in lib.ntc_last_error()
    # outputs, hashes, the second array
    assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, 1, None, FAKE) == ERR_ARG and b"output" in lib.ntc_last_error()
    assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, 1, FAKE, None) == ERR_ARG
    assert lib.ntc_cbloom_profile_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(good), 3, None) == ERR_ARG and b"output" in lib.ntc_last_error()
    assert lib.ntc_cbloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 4) == ERR_ARG
    assert lib.ntc_cbloom_insert_hashes_device(0, None, FAKE, M, H, K, FAKE + 4, 4) == ERR_ARG and b"8-byte" in lib.ntc_last_error()
    assert lib.ntc_cbloom_query_hashes_device(0, None, FAKE, M, H, K, None, 4, FAKE) == ERR_ARG
    assert lib.ntc_cbloom_query_hashes_device(0, None, FAKE, M, H, K, FAKE, 4, None) == ERR_ARG
    assert lib.ntc_cbloom_hist_device(0, None, FAKE, M, None) == ERR_ARG
    assert lib.ntc_cbloom_threshold_device(0, None, FAKE, M, 1, None) == ERR_ARG
    assert lib.ntc_cbloom_threshold_device(0, None, FAKE, M, 1, FAKE + 2) == ERR_ARG
    assert lib.ntc_cbloom_add_device(0, None, FAKE, FAKE, M) == ERR_ARG and b"same array" in lib.ntc_last_error()
    # the plain filter of the solid insert: its own checks
    for filt, mb, h in ((None, M, H), (FAKE + 1, M, H), (FAKE, 0, H), (FAKE, 1 << 40, H), (FAKE, M, 0), (FAKE, M, 33)):
        assert lib.ntc_bloom_insert_solid_device(0, None, filt, mb, h, FAKE, M, H, 2, K, 0, FAKE, ptr(good), 3, C.byref(n)) == ERR_ARG
    assert n.value == 77


def test_calls_without_work_need_no_device():
    lib = L()
    n = C.c_uint64(77)
    short = offs(3, 10, 10, 20)  # 17 bytes in all: no window of 32
    assert lib.ntc_cbloom_insert_device(0, None, FAKE, M, H, K, 0, FAKE, ptr(short), 3, C.byref(n)) == 0 and n.value == 0
    n.value = 77
    assert lib.ntc_bloom_insert_solid_device(0, None, FAKE, M, H, FAKE, M, H, 2, K, 0, FAKE, ptr(short), 3, C.byref(n)) == 0 and n.value == 0
    assert lib.ntc_cbloom_insert_hashes_device(0, None, FAKE, M, H, K, None, 0) == 0
    assert lib.ntc_cbloom_query_hashes_device(0, None, FAKE, M, H, K, None, 0, None) == 0
    assert lib.ntc_cbloom_query_device(0, None, FAKE, M, H, K, 0, None, ptr(offs(9)), 0, 1, None, None) == 0
    assert lib.ntc_cbloom_profile_device(0, None, FAKE, M, H, K, 0, None, ptr(offs(9, 9)), 1, None) == 0  # no position: nothing to write


# ---- the file ----
def header(k=32, h=3, strand=1, m=77, ins=12345, reserved=0):
    return _abi.NtcBloomHeader(k=k, n_hash=h, strand=strand, reserved=reserved, m_bits=m, n_inserted=ins)


def test_file_round_trip_and_damage(tmp_path):
    lib = L()
    rng = np.random.default_rng(3)
    for m in (1, 8, 77, 4093, (1 << 20) + 7):
        cnt = rng.integers(0, 256, size=m, dtype=np.uint8)
        path = tmp_path / f"f{m}.cbf"
        assert lib.ntc_cbloom_write(str(path).encode(), C.byref(header(m=m)), ptr(cnt)) == 0
        assert not os.path.exists(str(path) + ".part")
        raw = path.read_bytes()
        assert raw[:8] == b"NTCCB1\0\0" and len(raw) == 40 + m and raw[40:] == cnt.tobytes()
        assert np.frombuffer(raw[8:24], dtype="<u4").tolist() == [32, 3, 1, 0] and np.frombuffer(raw[24:40], dtype="<u8").tolist() == [m, 12345]
        h = _abi.NtcBloomHeader()
        assert lib.ntc_cbloom_read(str(path).encode(), C.byref(h), None, 0) == 0  # the size query: the header alone
        assert (h.k, h.n_hash, h.strand, h.reserved, h.m_bits, h.n_inserted) == (32, 3, 1, 0, m, 12345)
        back = np.zeros(m + 3, dtype=np.uint8)
        assert lib.ntc_cbloom_read(str(path).encode(), C.byref(h), ptr(back), back.size) == 0
        assert np.array_equal(back[:m], cnt) and not back[m:].any()
        if m > 1:
            small = np.zeros(m - 1, dtype=np.uint8)
            h2 = _abi.NtcBloomHeader()
            assert lib.ntc_cbloom_read(str(path).encode(), C.byref(h2), ptr(small), small.size) == ERR_ARG and h2.m_bits == m and not small.any()
    from ntcard_amd import bloom
    hd, image = bloom.read_counting_file(path)
    assert hd == {"k": 32, "n_hash": 3, "strand": "forward", "m_bits": m, "n_inserted": 12345} and np.array_equal(image, cnt)
    for name, data in (("cut", raw[:-1]), ("cut_header", raw[:39]), ("cut_magic", raw[:5]), ("grown", raw + b"\0"), ("magic", b"NTCSIG1\0" + raw[8:]),
                       ("empty", b""), ("k0", raw[:8] + b"\0\0\0\0" + raw[12:]), ("hash33", raw[:12] + b"\x21\0\0\0" + raw[16:]),
                       ("strand3", raw[:16] + b"\x03\0\0\0" + raw[20:]), ("reserved", raw[:20] + b"\x01\0\0\0" + raw[24:]),
                       ("m0", raw[:24] + b"\0" * 8 + raw[32:]), ("mhuge", raw[:24] + b"\xff" * 8 + raw[32:])):
        p = tmp_path / f"bad_{name}.cbf"
        p.write_bytes(data)
        h = header(k=99)
        assert lib.ntc_cbloom_read(str(p).encode(), C.byref(h), None, 0) == ERR_ARG and h.k == 99, name
    assert lib.ntc_cbloom_read(str(tmp_path / "none.cbf").encode(), C.byref(h), None, 0) == ERR_ARG
    assert lib.ntc_cbloom_read(None, C.byref(h), None, 0) == ERR_ARG and lib.ntc_cbloom_read(str(path).encode(), None, None, 0) == ERR_ARG


def test_the_two_kinds_of_file_are_told_apart(tmp_path):
    lib = L()
    m = 64  # 64 counters are 64 bytes, 64 bits are 8
    data = np.arange(64, dtype=np.uint8)
    bf, cbf = tmp_path / "x.bf", tmp_path / "x.cbf"
    assert lib.ntc_bloom_write(str(bf).encode(), C.byref(header(m=m)), ptr(data)) == 0
    assert lib.ntc_cbloom_write(str(cbf).encode(), C.byref(header(m=m)), ptr(data)) == 0
    assert len(bf.read_bytes()) == 40 + 8 and len(cbf.read_bytes()) == 40 + 64
    h = header(k=99)
    assert lib.ntc_cbloom_read(str(bf).encode(), C.byref(h), None, 0) == ERR_ARG and b"is not a counting filter file" in lib.ntc_last_error() and h.k == 99
    assert lib.ntc_bloom_read(str(cbf).encode(), C.byref(h), None, 0) == ERR_ARG and b"is not a filter file" in lib.ntc_last_error() and h.k == 99
    # a counting file under the plain magic has the wrong length for its header, and the reverse
    swapped = tmp_path / "swapped.bf"
    swapped.write_bytes(b"NTCBF1\0\0" + cbf.read_bytes()[8:])
    assert lib.ntc_bloom_read(str(swapped).encode(), C.byref(h), None, 0) == ERR_ARG and h.k == 99
    swapped.write_bytes(b"NTCCB1\0\0" + bf.read_bytes()[8:])
    assert lib.ntc_cbloom_read(str(swapped).encode(), C.byref(h), None, 0) == ERR_ARG and b"cut short" in lib.ntc_last_error() and h.k == 99


def test_file_write_refusals_leave_nothing_behind(tmp_path):
    lib = L()
    cnt = np.zeros(128, dtype=np.uint8)
    out = tmp_path / "x.cbf"
    for h in (header(k=0), header(k=lib.ntc_max_k() + 1), header(h=0), header(h=33), header(strand=3), header(m=0), header(m=1 << 40), header(reserved=1)):
        assert lib.ntc_cbloom_write(str(out).encode(), C.byref(h), ptr(cnt)) == ERR_ARG
    assert lib.ntc_cbloom_write(None, C.byref(header()), ptr(cnt)) == ERR_ARG
    assert lib.ntc_cbloom_write(str(out).encode(), None, ptr(cnt)) == ERR_ARG
    assert lib.ntc_cbloom_write(str(out).encode(), C.byref(header()), None) == ERR_ARG
    assert os.listdir(tmp_path) == []
    os.mkdir(out)  # a target that cannot be written: refused, no .part left
    assert lib.ntc_cbloom_write(str(out).encode(), C.byref(header()), ptr(cnt)) == ERR_ARG and b"cannot write" in lib.ntc_last_error()
    assert os.path.isdir(out) and not os.path.exists(str(out) + ".part")
    assert lib.ntc_cbloom_write(str(tmp_path / "no" / "x.cbf").encode(), C.byref(header()), ptr(cnt)) == ERR_ARG
    good = tmp_path / "y.cbf"  # an existing file is replaced only by a whole one
    assert lib.ntc_cbloom_write(str(good).encode(), C.byref(header(m=128)), ptr(cnt)) == 0
    first = good.read_bytes()
    assert lib.ntc_cbloom_write(str(good).encode(), C.byref(header(m=0)), ptr(cnt)) == ERR_ARG and good.read_bytes() == first
