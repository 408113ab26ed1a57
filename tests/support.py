"""What the tests share, host side: paths, read and mask generators, ntComp (ntcard.cpp:132-145), the row-slot and tiled layouts, the comparison with the
oracle, the command-line runner, the helpers of the Bloom filters' tests and the helpers of the C-ABI tests.  One definition each; tests/test_support.py pins them to tests/orc.py and to
ntcard_amd.tile_reads.  numpy, ctypes and the oracle only: torch is never imported here (tests/gpu_support.py holds what needs a device)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NTCARD = os.path.join(ROOT, "ntcard_amd", "bin", "ntcard")
NTHLL = os.path.join(ROOT, "ntcard_amd", "bin", "nthll")
NTSIG = os.path.join(ROOT, "ntcard_amd", "bin", "ntsig")
NTBLOOM = os.path.join(ROOT, "ntcard_amd", "bin", "ntbloom")

ALPHA = np.frombuffer(b"ACGTacgtUuNnRYKM.-*", dtype=np.uint8)  # random_reads: the first four are the clean draw, the rest the non-base one
TILE = 2048
ERR_ARG, ERR_DEVICE = -1, -2
FAKE = 0x10000  # a pointer that is never followed: every call that gets it is refused before it could be
LETTERS = b"ACGTUacgtu"  # rand_seq: the bases, and what it draws instead of one
BAD = b"NNNnRYKM"


# ---- reads ----
def small_reads():
    """the sequence lines of golden/reads_small.fq.gz"""
    with gzip.open(os.path.join(GOLD, "reads_small.fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    return [lines[i] for i in range(1, len(lines) - 1, 4)]


def rseq(rng, n, pn=0.0, plow=0.1, bad="NnRY-"):
    """n bytes from a random.Random: a byte of `bad` with probability pn, a lower-case base with plow, else an upper-case one (two draws per byte)"""
    out = []
    for _ in range(n):
        r = rng.random()
        if r < pn:
            out.append(rng.choice(bad))
        elif r < pn + plow:
            out.append(rng.choice("acgtu"))
        else:
            out.append(rng.choice("ACGTU"))
    return "".join(out).encode()


def rseq_acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def rand_seq(rng, n, pn=0.0):
    """n bytes from a random.Random: a byte of BAD with probability pn, else one of LETTERS (one draw per byte where pn is 0)"""
    return bytes(rng.choice(BAD) if pn and rng.random() < pn else rng.choice(LETTERS) for _ in range(n))


def random_reads(rng, n, L, p_bad, alpha=ALPHA):
    """(n, L) uint8 reads from a numpy Generator: alpha[:4], with probability p_bad a byte of alpha[4:] instead"""
    arr = alpha[rng.integers(0, 4, size=(n, L))]
    if p_bad:
        arr = np.where(rng.random((n, L)) < p_bad, alpha[rng.integers(4, len(alpha), size=(n, L))], arr).astype(np.uint8)
    return np.ascontiguousarray(arr)


# ---- masks ----
def mask_with(k, zeros):
    m = ["1"] * k
    for i in zeros:
        m[i] = "0"
    return "".join(m)


# masks of every shape the kernel distinguishes, per span: one interior run, several runs, runs touching offset 0, offset k-1 and both,
# a single '0', alternating 0101...1 (more toggle pairs than the rolling form takes), a single '1', and all '1' (plain k)
def masks_for(k):
    if k == 1:
        return ["1"]
    out = {"1" * k, mask_with(k, [k // 2]), "1" * (k - 1) + "0", "0" + "1" * (k - 1), ("01" * k)[:k - 1] + "1", "0" * (k - 1) + "1"}
    if k >= 4:
        out.add(mask_with(k, range(k // 4, k // 2)))                          # one interior run
        out.add(mask_with(k, list(range(0, k // 4)) + [k - 1]))               # runs at both ends
        out.add(mask_with(k, list(range(1, 2)) + list(range(k // 2, k // 2 + 2)) + [k - 2]))  # several runs
    return sorted(out)


def gap_mask(k, gap):
    """ntcard's one seed under -g (ntcard.cpp:407-413); gap 0: plain k-mers"""
    return "1" * ((k - gap) // 2) + "0" * gap + "1" * (k - gap - (k - gap) // 2)


# ---- ntComp (ntcard.cpp:132-145) ----
def nt_comp(h, r_bits, s_bits):
    """uint64 values -> (sample, index): sample 0 where (h >> (63 - s)) == 1, sample 1 where (h >> (64 - s)) == 2^(s-1) - 1 (it wins where both
    hold), 2 where the value is not sampled; index = the low r_bits bits"""
    h = np.asarray(h, dtype=np.uint64)
    s0 = (h >> np.uint64(63 - s_bits)) == np.uint64(1)
    s1 = (h >> np.uint64(64 - s_bits)) == np.uint64((1 << (s_bits - 1)) - 1)
    return np.where(s1, 1, np.where(s0, 0, 2)), (h & np.uint64((1 << r_bits) - 1)).astype(np.int64)


def sampled(h, s_bits):
    return nt_comp(h, 0, s_bits)[0] < 2


def key_of(h, r_bits, s_bits):
    """one value -> its counter index within the plane (sample * 2^r_bits + index), or None"""
    sample, index = nt_comp(np.array([h], dtype=np.uint64), r_bits, s_bits)
    return None if sample[0] == 2 else (int(sample[0]) << r_bits) + int(index[0])


def sketch_from_values(values_per_plane, r_bits, s_bits):
    """-> t_Counter [n][2][1 << r_bits] (uint16, as the engine reports it), F1 [n] = the number of values of every plane"""
    tc = np.zeros((len(values_per_plane), 2, 1 << r_bits), dtype=np.uint16)
    f1 = np.zeros(len(values_per_plane), dtype=np.uint64)
    for i, h in enumerate(values_per_plane):
        f1[i] = h.size
        sample, index = nt_comp(h, r_bits, s_bits)
        keep = sample < 2
        np.add.at(tc[i], (sample[keep], index[keep]), np.uint16(1))
    return tc, f1


# ---- layouts ----
def to_slots(reads, stride, fill=ord("A"), tail=16):
    """row slots: read i from byte i * stride on, `fill` behind its end and in the `tail` bytes behind the last slot"""
    buf = np.full(len(reads) * stride + tail, fill, dtype=np.uint8)
    for i, r in enumerate(reads):
        buf[i * stride: i * stride + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return buf


def tile_array(arr):
    """(n, L) uint8 array of reads -> tiled layout: tile t, chunk c, read r, 16 bytes (include/ntcard_hip.h: ntc_submit_tiled_device)"""
    n, L = arr.shape
    C16, ntl = (L + 15) // 16, (n + TILE - 1) // TILE
    a = np.full((ntl * TILE, C16 * 16), ord("A"), dtype=np.uint8)
    a[:n, :L] = arr
    return np.ascontiguousarray(a.reshape(ntl, TILE, C16, 16).transpose(0, 2, 1, 3)).reshape(-1)


def tile(reads, read_len, unused=ord("A")):
    """reads (list of bytes, none longer than 16 ceil(read_len / 16)) -> the tiled layout; bytes behind a read's end hold 'A' (the ABI asks for a base
    letter there), the slots behind the batch's last read hold `unused`"""
    n = len(reads)
    a = np.full(((n + TILE - 1) // TILE * TILE, (read_len + 15) // 16 * 16), ord("A"), dtype=np.uint8)
    a[n:] = unused
    for i, r in enumerate(reads):
        a[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    return tile_array(a)


def tile_ragged(reads, n_chunks):
    """one bin of a ragged read set (reads of 16 n_chunks - 15 .. 16 n_chunks bases) -> (tiles uint8, tails uint32 [n_tiles, 16]): every tile sorted longest
    read first, tails[t, d] = the reads of tile t with more than d bases in their last piece (include/ntcard_hip.h: ntc_submit_tiled_ragged_device)"""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    assert lens.size and lens.min() > 16 * (n_chunks - 1) and lens.max() <= 16 * n_chunks
    order = np.argsort(-lens, kind="stable")
    tiles = tile([reads[i] for i in order], 16 * n_chunks)
    last = np.full((len(reads) + TILE - 1) // TILE * TILE, 0, dtype=np.int64)
    last[:lens.size] = lens[order] - 16 * (n_chunks - 1)
    tails = (last.reshape(-1, TILE, 1) > np.arange(16).reshape(1, 1, 16)).sum(axis=1).astype(np.uint32)
    return tiles, tails


def spans_of(reads, lead=5, gap=3, fill=ord("#")):
    """reads as spans of one host buffer, `gap` bytes of `fill` between them (ntc_submit_spans) -> (buf uint8, starts uint64, lens uint32)"""
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    starts = lead + np.concatenate([[0], np.cumsum(lens[:-1].astype(np.uint64) + np.uint64(gap))]).astype(np.uint64)
    buf = np.full(int(starts[-1]) + int(lens[-1]) + gap, fill, dtype=np.uint8)
    for s, r in zip(starts.tolist(), reads):
        buf[s:s + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return buf, starts, lens


def offsets_of(lens_or_seqs, lead=0):
    """uint64 offsets [n + 1] of sequences (or of their lengths) laid behind one another, the first one at `lead`"""
    lens = lens_or_seqs if isinstance(lens_or_seqs, np.ndarray) else [x if isinstance(x, (int, np.integer)) else len(x) for x in lens_or_seqs]
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum(lens, dtype=np.uint64)
    return offs


# ---- the comparison with the oracle ----
def oracle_counts(arr_or_reads, klist, gap=0, r_bits=16, s_bits=7):
    """tests/orc.py over an (n, L) array of equal-length reads or over a list of reads -> (t_Counter, F1)"""
    if isinstance(arr_or_reads, np.ndarray):
        n, L = arr_or_reads.shape
        counters = np.zeros((len(klist), 2, 1 << r_bits), dtype=np.uint16)
        f1 = orc.sketch_update(counters, np.ascontiguousarray(arr_or_reads).reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(L), list(klist), gap,
                               r_bits, s_bits)
        return counters, f1
    return orc.sketch_reads(list(arr_or_reads), list(klist), gap, r_bits, s_bits)


def same_sketch(got, want):
    """(t_Counter, F1) against (t_Counter, F1) -> bool"""
    return np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def assert_same_sketch(got, want, what, nonempty=False, hist_r_bits=None):
    """got: (t_Counter, F1) or what finish(counters=True) returns, (t_Counter, histograms, F1); want: the oracle's (t_Counter, F1).  nonempty: every
    plane of the oracle counted something; hist_r_bits: the value histograms are those of the oracle's counters too"""
    tc, f1, (oc, of1) = got[0], got[-1], want
    off = int((tc != oc).sum()) if tc.shape == oc.shape else "another shape"
    print(what, "F1", np.asarray(f1).tolist(), "oracle", np.asarray(of1).tolist(), "counters off", off)
    if nonempty:
        assert of1.all(), "the oracle counted nothing"
    assert np.array_equal(f1, of1), (what, f1, of1)
    assert np.array_equal(tc, oc), (what, off)
    if hist_r_bits is not None:
        for ki in range(oc.shape[0]):
            assert np.array_equal(got[1][ki], orc.value_hist(oc[ki], hist_r_bits)), what


# ---- command lines ----
def run_cli(binary, args, cwd=None, timeout=60, text=False):
    """binary + args with both streams captured; text: str instead of bytes"""
    return subprocess.run([binary] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=text)


# ---- ntbloom (the Bloom filters' command-line tests) ----
def run(args, cwd):
    return run_cli(NTBLOOM, args, cwd=cwd, timeout=120)


def swap(args, flag, value):
    out = list(args)
    out[out.index(flag) + 1] = value
    return out


def without(args, flag):
    i = args.index(flag)
    return args[:i] + args[i + 2:]


def fastq(seqs, prefix=b"q"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (prefix, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def rows_of(stdout):
    lines = stdout.decode().splitlines()
    assert lines[0] == "name\tlength\twindows\thits\tfraction"
    return [line.split("\t") for line in lines[1:]]


# ---- the C ABI ----
def L():
    from ntcard_amd import _abi
    return _abi.lib()


def offs(*v):
    return np.array(v, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the C ABI's create calls ----
def abi_config(k=(32,), gap=0, flags=0, r_bits=14, s_bits=7, n_k=None):
    """an NtcConfig; k None: no k array (the seeded create), n_k: what the struct says where that is not len(k)"""
    from ntcard_amd import _abi
    c = _abi.NtcConfig(r_bits=r_bits, s_bits=s_bits, device=0, gap=gap, flags=flags)
    c.n_k = (len(k) if k is not None else 0) if n_k is None else n_k
    if k is not None:
        arr = (C.c_uint32 * len(k))(*k)
        c.k = C.cast(arr, C.POINTER(C.c_uint32))
        c._keep = arr
    return c


def hll_create_ex(k=None, seeds=None, n_bits=16, flags=0, n_k=None, n_seeds=None):
    """ntc_hll_create_ex over an NtcHllConfig of these lists (n_k, n_seeds: what the struct says where that is not their length) -> (rc, handle, library)"""
    from ntcard_amd import _abi
    L = _abi.lib()
    cfg = _abi.NtcHllConfig()
    keep = []
    if k is not None:
        arr = (C.c_uint32 * max(1, len(k)))(*k)
        keep.append(arr)
        cfg.k = C.cast(arr, C.POINTER(C.c_uint32))
    cfg.n_k = len(k) if n_k is None and k is not None else (n_k or 0)
    if seeds is not None:
        sarr = (C.c_char_p * max(1, len(seeds)))(*seeds)
        keep.append(sarr)
        cfg.seeds = C.cast(sarr, C.POINTER(C.c_char_p))
    cfg.n_seeds = len(seeds) if n_seeds is None and seeds is not None else (n_seeds or 0)
    cfg.n_bits, cfg.device, cfg.flags = n_bits, 0, flags
    h = C.c_void_p()
    return L.ntc_hll_create_ex(C.byref(cfg), C.byref(h)), h, L


def no_gpu():
    import torch
    return not torch.cuda.is_available()


def created(rc, h, L):
    """the call got past its argument checks: on a machine without a GPU it fails at the device probe, with one it makes an engine"""
    if h:
        L.ntc_destroy(h)
    assert rc == (ERR_DEVICE if no_gpu() else 0), (rc, L.ntc_last_error())
    return True
