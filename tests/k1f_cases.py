"""k1f_cases.py — deterministic inputs for the fix-up kernels K1f (ntcard_amd/csrc/ntc_sketch_k1h.hip: the F1 role and the suspect role of
k1h_fix_kernel, k1h_slow_kernel).  Test infrastructure only: numpy, the oracle and the K1h model; neither torch nor a GPU.

What K1f decides depends on the window's offset in its first 16-byte piece, on which of the pieces c0 .. c0 + 2 the window reaches and which of
them are dirty, on whether the suspect is a tie, and on where exactly the non-base byte lies.  Random placement visits those combinations by
chance; the families here visit each of them on purpose.  Every family is a batch of 2049 + a few reads (it crosses a tile boundary, its last
tile is partial), filled up with plain random reads, and everything derives from fixed seeds.

Planted windows come from four pools per (k, sBits, gap) — `tie` (both strands flagged), `plain` (one strand flagged, sampled), `below`
(flagged by the 8-bit prefix, sampled by neither pattern: sBits >= 8) and `none` (not flagged).  A non-base byte INSIDE a planted window is a
"mimic" of the base it replaces: K1h packs a byte to the 2-bit code (byte >> 1) & 3 whatever it is, so H / K / D / N in the place of
A / C / T / G leave K1h's hash of the window as it was — the window still is a candidate, K1h hands it over as a suspect of a dirty piece, and
K1f alone decides that it must not count.
"""
import collections
import functools

import numpy as np

import k1h_model as km
import orc
from support import TILE, sampled, tile  # noqa: F401  (re-exported: kc.tile)

Case = collections.namedtuple("Case", "reads read_len k s_bits gap tails")

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MIMIC = {ord("A"): ord("H"), ord("C"): ord("K"), ord("T"): ord("D"), ord("G"): ord("N")}  # same (byte >> 1) & 3, no base
SLOT_BYTES = (1, 3, 4, 5, 7)  # bases to the reference's seed table, no letters to the packing kernels
FILL_TO = TILE + 1 + 3
POOL_MIN = 16
N = ord("N")


def _rand_read(rng, n):
    return bytearray(ACGT[rng.integers(0, 4, size=n)].tobytes())


def _filled(reads, rng, L):
    """the family's reads, then plain random ones up to 2049 + a few"""
    reads = [bytes(r) for r in reads]
    assert all(len(r) == L for r in reads)
    while len(reads) < FILL_TO:
        reads.append(bytes(_rand_read(rng, L)))
    assert TILE < len(reads) < 3 * TILE and len(reads) % TILE
    return reads


# ---- planted windows ----------------------------------------------------------------------------------------------------------------
def _strand_hashes(idx, k, gap):
    """forward and reverse ntHash of every window of a sequence given as indices into "ACGT" (the closed form, nthash.hpp:220-239; spaced seed: the
    don't-care positions left out)"""
    L = orc.lib()
    n = len(idx) - k + 1
    f, r = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(k):
        if gap and (k - gap) // 2 <= i < (k - gap) // 2 + gap:
            continue
        tf = np.array([L.orc_srol(L.orc_seed(b), k - 1 - i) for b in b"ACGT"], dtype=np.uint64)
        tr = np.array([L.orc_srol(L.orc_seed_comp(b), i) for b in b"ACGT"], dtype=np.uint64)
        f ^= tf[idx[i:i + n]]
        r ^= tr[idx[i:i + n]]
    return f, r


@functools.lru_cache(maxsize=None)
def pools(k, s_bits, gap=0):
    """-> {"tie" | "plain" | "below" | "none": [k-byte windows]}, at least POOL_MIN (at most 64) in every pool that exists for s_bits"""
    names = ("tie", "plain", "none") + (("below",) if s_bits >= 8 else ())
    n = 600_000
    while True:
        rng = np.random.default_rng(100_000 * k + 100 * s_bits + gap)
        idx = rng.integers(0, 4, size=n)
        seq = ACGT[idx].tobytes()
        f, r = _strand_hashes(idx, k, gap)
        h = np.minimum(f, r)
        if gap == 0:
            oh, _ = orc.hash_read(seq, k)
            assert np.array_equal(oh, h)
        # a flagged strand leaves min(fh, rh) with one of these top bytes (k1h_model.flags_of)
        cand = np.flatnonzero(np.isin(h >> np.uint64(56), np.array([0, 1, 0x7e, 0x7f], dtype=np.uint64)))
        out = {nm: [] for nm in names}
        for s in cand:
            win = seq[s:s + k]
            ok, fv, rv = km.window_hashes(win, k, gap)
            assert ok and fv == int(f[s]) and rv == int(r[s])
            cf, cr = km.flags_of(fv, rv, s_bits)
            hit = bool(sampled(min(fv, rv), s_bits))
            if cf and cr:
                out["tie"].append(win)
            elif cf or cr:
                assert hit or s_bits >= 8
                out["plain" if hit else "below"].append(win)
        for s in range(0, n - k, 997):
            ok, fv, rv = km.window_hashes(seq[s:s + k], k, gap)
            if not any(km.flags_of(fv, rv, s_bits)) and len(out["none"]) < 64:
                out["none"].append(seq[s:s + k])
        if all(len(out[nm]) >= POOL_MIN for nm in names):
            return {nm: out[nm][:64] for nm in names}
        n *= 2
        assert n <= 40_000_000, (k, s_bits, gap, {nm: len(v) for nm, v in out.items()})


class _Picker:
    """the windows of a pool, one after the other"""

    def __init__(self, k, s_bits, gap):
        self.p, self.i = pools(k, s_bits, gap), collections.Counter()

    def names(self):
        return tuple(self.p)

    def take(self, name):
        w = self.p[name][self.i[name] % len(self.p[name])]
        self.i[name] += 1
        return w


def _spoil(read, positions, w, k):
    """non-base bytes at `positions`: a mimic of the base inside the planted window [w, w + k), N outside"""
    for p in positions:
        read[p] = MIMIC[read[p]] if w <= p < w + k else N


# ---- F1 families --------------------------------------------------------------------------------------------------------------------
F1_K = (12, 17, 32)


def f1_lengths(k):
    return tuple(L for L in (k, k + 1, 47, 48, 49, 80) if L >= k)


@functools.lru_cache(maxsize=None)
def f1_single(k, L, s_bits=7, gap=0):
    """one N at position p of a read of L bases, for every p"""
    rng = np.random.default_rng(11 * k + L)
    reads = []
    for p in range(L):
        r = _rand_read(rng, L)
        r[p] = N
        reads.append(r)
    return Case(_filled(reads, rng, L), L, k, s_bits, gap, None)


@functools.lru_cache(maxsize=None)
def f1_pairs(k, s_bits=7, gap=0):
    """two N: the first at every offset of piece 1, the second d bytes behind it (and, so that the family's dirty bytes visit every position of the
    read, the first at every offset of piece 0 with the second k - 1 behind)"""
    L = 80
    rng = np.random.default_rng(13 * k)
    reads = []
    for o in range(16):
        for first, d in [(16 + o, d) for d in sorted({1, 15, 16, 17, k - 2, k - 1, k, k + 1, 31, 32, 33, 47})] + [(o, k - 1), (16 + o, L - 1 - 16 - o)]:
            if first + d < L:
                r = _rand_read(rng, L)
                r[first] = r[first + d] = N
                reads.append(r)
    return Case(_filled(reads, rng, L), L, k, s_bits, gap, None)


@functools.lru_cache(maxsize=None)
def f1_runs(k, s_bits=7, gap=0):
    """a run of 1 .. k + 1 N from the offsets 0, 7 and 15 of a piece; an all-N read; reads whose first / last byte is N"""
    L = 80
    rng = np.random.default_rng(17 * k)
    reads = []
    for start in (16, 23, 31):
        for n in range(1, k + 2):
            r = _rand_read(rng, L)
            r[start:start + n] = b"N" * n
            reads.append(r)
    reads.append(bytearray(b"N" * L))
    for p in (0, L - 1):
        r = _rand_read(rng, L)
        r[p] = N
        reads.append(r)
    return Case(_filled(reads, rng, L), L, k, s_bits, gap, None)


BYTES256 = tuple(v for v in range(256) if v not in SLOT_BYTES)


@functools.lru_cache(maxsize=None)
def bytes256(k=32, s_bits=7):
    """every byte value but the reference table's slot bytes, once at piece offset 0 and once at piece offset 15 of a mid-read piece.  The oracle
    decides what a base is (U and u are: dirty to K1h, but they must not leave F1; the values one bit away from a letter are not)"""
    L = 80
    rng = np.random.default_rng(256 + k)
    reads = []
    for v in BYTES256:
        for p in (32, 47):
            r = _rand_read(rng, L)
            r[p] = v
            reads.append(r)
    return Case(_filled(reads, rng, L), L, k, s_bits, 0, None)


# ---- suspects -----------------------------------------------------------------------------------------------------------------------
def _position_sets(w, k, L):
    """the placements of non-base bytes around the window [w, w + k) of a read of L bases (absolute positions)"""
    c0 = w // 16
    sets = [(w + rel,) for rel in (-1, 0, 1, k - 2, k - 1, k)]
    ins, unc = [], []  # per piece c0 + j: a position the window covers / one it does not (the farthest from the window)
    for j in range(3):
        piece = range(16 * (c0 + j), 16 * (c0 + j) + 16)
        cov = [p for p in piece if w <= p < w + k]
        out = [p for p in piece if not w <= p < w + k and p < L]
        ins.append(cov[len(cov) // 2] if cov else None)
        unc.append((out[0] if out[0] < w else out[-1]) if out else None)
    for j in range(3):
        sets += [(unc[j],), (ins[j],)]
    for j1 in range(3):
        for j2 in range(j1 + 1, 3):  # pairs in two different pieces
            sets += [(a, b) for a in (ins[j1], unc[j1]) for b in (ins[j2], unc[j2])]
    sets += [tuple(ins), tuple(unc), (unc[0], ins[1], unc[2]), (ins[0], unc[1], ins[2])]  # one in each piece
    good = []
    for s in sets:
        if all(p is not None and 0 <= p < L for p in s) and tuple(sorted(s)) not in good:
            good.append(tuple(sorted(s)))
    return good


def _suspect_reads(k, s_bits, gap, L, starts, seed):
    rng = np.random.default_rng(seed)
    pick = _Picker(k, s_bits, gap)
    reads, planted = [], []
    for name in pick.names():
        for w in starts:
            assert 0 <= w and w + k <= L
            for pos in _position_sets(w, k, L):
                r = _rand_read(rng, L)
                r[w:w + k] = pick.take(name)
                _spoil(r, pos, w, k)
                planted.append((len(reads), w, name))
                reads.append(r)
    return reads, planted, rng


@functools.lru_cache(maxsize=None)
def _suspects(k, s_bits, gap, L, starts):
    reads, planted, rng = _suspect_reads(k, s_bits, gap, L, starts, 19 * k + s_bits + 1000 * gap + L)
    return Case(_filled(reads, rng, L), L, k, s_bits, gap, None), tuple(planted)


def suspects(k, s_bits=7, gap=0):
    """the directed suspect matrix: every pool x every offset 0 .. 15 of the window's first piece (the window at 16 + off of an 80-base read) x
    _position_sets"""
    return _suspects(k, s_bits, gap, 80, tuple(range(16, 32)))[0]


def suspects_planted(k, s_bits=7, gap=0):
    """-> ((read, window start, pool), ...) of suspects(k, s_bits, gap)"""
    return _suspects(k, s_bits, gap, 80, tuple(range(16, 32)))[1]


def suspects_end_lengths(k):
    """read lengths at which the planted window ends on the read's last base: 16 + off + k for the offsets 9 and 15, and 64 (the window's last piece is the
    read's last: c0 + j < C cuts the loop over the pieces)"""
    return tuple(sorted({16 + off + k for off in (9, 15)} | {64}))


def suspects_end(k, L, s_bits=7, gap=0):
    """the planted window ends on the last base of a read of L bases (and, for L = 64, windows further in front as well)"""
    starts = (L - k,) + ((16, 25) if L == 64 and L - k > 25 else ())
    return _suspects(k, s_bits, gap, L, starts)[0]


def suspects_end_planted(k, L, s_bits=7, gap=0):
    starts = (L - k,) + ((16, 25) if L == 64 and L - k > 25 else ())
    return _suspects(k, s_bits, gap, L, starts)[1]


@functools.lru_cache(maxsize=None)
def slot_bytes(v, k=32):
    """suspects(k) with one reference-table slot byte in a plain read, and a copy of a planted read with the byte inside its window: the whole launch
    takes K1f's slow path, every planted tie and suspect is re-derived by k1h_slow_kernel"""
    assert v in SLOT_BYTES
    base, planted = _suspects(k, 7, 0, 80, tuple(range(16, 32)))
    reads = list(base.reads)
    a = bytearray(reads[-1])
    a[40] = v
    reads[-1] = bytes(a)
    i, w, _ = next(p for p in planted if p[2] == "plain")
    b = bytearray(reads[i])
    b[w + k // 2] = v
    reads.append(bytes(b))
    return Case(reads, 80, k, 7, 0, None)


@functools.lru_cache(maxsize=None)
def dense(k=32, n_dense=1500):
    """n_dense reads with one planted tie / plain window each (all of them end in the same block) and an N just outside it: one K1h wave hands over
    that many suspects that count, and the four K1f waves that share its region fill their hit-log regions of 256 entries (log_entries = 2^18)"""
    L = 80
    rng = np.random.default_rng(23 * k)
    pick = _Picker(k, 7, 0)
    reads = []
    for i in range(n_dense):
        w = 16 + i % 16
        r = _rand_read(rng, L)
        r[w:w + k] = pick.take("tie" if i % 8 == 0 else "plain")
        r[w - 1 if i % 2 else w + k] = N
        reads.append(r)
    return Case(_filled(reads, rng, L), L, k, 7, 0, None)


# ---- ragged -------------------------------------------------------------------------------------------------------------------------
RAGGED = ((3, 32), (5, 17), (3, 12))


@functools.lru_cache(maxsize=None)
def ragged(C, k, s_bits=7):
    """reads of 16 C - 15 .. 16 C bases, sorted longest first (so is every tile), with tails[tile][d] = the tile's reads with more than d bases in their
    last piece.  In every read length: the read's last real base is N behind a planted window; the planted window ends on the read's last base with an N
    k bases before that base; the read's last base is a non-base byte inside the planted window"""
    rng = np.random.default_rng(29 * C + k)
    pick = _Picker(k, s_bits, 0)
    reads = []
    for ln in range(16 * C - 15, 16 * C + 1):
        for name in pick.names():
            for w, pos in ((ln - 1 - k, (ln - 1,)), (ln - k, (ln - k - 1,)), (ln - k, (ln - 1,))):
                if w < 0 or min(pos) < 0:
                    continue
                r = _rand_read(rng, ln)
                r[w:w + k] = pick.take(name)
                _spoil(r, pos, w, k)
                reads.append(bytes(r))
    while len(reads) < FILL_TO:
        reads.append(bytes(_rand_read(rng, int(rng.integers(16 * C - 15, 16 * C + 1)))))
    reads.sort(key=len, reverse=True)  # (stable)
    ntl = (len(reads) + TILE - 1) // TILE
    tails = np.zeros((ntl, 16), dtype=np.uint32)
    for t in range(ntl):
        ls = np.array([len(r) for r in reads[t * TILE:(t + 1) * TILE]])
        for d in range(16):
            tails[t, d] = int(np.count_nonzero(ls - 16 * (C - 1) > d))
    return Case(reads, 16 * C, k, s_bits, 0, tails)


# ---- the long path under a k list -----------------------------------------------------------------------------------------------------
TRIMMED_PIECE = 48
TRIMMED_LISTS = ((17, 32), (12, 27))


@functools.lru_cache(maxsize=None)
def trimmed(klist):
    """ONE sequence for the long path (pieces of 48 bytes, step S = 48 - (kmax - 1)).  Under a list the smaller k is launched with the trimmed piece
    length T = S + kmin - 1: the bytes behind a "read's" end are real data.  One N at every piece-relative position 0 .. 47, each in a piece of its own
    three pieces apart (no two N share a window); planted tie / plain windows of kmin that end exactly at the trimmed length (the piece's last window)
    and that straddle it (the next piece's first window), each once with an N next to it — behind the trimmed length, or just in front of the window —
    and once without"""
    kmin, kmax = min(klist), max(klist)
    S, PL = TRIMMED_PIECE - (kmax - 1), TRIMMED_PIECE
    T = S + kmin - 1
    rng = np.random.default_rng(31 * kmin + kmax)
    n_pieces = 215
    seq = _rand_read(rng, n_pieces * S + PL - S + 5)
    for p in range(PL):
        seq[(5 + 3 * p) * S + p] = N
    pick = _Picker(kmin, 7, 0)
    j = 5 + 3 * PL + 6
    for with_n in (True, False):
        for name in ("tie", "plain"):
            w = j * S + S - 1  # the last window of piece j for kmin: it ends at the trimmed length
            assert w + kmin == j * S + T
            seq[w:w + kmin] = pick.take(name)
            if with_n:
                seq[j * S + T] = N  # the first byte behind the trimmed "read"
            j += 6
            w = j * S + S  # straddles the trimmed length of piece j: the first window of piece j + 1
            seq[w:w + kmin] = pick.take(name)
            if with_n:
                seq[w - 1] = N
            j += 6
    assert j < n_pieces and (len(seq) - PL) // S + 1 < 300
    return bytes(seq)
