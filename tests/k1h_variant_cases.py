"""The cases that run every generated K1h body (ntcard_amd/csrc/gen_k1h.py: one body per (k, gap, sBits class, strand) — VARIANTS x classes 7 / 8 canonical,
STRAND_VARIANTS x classes 7 / 8 one-strand, 138 in all), once on a GPU (tests/test_k1h_variants_gpu.py) and once on the CPU wave emulator
(tests/test_k1h_emulator.py, tests/test_k1h_strand_emulator.py), and the cases over the sBits range of the tiled pair up to and just beyond
r_bits + 1 + (s_bits - 7) = 32.  Host only: numpy, the oracle and gen_k1h.  tests/test_k1h_variant_cases_host.py proves that the two case sets cover the
bodies and that no case is vacuous.

Shapes (the smallest that still reach what depends on k: the window's start chunk, the phase (k - 1) mod 16, the table groups, the parity of the bit that
wraps in a reverse step):
  class 7   2049 reads of k + 29 bases, 1 % non-base bytes (a partial last tile of one read, a window phase per k); on the GPU also 2100 clean reads of k bases
  class 8   sBits 8 over 2500 reads of k + 1 bases, 1 % non-base bytes, and sBits 11 over 2049 clean reads of 97 bases; a gap seed takes k + 29 bases for
            the first; the emulator takes sBits 8 at k + 29 bases and r_bits 12
A canonical body gets one of these (the tests of tests/test_tiled_gpu.py stay); K1H_ASM_K32_G8_S8, which nothing else runs, gets both class-8 shapes.

Seeds: seed_of() unless SEEDS names another — chosen so that the MODEL puts at least 8 increments into both samples (a condition on the inputs alone)."""
import collections
import functools

import numpy as np

import k1h_model as km
import strand_model as sm
from support import gap_mask, oracle_counts, random_reads

gen_k1h = km.gen_k1h

Case = collections.namedtuple("Case", "k gap strand s_bits r_bits n L p_bad seed kind")
STRAND_NAME = {sm.CANONICAL: "canonical", sm.FORWARD: "forward", sm.REVERSE: "reverse"}
MIN_PER_SAMPLE = 8


def case_id(c):
    return f"k{c.k}g{c.gap}-{STRAND_NAME[c.strand]}-s{c.s_bits}r{c.r_bits}-{c.n}x{c.L}" + ("" if c.kind == "equal" else "-" + c.kind)


def sb_class(s_bits):
    return 7 if s_bits == 7 else 8


def body_of(c):
    """the generated body a case runs: (k, gap, strand, sBits class)"""
    return c.k, c.gap, c.strand, sb_class(c.s_bits)


def all_bodies():
    """every body the library is built with, read from the generator"""
    return ({(k, g, sm.CANONICAL, cl) for k, g in gen_k1h.VARIANTS for cl in (7, 8)}
            | {(k, g, st, cl) for k, g, st in gen_k1h.STRAND_VARIANTS for cl in (7, 8)})


# seeds other than seed_of() (found with the model: the default one leaves a sample of the plane with fewer than MIN_PER_SAMPLE increments)
SEEDS = {  # (k, gap, strand, s_bits, n, L): seed
    (12, 0, 1, 7, 2100, 12): 19936, (13, 0, 1, 8, 2500, 14): 28856, (13, 0, 2, 7, 2100, 13): 28865,
    (14, 0, 1, 7, 2100, 14): 37774, (14, 0, 2, 7, 2100, 14): 21946, (15, 0, 1, 7, 2100, 15): 30855,
    (17, 0, 2, 7, 2100, 17): 24946, (18, 0, 1, 8, 2500, 19): 33856, (19, 0, 2, 8, 2500, 20): 26947,
    (20, 0, 2, 7, 2100, 20): 43784, (21, 0, 1, 7, 2100, 21): 36855, (21, 0, 2, 8, 2500, 22): 36866,
    (22, 0, 2, 8, 2500, 23): 37866, (23, 0, 1, 8, 2500, 24): 30937, (23, 0, 2, 7, 2100, 23): 30946,
    (23, 0, 2, 8, 2500, 24): 30947, (24, 0, 1, 7, 2100, 24): 31936, (24, 0, 2, 8, 2500, 25): 31947,
    (25, 0, 2, 7, 2100, 25): 40865, (25, 0, 2, 8, 2500, 26): 32947, (27, 0, 1, 7, 2100, 27): 58693,
    (27, 0, 1, 8, 2500, 28): 34937, (27, 0, 2, 8, 2500, 28): 34947, (28, 0, 1, 7, 2100, 28): 51774,
    (28, 0, 2, 7, 2100, 28): 35946, (28, 0, 2, 8, 2500, 29): 43866, (29, 0, 1, 8, 2500, 30): 36937,
    (29, 0, 2, 7, 2100, 29): 36946, (29, 0, 2, 8, 2500, 30): 36947, (31, 0, 1, 7, 2100, 31): 46855,
    (31, 0, 1, 8, 2500, 32): 38937, (31, 0, 2, 7, 2100, 31): 38946, (31, 0, 2, 8, 2500, 32): 38947,
    (32, 0, 1, 7, 2100, 32): 39936, (32, 0, 2, 7, 2100, 32): 39946, (32, 8, 2, 7, 2100, 32): 48665,
}


def seed_of(k, gap, strand, s_bits, n, L):
    if n >= 50_000:  # a large case: one read set per (k, n, L), shared by the strands and sBits (the model walks it once)
        return 1000 * k + L
    return SEEDS.get((k, gap, strand, s_bits, n, L), 1000 * k + 100 * gap + 10 * strand + s_bits)


def case(k, gap, strand, s_bits, r_bits, n, L, p_bad, kind="equal"):
    return Case(k, gap, strand, s_bits, r_bits, n, L, p_bad, seed_of(k, gap, strand, s_bits, n, L), kind)


# ---- the bodies ----
def _gpu_body_cases():
    out = []
    for k, gap in gen_k1h.VARIANTS:
        ls8 = k + 29 if gap else k + 1
        for strand in (sm.FORWARD, sm.REVERSE):
            out += [case(k, gap, strand, 7, 14, 2049, k + 29, 0.01), case(k, gap, strand, 7, 14, 2100, k, 0.0),
                    case(k, gap, strand, 8, 14, 2500, ls8, 0.01), case(k, gap, strand, 11, 14, 2049, 97, 0.0)]
        out += [case(k, gap, sm.CANONICAL, 7, 14, 2049, k + 29, 0.01), case(k, gap, sm.CANONICAL, 8, 14, 2500, ls8, 0.01)]
        if (k, gap) == (32, 8):
            out.append(case(k, gap, sm.CANONICAL, 11, 14, 2049, 97, 0.0))
    return out


def _emu_cases():
    out = []
    for k, gap in gen_k1h.VARIANTS:
        for strand in (sm.CANONICAL, sm.FORWARD, sm.REVERSE):
            out += [case(k, gap, strand, 7, 14, 2049, k + 29, 0.01), case(k, gap, strand, 8, 12, 2500, k + 29, 0.01)]
    return out


GPU_BODY_CASES = _gpu_body_cases()
EMU_CASES = _emu_cases()

# ---- other routes over bodies no strand test runs (k = 23): a ragged batch beside an equal-length one, with and without NTC_FLAG_DEFER_REDO ----
RAGGED_CASES = [case(23, 0, strand, s_bits, 14, 2100, 64, 0.01, kind="ragged") for strand in (sm.FORWARD, sm.REVERSE) for s_bits in (7, 8)]

# ---- several tiles per team: the queue's tile tags and the ring phase wrap within one launch (tests/test_tiled_gpu.py: the canonical form) ----
SHORT_READ_CASES = [case(k, 0, strand, 7, 20, 3_200_000, L, 0.015) for L, k in ((16, 12), (20, 16)) for strand in (sm.FORWARD, sm.REVERSE)]

# ---- the sBits range: the table word holds r_bits + 1 + (s_bits - 7) bits, up to 17 extra hash bits above the counter index ----
ALL_STRANDS = (sm.CANONICAL, sm.FORWARD, sm.REVERSE)
RANGE_CASES = ([case(k, 0, strand, s_bits, 14, 60_000, 150, 0.002) for k in (32, 23) for s_bits in (13, 16) for strand in ALL_STRANDS]
               + [case(k, 0, strand, 20, 18, 200_000, 150, 0.002) for k in (32, 23) for strand in ALL_STRANDS])  # 18 + 1 + 13 = 32
# 14 + 1 + 17 = 32, the widest extra field: random reads hold no sampled window, so windows that sample are planted (planted_reads)
PLANT_CASES = [case(32, 0, strand, 24, 14, 2049, 150, 0.002, kind="plant") for strand in ALL_STRANDS]
# just beyond: NTC_FLAG_REQUIRE_TILED refuses, without it the general kernel counts
REFUSE_CASES = [case(32, 0, strand, s_bits, r_bits, 2049, 150, 0.002, kind="plant") for r_bits, s_bits in ((18, 21), (15, 24)) for strand in ALL_STRANDS]

GPU_CASES = GPU_BODY_CASES + RAGGED_CASES + SHORT_READ_CASES + RANGE_CASES + PLANT_CASES
ALL_CASES = GPU_CASES + REFUSE_CASES + EMU_CASES

# ---- long sequences on the shared cut: a k list and a piece length no strand test runs, sBits 8 ----
LONG_KLIST, LONG_PIECE, LONG_S_BITS, LONG_R_BITS = (13, 19, 28), 272, 8, 14


def tiled_supports(c):
    """ntc::sketch_k1h_supports for a (k, gap) the library is built with"""
    return 7 <= c.s_bits <= 30 and c.r_bits + 1 + (c.s_bits - 7) <= 32


# ---- planted windows ----
PLANTS = (("clean", 8), ("n_before", 3), ("n_behind", 3), ("n_inside", 3))  # per sample


def solve_window(rng, k, strand, s_bits, sample):
    """-> k bases whose `strand` value matches ntComp's pattern of `sample`.  Per offset the window takes one of two bases; the value is then affine
    over GF(2) in these k choices (an XOR of table words), and the pattern fixes its top s_bits + 1 (sample 0) or s_bits (sample 1) bits: a linear
    system, solved by elimination from a random starting point"""
    nbits = s_bits + 1 if sample == 0 else s_bits
    target = 1 if sample == 0 else (1 << (s_bits - 1)) - 1
    tabs = sm.offset_tables("1" * k)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    while True:
        pairs = [letters[rng.permutation(4)[:2]] for _ in range(k)]
        word = [[int((F if strand == sm.FORWARD else R)[b]) >> (64 - nbits) for b in pairs[i]] for i, F, R in tabs]
        x = [int(v) for v in rng.integers(0, 2, size=k)]
        t = target
        for i in range(k):
            t ^= word[i][x[i]]
        basis = {}  # top bit -> (vector, offsets whose flip gives it)
        for i in range(k):
            v, combo = word[i][0] ^ word[i][1], 1 << i
            while v and v.bit_length() in basis:
                bv, bc = basis[v.bit_length()]
                v, combo = v ^ bv, combo ^ bc
            if v:
                basis[v.bit_length()] = (v, combo)
        flip = 0
        while t and t.bit_length() in basis:
            bv, bc = basis[t.bit_length()]
            t, flip = t ^ bv, flip ^ bc
        if t:
            continue  # these pairs do not span the target: draw others
        return bytes(int(pairs[i][x[i] ^ ((flip >> i) & 1)]) for i in range(k))


def planted_reads(c):
    """-> (arr [n, L], plants): random reads, and in reads of their own (clean otherwise) windows whose value samples at c.s_bits, PLANTS per sample:
    clean; with an N right in front of or right behind the window within one of the 16-byte chunks the window touches (K1h hands it to K1f as a suspect,
    whose verdict on the extra hash bits decides it); with an N inside (no window).  A canonical case plants through either strand and keeps the windows
    whose planted strand is the smaller value.  plants: [(read, offset, sample, what)]"""
    rng = np.random.default_rng(c.seed)
    arr = random_reads(rng, c.n, c.L, c.p_bad)
    rows = rng.permutation(c.n)
    plants = []
    for sample in (0, 1):
        for what, count in PLANTS:
            for _ in range(count):
                r = int(rows[len(plants)])
                while True:
                    via = c.strand if c.strand != sm.CANONICAL else (sm.FORWARD, sm.REVERSE)[int(rng.integers(0, 2))]
                    win = solve_window(rng, c.k, via, c.s_bits, sample)
                    f, v, _ = sm.window_values(win, "1" * c.k)
                    if c.strand != sm.CANONICAL or (f[0] < v[0]) == (via == sm.FORWARD):
                        break
                while True:
                    w = int(rng.integers(0, c.L - c.k + 1))
                    if what == "n_before" and w % 16 == 0:
                        continue
                    if what == "n_behind" and ((w + c.k) % 16 == 0 or w + c.k >= c.L):
                        continue
                    break
                arr[r] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=c.L)]
                arr[r, w:w + c.k] = np.frombuffer(win, dtype=np.uint8)
                if what == "n_before":
                    arr[r, w - 1] = ord("N")
                elif what == "n_behind":
                    arr[r, w + c.k] = ord("N")
                elif what == "n_inside":
                    arr[r, w + int(rng.integers(0, c.k))] = ord("n")
                plants.append((r, w, sample, what))
    return arr, plants




# ---- inputs and expected results ----
def reads_key(c):
    """what a case's reads depend on.  The large cases (seed_of) share their reads across strands and sBits, so the model walks them once; a plant
    depends on the strand and on sBits by construction"""
    return (c.k, c.gap, c.n, c.L, c.p_bad, c.seed, c.kind) + ((c.strand, c.s_bits) if c.kind == "plant" else (None, None))


@functools.lru_cache(maxsize=4)
def _reads(key):
    k, gap, n, L, p_bad, seed, kind, strand, s_bits = key
    if kind == "plant":
        return planted_reads(Case(k, gap, strand, s_bits, 0, n, L, p_bad, seed, kind))[0]
    arr = random_reads(np.random.default_rng(seed), n, L, p_bad)
    if kind == "ragged":  # reads of L - 15 .. L bases; behind a read's end a non-base byte for the model (the tiles hold 'A' there, as the ABI asks)
        lens = np.random.default_rng(seed + 1).integers(L - 15, L + 1, size=n)
        arr[np.arange(L)[None, :] >= lens[:, None]] = ord("#")
    arr.setflags(write=False)
    return arr


def reads_of(c):
    """uint8 [n, L]; kind "ragged": every read ends at its first '#'; kind "plant": planted_reads"""
    return _reads(reads_key(c))


def ragged_list(arr):
    """the reads of a "ragged" case as bytes, each up to its first '#'"""
    return [row[:n].tobytes() for row, n in zip(arr, (arr != ord("#")).sum(axis=1))]


@functools.lru_cache(maxsize=None)
def long_seqs():
    """sequences around the piece length and far above it, with runs of N"""
    rng = np.random.default_rng(LONG_PIECE)
    seqs = []
    for n in (3000, 4097, LONG_PIECE - 1, LONG_PIECE, 5000, 100, 2500, LONG_PIECE + 1):
        s = random_reads(rng, 1, n, 0.0)[0].copy()
        if n > 1000:
            for run in (1, 7, 33):
                p = int(rng.integers(0, n - 40))
                s[p:p + run] = ord("N")
        seqs.append(s.tobytes())
    return tuple(seqs)


CONFIGS_OF_READS = collections.defaultdict(set)  # reads_key -> the (r_bits, s_bits) the table counts these reads under
for _c in ALL_CASES:
    CONFIGS_OF_READS[reads_key(_c)].add((_c.r_bits, _c.s_bits))


@functools.lru_cache(maxsize=6)
def _sketches(key, configs):
    k, gap = key[0], key[1]
    return sm.array_sketches(_reads(key), gap_mask(k, gap), [(s, r, sb) for r, sb in configs for s in ALL_STRANDS])


def model_sketches(c):
    """{strand: (t_Counter, F1)} of the case's reads under its r_bits and sBits, from tests/strand_model.py's array form; one pass over the reads serves
    every case of the table that shares them"""
    configs = CONFIGS_OF_READS.get(reads_key(c), set()) | {(c.r_bits, c.s_bits)}
    got = _sketches(reads_key(c), tuple(sorted(configs)))
    return {s: got[s, c.r_bits, c.s_bits] for s in ALL_STRANDS}


def want(c):
    """the expected (t_Counter, F1): the C oracle for a canonical case, the one-strand model for a strand"""
    if c.strand == sm.CANONICAL:
        arr = reads_of(c)
        return oracle_counts(ragged_list(arr) if c.kind == "ragged" else arr, [c.k], c.gap, c.r_bits, c.s_bits)
    return model_sketches(c)[c.strand]
