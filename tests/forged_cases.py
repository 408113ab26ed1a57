"""The case tables of the forged k-mer tests (tests/test_hash_forge_host.py on the CPU, tests/test_forged_hll_gpu.py and tests/test_forged_sketch_gpu.py on
the device).  tests/hash_forge.py chooses k-mers whose hash values have prescribed bits; a case holds engine parameters, the reads and the PLANNED effect —
which register or counter, what value or count.  The expected results of the GPU tests are the models' (tests/hll_model.py, tests/strand_model.py); the
host test shows that the models compute what every case plans.  Everything is built once (functools.lru_cache) and never changed.

k: 96 where one strand is prescribed (rank 64 of 64 from k = 70 on; a second strand that only has to be the larger one costs one or two bits more), 160
where both are (rank 124 of 128), 300 for K1's long windows, 32 and 20 for the tiled kernels (rank k: at k = 32 at most 25 bits of one strand or 16 of each)."""
import collections
import functools
import random

import numpy as np

import hash_forge as hf
import strand_model as sm
from support import sampled

NAMES = {sm.CANONICAL: "canonical", sm.FORWARD: "forward", sm.REVERSE: "reverse"}
SPACED96 = "1" * 40 + "0" * 16 + "1" * 40  # one interior run of zeros


def kmer(k, picked, strand=sm.CANONICAL, holder=sm.FORWARD, mask=None, other=None, seed=None):
    """a k-mer whose value on the engine's `strand` has the bits `picked`.  One strand: nothing is asked of the other (unless `other`).  Canonical: `holder`
    (FORWARD / REVERSE) carries `picked` and the other strand is made the larger one by a few top bits (hf.smaller), or carries `other`"""
    if strand != sm.CANONICAL:
        holder = strand
        other = hf.NONE if other is None else other
    elif other is None:
        picked, other = hf.smaller(picked)
    wf, wr = (picked, other) if holder == sm.FORWARD else (other, picked)
    return hf.forge(k, wf, wr, mask=mask, seed=seed)


def seeded(*key):
    """a forge seed that depends on the entry alone, not on the order the tables are built in"""
    return random.Random(repr(key)).randrange(1 << 30)


def n_reads(k, n):
    return [b"N" * k] * n


# ================================================================ nthll ================================================================
# plan: {(plane, bucket): value} — registers that must hold exactly this at the end; complete: every other register of the case is zero
HllCase = collections.namedtuple("HllCase", "name masks seeded strand n_bits submits plan complete f1")


def hll_case(name, masks, strand, n_bits, submits, plan, complete=True, seeded_engine=False, f1=None):
    submits = tuple(tuple(s) for s in submits)
    if f1 is None and complete:  # reads of exactly k bases without an N: one window each
        f1 = (sum(1 for s in submits for r in s if len(r) == len(masks[0]) and b"N" not in r),)
    return HllCase(name, tuple(masks), seeded_engine, strand, n_bits, submits, dict(plan), complete, f1)


def bucket_of(j, n_bits):
    return j if n_bits == 4 else (j * 0x9E3779B1 + 5) & ((1 << n_bits) - 1)


LADDER_K = 96


@functools.lru_cache(maxsize=None)
def ladder(n_bits, strand=sm.CANONICAL, mask=None):
    """[(what, k-mer, bucket, run0 or None)]: one k-mer per bucket with run0 in 0, 1, 30, 31, 32, 33 and 63 - n_bits (only the lowest bit of the rest set),
    one with rest == 0 (changes nothing), and two of one bucket with run0 31 and 32; the holder of the prescribed value alternates between the strands"""
    k = LADDER_K if mask is None else len(mask)
    out = []
    rows = [(str(r), hf.lz(r, n_bits, bucket_of(j, n_bits)), bucket_of(j, n_bits), r) for j, r in enumerate((0, 1, 30, 31, 32, 33))]
    rows.append(("lowest", hf.lz_only_lowest(n_bits, bucket_of(6, n_bits)), bucket_of(6, n_bits), 63 - n_bits))
    rows.append(("rest0", hf.lz(64 - n_bits, n_bits, bucket_of(7, n_bits)), bucket_of(7, n_bits), None))
    rows.append(("pair31", hf.lz(31, n_bits, bucket_of(8, n_bits)), bucket_of(8, n_bits), 31))
    rows.append(("pair32", hf.lz(32, n_bits, bucket_of(8, n_bits)), bucket_of(8, n_bits), 32))
    deep = min(40, 62 - n_bits)
    rows.append(("deep", hf.lz(deep, n_bits, bucket_of(5, n_bits)), bucket_of(5, n_bits), deep))  # the bucket of run0 33: for the merge
    for j, (what, want, bucket, run0) in enumerate(rows):
        holder = sm.FORWARD if j % 2 == 0 else sm.REVERSE
        out.append((what, kmer(k, want, strand, holder, mask, seed=seeded("ladder", n_bits, strand, mask, what)), bucket, run0))
    return tuple(out)


def ladder_plan(rows, plane=0):
    plan = {}
    for _, _, bucket, run0 in rows:
        if run0 is not None:
            plan[(plane, bucket)] = max(plan.get((plane, bucket), 0), run0)
    return plan


def ladder_rows(n_bits, *skip, **kw):
    return [r for r in ladder(n_bits, **kw) if r[0] not in skip]


@functools.lru_cache(maxsize=None)
def ladder_cases():
    out = []
    for n_bits in (4, 16, 24):
        base = ladder_rows(n_bits, "pair31", "pair32", "deep")
        a, b = (next(r for r in ladder(n_bits) if r[0] == w) for w in ("pair31", "pair32"))
        for name, first, second in (("up", a, b), ("down", b, a)):
            out.append(hll_case(f"ladder_b{n_bits}_{name}", ["1" * LADDER_K], sm.CANONICAL, n_bits, [[r[1] for r in base] + [first[1]], [second[1]]],
                                ladder_plan(base + [a, b])))
    return tuple(out)


STRAND_K = 160


@functools.lru_cache(maxsize=None)
def strand_kmers():
    """[(k-mer, (forward bucket, run0), (reverse bucket, run0), the strand the canonical value is)] at n_bits 16: both strands prescribed.  The strands
    differ first in the bit under the leading one / in bit 31 behind equal top halves, and each has its own bucket"""
    out = []
    rows = [("f_smaller", hf.both(hf.top("0" * 20 + "10"), hf.low(16, 0x1111)), hf.both(hf.top("0" * 20 + "11"), hf.low(16, 0x2222)), 20, 20, sm.FORWARD),
            ("r_smaller", hf.both(hf.top("0" * 9 + "11"), hf.low(16, 0x3333)), hf.both(hf.top("0" * 9 + "10"), hf.low(16, 0x4444)), 9, 9, sm.REVERSE),
            ("f_deeper", hf.lz(25, 16, 0x5555), hf.lz(3, 16, 0x6666), 25, 3, sm.FORWARD),
            ("r_deeper", hf.lz(2, 16, 0x7777), hf.lz(33, 16, 0x8888), 2, 33, sm.REVERSE)]
    for what, top32, first in (("tie_f", 0x000A5A5A, sm.FORWARD), ("tie_r", 0x00000C3C, sm.REVERSE)):
        j = len(rows)
        lf, lr = ("0", "1") if first == sm.FORWARD else ("1", "0")
        wf, wr = hf.tie32(top32, lf, lr, 16, 0x9000 + j, 0xA000 + j)
        run0 = 64 - top32.bit_length() - 32
        rows.append((what, wf, wr, run0, run0, first))
    for what, wf, wr, rf, rr, first in rows:
        out.append((hf.forge(STRAND_K, wf, wr, seed=seeded("strand", what)), (wf[0] & 0xFFFF, rf), (wr[0] & 0xFFFF, rr), first))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def strand_cases():
    rows = strand_kmers()
    out = []
    for strand in (sm.CANONICAL, sm.FORWARD, sm.REVERSE):
        plan = {}
        for _, f, r, first in rows:
            bucket, run0 = f if (strand == sm.FORWARD or (strand == sm.CANONICAL and first == sm.FORWARD)) else r
            plan[(0, bucket)] = run0
        out.append(hll_case(f"strands_{NAMES[strand]}", ["1" * STRAND_K], strand, 16, [[r[0] for r in rows]], plan))
    return tuple(out)


THRESHOLD_M = (1, 7, 29, 30, 31, 35)


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """n_bits 4.  Submit 1 puts all 16 registers at m; the launch of submit 2 reads its threshold from them.  Submit 2: run0 = m (no change), m + 1 and m + 5
    (must raise), and on the canonical engine a k-mer whose qualifying value is the reverse strand's while the forward value starts with a 1, and its mirror"""
    out = []
    for m in THRESHOLD_M:
        for strand, k in ((sm.FORWARD, 96), (sm.CANONICAL, 160)):
            key = ("thr", m, strand)
            warm = [kmer(k, hf.lz(m, 4, b), strand, sm.FORWARD if b % 2 else sm.REVERSE, seed=seeded(key, "warm", b)) for b in range(16)]
            plan = {(0, b): m for b in range(16)}
            second = [kmer(k, hf.lz(m, 4, 0), strand, sm.FORWARD, seed=seeded(key, "same")),
                      kmer(k, hf.lz(m + 1, 4, 1), strand, sm.REVERSE, seed=seeded(key, "one")),
                      kmer(k, hf.lz(m + 5, 4, 2), strand, sm.FORWARD, seed=seeded(key, "five"))]
            plan[(0, 1)], plan[(0, 2)] = m + 1, m + 5
            if strand == sm.CANONICAL:
                second.append(kmer(k, hf.lz(m + 2, 4, 3), strand, sm.REVERSE, other=hf.both(hf.top("1"), hf.low(4, 5)), seed=seeded(key, "rev")))
                second.append(kmer(k, hf.lz(m + 3, 4, 4), strand, sm.FORWARD, other=hf.both(hf.top("1"), hf.low(4, 6)), seed=seeded(key, "fwd")))
                plan[(0, 3)], plan[(0, 4)] = m + 2, m + 3
            out.append(hll_case(f"threshold_m{m}_{NAMES[strand]}", ["1" * k], strand, 4, [warm, second], plan))
    return tuple(out)


SUB_BATCH = 16384  # ntc_launch.hip: run_hll's first sub-batch of an engine that has seen nothing


@functools.lru_cache(maxsize=None)
def one_submit_case():
    """one submit of 16384 + 64 reads of 96 bytes: 16 warm every register (run0 7), all-N reads fill the first sub-batch, the second one — launched under the
    threshold of those registers — holds run0 7 (no change), 8 and 12 (must raise)"""
    k, m = 96, 7
    warm = [kmer(k, hf.lz(m, 4, b), sm.FORWARD, seed=seeded("one_submit", b)) for b in range(16)]
    tail = [kmer(k, hf.lz(m + d, 4, b), sm.FORWARD, seed=seeded("one_submit", "tail", d)) for b, d in ((0, 0), (1, 1), (2, 5))]
    reads = warm + n_reads(k, SUB_BATCH - 16) + n_reads(k, 20) + tail + n_reads(k, 64 - 23)
    plan = {(0, b): m for b in range(16)}
    plan[(0, 1)], plan[(0, 2)] = m + 1, m + 5
    return hll_case("one_submit", ["1" * k], sm.FORWARD, 4, [reads], plan)


@functools.lru_cache(maxsize=None)
def plane_case():
    """an engine over k = 96 and 160 (forward, n_bits 4): submit 1 puts plane 0's registers at 30 (reads of 96 bases, no window of 160) and plane 1's at 1
    (reads of 160 bases; their 65 windows of 96 are whatever they are).  Submit 2: a window of 160 with run0 2 — lost if plane 1 ran under plane 0's threshold"""
    warm0 = [kmer(96, hf.lz(30, 4, b), sm.FORWARD, seed=seeded("plane", 0, b)) for b in range(16)]
    warm1 = [kmer(160, hf.lz(1, 4, b), sm.FORWARD, seed=seeded("plane", 1, b)) for b in range(16)]
    second = [kmer(160, hf.lz(2, 4, 5), sm.FORWARD, seed=seeded("plane", "second"))]
    plan = {(1, b): 1 for b in range(16)}
    plan[(1, 5)] = 2
    return hll_case("planes_96_160", ["1" * 96, "1" * 160], sm.FORWARD, 4, [warm0 + warm1, second], plan, complete=False)


def flank(what, n):
    rng = random.Random(repr(what))
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """the ladder's k-mers (n_bits 16) inside reads of ragged lengths (0 .. 9 random bases in front and behind): for submit_reads"""
    rows = ladder_rows(16)
    reads = [flank(("front", j), j % 4) + r[1] + flank(("behind", j), (3 * j) % 10) for j, r in enumerate(rows)]
    return hll_case("ladder_ragged", ["1" * LADDER_K], sm.CANONICAL, 16, [reads], ladder_plan(rows), complete=False)


@functools.lru_cache(maxsize=None)
def offsets_case():
    """the ladder's k-mers at the first, a middle and the last offset of reads of k + 37 bases: for submit_device"""
    rows = ladder_rows(16)
    reads = []
    for j, r in enumerate(rows):
        at = (0, 18, 37)[j % 3]
        reads.append(flank(("front", j), at) + r[1] + flank(("behind", j), 37 - at))
    return hll_case("ladder_offsets", ["1" * LADDER_K], sm.CANONICAL, 16, [reads], ladder_plan(rows), complete=False)


@functools.lru_cache(maxsize=None)
def tiled_case():
    rows = ladder_rows(16)
    return hll_case("ladder_tiled", ["1" * LADDER_K], sm.CANONICAL, 16, [[r[1] for r in rows]], ladder_plan(rows))


@functools.lru_cache(maxsize=None)
def spaced_cases():
    out = []
    for strand in (sm.FORWARD, sm.REVERSE):
        rows = ladder_rows(16, strand=strand, mask=SPACED96)
        out.append(hll_case(f"ladder_spaced_{NAMES[strand]}", [SPACED96], strand, 16, [[r[1] for r in rows]], ladder_plan(rows), seeded_engine=True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def merge_parts():
    """the ladder's k-mers (n_bits 16) split over two engines: each holds registers above 32, bucket_of(5) has 33 in one and 40 in the other"""
    rows = ladder_rows(16)
    a = [r for r in rows if r[0] in ("0", "31", "33", "lowest", "pair32")]
    b = [r for r in rows if r not in a]
    return tuple(a), tuple(b)


@functools.lru_cache(maxsize=None)
def cli_case():
    """n_bits 4: the registers go up to 59"""
    rows = ladder_rows(4)
    return hll_case("ladder_cli", ["1" * LADDER_K], sm.CANONICAL, 4, [[r[1] for r in rows]], ladder_plan(rows))


def hll_cases():
    return (ladder_cases() + strand_cases() + threshold_cases() + (one_submit_case(), plane_case(), ragged_case(), offsets_case(), tiled_case())
            + spaced_cases() + (cli_case(),))


def all_reads(c):
    return [r for s in c.submits for r in s]


@functools.lru_cache(maxsize=None)
def hll_model_after(name, n_submits):
    """(registers, F1) of the model after the first n_submits submits of the case"""
    import hll_model as hm
    c = next(c for c in hll_cases() if c.name == name)
    return hm.model([r for s in c.submits[:n_submits] for r in s], list(c.masks), c.strand, c.n_bits)


def hll_model(c):
    return hll_model_after(c.name, len(c.submits))


# ================================================================ ntcard ================================================================
S_BITS = (2, 7, 8, 11, 12, 16, 20, 23, 24)
R_BITS = 14
# what: the entry's name; kmer; count: how often it is submitted; sample: 0 / 1, None for a miss; index, index_bits: the low bits prescribed of the picked value
Entry = collections.namedtuple("Entry", "what kmer count sample index index_bits")
Family = collections.namedtuple("Family", "name k mask strand s_bits r_bits entries")


def index_budget(k, s_bits, r_bits, both_strands=False):
    """how many low bits a k-mer of this family may prescribe beside its pattern: all r_bits where the rank is no concern (k >= 96), else what stays
    within the rank with a margin (k = 32: 25 bits of one strand, 16 of each of two; k = 20: 18 bits)"""
    if k >= 96:
        return r_bits
    room = (15 if both_strands else 24) if k >= 32 else (9 if both_strands else 18)
    return max(0, min(r_bits, room - (s_bits + 3)))


@functools.lru_cache(maxsize=None)
def family(k, s_bits, r_bits=R_BITS, mask=None, strand=sm.CANONICAL):
    """the k-mers of one (k, mask, strand, s_bits, r_bits): hits of both samples, with the bit just under the pattern both ways, with the lowest and the
    highest index; near misses that flip the first and the last pattern bit of either sample; on a canonical engine K1's superset case (one strand 0^s 1..,
    the other 0^(s+1)..: the minimum is not sampled) and both strands matching the pattern with lower bits deciding.  Every hit has a counter of its own and
    is submitted 1, 2, 3, ... times; a miss once.  The prescribed value is the picked one, its holder alternates between the strands"""
    kk = k if mask is None else len(mask)
    name = f"k{kk}{'m' if mask else ''}_{NAMES[strand]}_s{s_bits}r{r_bits}"
    nb = index_budget(kk, s_bits, r_bits)
    top_index = (1 << nb) - 1
    rows = [("hit0", 0, dict(), 1), ("hit1", 1, dict(), 2), ("hit0_below0", 0, dict(below=0), 3), ("hit0_below1", 0, dict(below=1), 4),
            ("hit1_below0", 1, dict(below=0), 5), ("hit1_below1", 1, dict(below=1), 6), ("hit0_index0", 0, dict(), 0), ("hit1_index_top", 1, dict(), top_index),
            ("miss0_first", None, dict(sample=0, flip=0, below=0), 9), ("miss0_last", None, dict(sample=0, flip=-1, below=0), 10),
            ("miss1_first", None, dict(sample=1, flip=0, below=0), 11), ("miss1_last", None, dict(sample=1, flip=-1, below=0), 12)]
    entries = []
    for j, (what, sample, kw, index) in enumerate(rows):
        index &= top_index
        want = hf.sampled(kw.pop("sample", sample), s_bits, index if nb else None, nb, **kw)
        holder = sm.FORWARD if j % 2 == 0 else sm.REVERSE
        other = None
        if what == "miss1_first" and strand == sm.CANONICAL and kk < 96 and 2 * s_bits + 3 + nb > kk - 2:
            # 1^s 0: a larger other strand would cost s + 1 bits more than the rank has.  The other strand starts 10 instead: it is the picked one, and not sampled either
            other = hf.top("10")
        km = kmer(kk, want, strand, holder, mask, other=other, seed=seeded(name, what))
        entries.append(Entry(what, km, 1 if sample is None else len(entries) + 1, sample, index if nb else None, nb))
    if strand == sm.CANONICAL:
        nb2 = index_budget(kk, s_bits, r_bits, both_strands=True)
        for what, holder in (("superset_f", sm.FORWARD), ("superset_r", sm.REVERSE)):
            if kk >= 96 or 2 * (s_bits + 1) <= kk - 2:  # s_bits + 1 bits of either strand: within the rank k with a margin
                km = kmer(kk, hf.top("0" * s_bits + "1"), strand, holder, mask, other=hf.top("0" * (s_bits + 1)), seed=seeded(name, what))
                entries.append(Entry(what, km, 1, None, None, 0))
        if nb2 >= 3:  # both strands sample 0, the bit under the pattern orders them; index 6 is the picked one's, 7 the other's
            for what, holder in (("both_match_f", sm.FORWARD), ("both_match_r", sm.REVERSE)):
                index = 6 if holder == sm.FORWARD else 7 + 8 * (nb2 > 3)
                km = kmer(kk, hf.sampled(0, s_bits, index, nb2, below=0), strand, holder, mask, other=hf.sampled(0, s_bits, index ^ 1, nb2, below=1),
                          seed=seeded(name, what))
                entries.append(Entry(what, km, sum(1 for e in entries if e.sample is not None) + 1, 0, index, nb2))
        if kk >= 96:  # both strands sample 0 and equal in bits 63 .. 32, bit 31 orders them: a choice made on the top halves alone takes the other counter
            top32 = int((hf.pattern(0, s_bits) + "10110011100011110101100111000111")[:32], 2)
            for what, holder, index in (("tie_f", sm.FORWARD, 20), ("tie_r", sm.REVERSE, 23)):
                wp, wo = hf.tie32(top32, "0", "1", 8, index, index ^ 1)
                km = kmer(kk, wp, strand, holder, mask, other=wo, seed=seeded(name, what))
                entries.append(Entry(what, km, sum(1 for e in entries if e.sample is not None) + 1, 0, index, 8))
    return Family(name, kk, mask if mask else "1" * kk, strand, s_bits, r_bits, tuple(entries))


def family_reads(fam, lead=b"", trail=b""):
    """every entry `count` times, as reads of the k-mer alone (one window each), or with bytes in front / behind"""
    return [lead + e.kmer + trail for e in fam.entries for _ in range(e.count)]


@functools.lru_cache(maxsize=None)
def values_of_reads(reads, mask):
    return sm.values_of(list(reads), [mask])


def model_sketch(reads, mask, strand, r_bits, s_bits):
    """(t_Counter, F1) of tests/strand_model.py; the windows' values are computed once per read set and mask"""
    return sm.sketch_of(values_of_reads(tuple(reads), mask), strand, r_bits, s_bits)


def model_signature(reads, mask, strand, s_bits):
    """(hashes ascending, counts) of the sampled picked values"""
    fs, rs = values_of_reads(tuple(reads), mask)[0]
    h = sm.pick(fs, rs, strand)
    h = h[sampled(h, s_bits)]
    u, c = np.unique(h, return_counts=True)
    return u.astype(np.uint64), c.astype(np.uint32)


# the families of the GPU tests
K1_FAMILIES = [(k, s) for k in (96, 300) for s in S_BITS]
TILED_FAMILIES = [(32, s, R_BITS) for s in (7, 8, 11, 12, 16)] + [(20, s, R_BITS) for s in (7, 8, 11, 12)] + [(32, 24, 14), (32, 18, 20)]


def sketch_families():
    out = [family(k, s) for k, s in K1_FAMILIES]
    out += [family(96, s, strand=st) for s in S_BITS for st in (sm.FORWARD, sm.REVERSE)]
    out += [family(96, s, mask=SPACED96) for s in S_BITS]
    out += [family(k, s, r) for k, s, r in TILED_FAMILIES]
    out += [family(32, 16, strand=st) for st in (sm.FORWARD, sm.REVERSE)]
    return out
