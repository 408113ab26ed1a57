"""The directed cases of the general kernel K1 (ntcard_amd/csrc/ntc_sketch_hf.hip: sketch_hf_kernel), host side: numpy, ctypes and the oracle only.

A case names a family, its planes, a read set and how it is submitted.  From that alone this module says
  * which row of K1's table of instantiations every launch of the case selects (launches(): a restatement of launch_sketch_hf's choice and of the host
    planning in front of it: hf_shape, hf_plan, pick_stride, the fused groups and their split, nthll's doubling sub-batches, the signature cut),
  * in which regimes of ntc_k1_variant_stats those launches are (the same conditions, from the ported launch shape),
  * which paths of the kernel the reads reach (paths(): the kernel's own predicates, per wave-batch of 64 consecutive slots),
  * and what the engine must return (expected_sketch, _signature, _hll, _dump: tests/orc.py, strand_model, hll_model and np.unique — no model of the
    hash lives here).
tests/test_k1_cases_host.py shows that the cases cover every row, regime and path, so that tests/test_k1_cases_gpu.py cannot quietly test less than it
claims; the GPU file pins the ports to what the library reports (row, regimes, waves per block).  Every model evaluation is cached: the two files
together compute each reference once per process."""
import functools
import random
from dataclasses import dataclass

import numpy as np

import hll_model
import orc
import strand_model as sm
from support import gap_mask, nt_comp, rseq, sketch_from_values

R_BITS = 14
REGIMES = ("PREFETCH", "BLOCKING", "PARTIAL", "META", "SMALL_BLOCK", "IDLE", "MULTI", "LOG")  # ntc_k1_variant_info::regime, in order
CUS = 256  # the host file plans with the MI355X's CUs; the GPU file with the device's

# ---- K1's table, as launch_sketch_hf walks it: (multi, mode, pref, dump, tiled, one, sig) ----
MAX_FUSED = 4
MAX_ROLL_PAIRS = 4
MAX_DYN_LDS = 160 * 1024 - 2048
TILE = 2048
SIG_CHUNK, SIG_LOG_LIMIT = 1024, 1 << 27


def plain(mask):
    return "0" not in mask


def mask_pairs(mask):
    """(don't-care positions, toggle pairs) of a mask (nthash_tables.hpp: build_seed_plan)"""
    k = len(mask)
    tog = ([0] if mask[0] == "0" else []) + [j + 1 for j in range(k - 1) if mask[j] != mask[j + 1]] + ([k] if mask[-1] == "0" else [])
    return mask.count("0"), (len(tog) + 1) // 2


def n_roll(mask):
    return 0 if plain(mask) or mask_pairs(mask)[1] > MAX_ROLL_PAIRS else mask_pairs(mask)[1]


def seed_lds(mask):
    """ntc_plan.hip: seed_lds — the LDS a spaced seed adds to K1's tables (SeedPlan::blob and 16 B)"""
    if plain(mask):
        return 0
    n_dc, pairs = mask_pairs(mask)
    ngp, nrx = (n_dc + 1) // 2, (pairs - 1 if 1 < pairs <= MAX_ROLL_PAIRS else 0)
    return ((ngp + nrx) * 64 + (ngp + 3) // 4 * 4) * 4 + 16


def hf_shape(stride, ks, seed=0):
    """ntc_plan.hip: hf_shape -> (waves per block, waves per CU, shared bytes); 0 waves: does not fit"""
    per_wave, shared = 64 * stride, 16 + seed + sum((k + 1) // 2 * 256 for k in ks)
    granule, per_cu, static_lds = 1280, 128, 1024 + 256 + 64
    best, wpb = 0, 0
    for w in (4, 8, 12, 16, 3, 2, 1):  # whole multiples of the 4 SIMDs; smaller blocks only when not even 4 waves fit
        if w < 4 and best:
            break
        alloc = (shared + w * per_wave + static_lds + granule - 1) // granule
        if alloc > per_cu or shared + w * per_wave > MAX_DYN_LDS:
            continue
        waves = min(16, per_cu // alloc * w)
        if waves >= best:  # ties: the larger block
            best, wpb = waves, w
    return wpb, best, shared


def hf_plan(cus, n_slots, stride, ks, seed=0):
    """ntc_launch.hip: hf_plan -> (grid, wpb, waves per CU) or None"""
    wpb, wpc, shared = hf_shape(stride, ks, seed)
    if wpc == 0 or shared + wpb * 64 * stride > MAX_DYN_LDS:
        return None
    need = (n_slots + 64 * wpb - 1) // (64 * wpb)
    return max(1, min(need, cus * max(1, wpc // wpb))), wpb, wpc


def pick_stride(maxlen, ks, seed=0):
    """ntc_plan.hip: pick_stride"""
    s0 = (maxlen + 3) & ~3
    if (s0 // 4) & 1:
        return s0
    a, b = hf_shape(s0, ks[:MAX_FUSED], seed), hf_shape(s0 + 4, ks[:MAX_FUSED], seed)
    return s0 + 4 if b[1] >= a[1] and b[1] > 0 else s0


def regimes_of(n_slots, stride, grid, wpb, pref, meta, log):
    nchunk, n_wb, waves = (64 * stride + 1023) >> 10, (n_slots + 63) // 64, grid * wpb
    on = (nchunk <= pref, nchunk > pref, n_slots % 64 != 0, meta, wpb % 4 != 0, n_wb < waves, n_wb >= 2 * waves, log)
    return frozenset(r for r, x in zip(REGIMES, on) if x)


# ---- cases ----
@dataclass(frozen=True)
class Case:
    name: str
    family: str                 # plain, tiled, spaced, hll, sig, dump
    masks: tuple                # one mask per plane; '1' * k: plain k-mers
    gap: int = 0                # 0: Engine(k list); > 0: Engine([k], gap=); -1: Engine.from_seeds(masks)
    strand: str = "canonical"
    s_bits: int = 7
    kind: str = "sketch"        # sketch, sig, hll, dump
    n_bits: int = 0             # nthll
    reads: tuple = ("base", 150, 209)  # read_set() key
    submit: str = "rows"        # rows (stride), tiles, tiles_ragged, host
    stride: int = 152
    rep: int = 0                # MULTI by replication: 1 whole copies of the base set, 2 whole copies + 37 reads (PARTIAL)
    update: str = "atomics"     # atomics: NTC_FLAG_DIRECT_ATOMICS; log: NTC_FLAG_ALWAYS_LOG
    log_entries: int = 0

    @property
    def ks(self):
        return [len(m) for m in self.masks]

    @property
    def one(self):
        return self.strand != "canonical"


def read_len(case):
    return case.reads[1]


# dirty bytes of the second wave: offset 0, k - 1 and k of every k and mask span in use, and L - 1
DIRTY_AT = (0, 11, 12, 13, 15, 16, 23, 24, 28, 29, 30, 31, 32, 33, 38, 39, 47, 48, 63, 64, 96, 97)


@functools.lru_cache(maxsize=None)
def read_set(kind, L, n):
    """base: n reads of L bases — 64 without a non-base byte (CLEAN), 64 with some (DIRTY; among them one each at DIRTY_AT and at L - 1), the rest drawn;
    ragged: n reads of L - 15 .. L bases, one of no bases and two shorter than any k among them; raggedt: without those three"""
    rng = random.Random(7919 * L + 31 * n + len(kind))
    out = []
    if kind == "base":
        at = [p for p in DIRTY_AT if p < L - 1] + [L - 1]
        for i in range(n):
            if i < 64:
                out.append(rseq(rng, L))
            elif i < 128:
                r = bytearray(rseq(rng, L, pn=0.004))
                if i - 64 < len(at):
                    r[at[i - 64]] = ord("N")
                out.append(bytes(r))
            else:
                out.append(rseq(rng, L, pn=rng.choice([0.0, 0.0, 0.004, 0.02])))
    else:
        for i in range(n):
            out.append(rseq(rng, rng.randint(L - 15, L), pn=rng.choice([0.0, 0.0, 0.004])))
        if kind == "ragged":  # ("raggedt": a ragged TILED batch holds reads of one piece count only)
            out[n // 3], out[n // 2], out[n // 2 + 1] = b"", rseq(rng, 9), rseq(rng, 5)
        out[0] = rseq(rng, L)  # (the longest length occurs)
    return tuple(out)


def slot_index(case):
    """the read of every slot: a ragged batch is packed longest first (ntc_submit.hip: plan_rows; ntcard_amd.tile_reads_ragged), stable"""
    reads = read_set(*case.reads)
    if case.submit in ("host", "tiles_ragged"):
        return np.argsort(-np.array([len(r) for r in reads]), kind="stable")
    return np.arange(len(reads))


def rep_slots(case, stride, cus):
    """slots of a replicated case: 2.3 wave-batches per wave of a full launch, in whole copies of the base set (+ 37 reads: PARTIAL)"""
    base = len(read_set(*case.reads))
    wpc = min(hf_shape(stride, g, seed_lds(case.masks[0]))[1] for g in groups_of(case))
    n = -(-int(np.ceil(2.3 * cus * wpc * 64)) // base) * base
    return n + (37 if case.rep == 2 else 0)


def copies(case, n_slots):
    """-> (whole copies m, extra reads): the slots of a replicated case are m copies of the base set and the first `extra` reads once more"""
    base = len(read_set(*case.reads))
    return n_slots // base, n_slots % base


# ---- the launches of a case ----
def groups_of(case):
    """the k groups run_k1 launches for this case, before launch_k1_group's split: runs of up to 4 plain k; a mask alone; tiles: only K1's share"""
    ks, mine = case.ks, [True] * len(case.masks)
    if case.submit in ("tiles", "tiles_ragged"):
        mine = [not k1h_takes(case, i) for i in range(len(ks))]
    out, i = [], 0
    while i < len(ks):
        if not mine[i]:
            i += 1
            continue
        n = 1
        while n < MAX_FUSED and i + n < len(ks) and mine[i + n] and plain(case.masks[i]) and plain(case.masks[i + n]):
            n += 1
        out.append(ks[i:i + n])
        i += n
    return out


def k1h_takes(case, i):
    """ntc_lifecycle.hip: k_tiled — the tiled kernel pair serves plain k = 12 .. 32 of a canonical sketch engine at sBits >= 7 (and the two -g seeds, which
    no case here submits as tiles)"""
    return case.kind == "sketch" and not case.one and plain(case.masks[i]) and 12 <= len(case.masks[i]) <= 32 and case.s_bits >= 7


def split_group(cus, n, stride, ks, seed):
    """ntc_launch.hip: launch_k1_group — a fused group whose tables push the CU below 12 waves and below its members' is halved"""
    p = hf_plan(cus, n, stride, ks, seed)
    wpc = p[2] if p else 0
    worst = min([16] + [hf_shape(stride, [k], seed)[1] for k in ks]) if len(ks) > 1 else 16
    if len(ks) > 1 and wpc < 12 and wpc < worst:
        h = len(ks) // 2
        return split_group(cus, n, stride, ks[:h], seed) + split_group(cus, n, stride, ks[h:], seed)
    assert p, ("does not fit", stride, ks)
    return [(ks, p)]


def row_of(case, ks, stride, wpb, tiled):
    """launch_sketch_hf's choice"""
    sig, dump, hll = case.kind == "sig", case.kind == "dump", case.kind == "hll"
    spaced = not plain(case.masks[case.ks.index(ks[0])]) if len(ks) == 1 else False
    mode = (1 if spaced else 0) | (2 if hll else 0)
    multi = len(ks) > 1 and mode == 0 and not dump
    deep = 10 * 1024 < 64 * stride <= 16 * 1024
    pref = 16 if mode == 0 and not dump and not sig and deep and wpb <= 12 else 10
    return (multi, mode, pref, dump, tiled, case.one, sig)


def batch_of(case, cus):
    """-> (n_slots, stride, meta, tiled) of the batch run_batch gets"""
    n = len(read_set(*case.reads))
    L = read_len(case)
    meta, tiled = case.submit in ("host", "tiles_ragged"), False
    if case.submit == "rows":
        stride = case.stride
    elif case.submit == "host" or not any(k1h_takes(case, i) for i in range(len(case.masks))):  # (tiles of a K1 engine are re-laid out as row slots)
        stride = pick_stride(L, case.ks, max(seed_lds(m) for m in case.masks))
    else:  # K1 stages the tiles themselves
        stride, tiled = 16 * ((L + 15) // 16), True
    return (rep_slots(case, stride, cus) if case.rep else n), stride, meta, tiled


@functools.lru_cache(maxsize=None)
def launches(case, cus=CUS):
    """every K1 launch of the case, in order -> [dict(row, ks, n_slots, first, stride, grid, wpb, regimes)]"""
    n, stride, meta, tiled = batch_of(case, cus)
    log = case.update == "log" and case.kind in ("sketch", "sig")
    out = []

    def add(ks, n_slots, first, plan):
        grid, wpb, _ = plan
        row = row_of(case, ks, stride, wpb, tiled)
        out.append(dict(row=row, ks=ks, n_slots=n_slots, first=first, stride=stride, grid=grid, wpb=wpb,
                        regimes=regimes_of(n_slots, stride, grid, wpb, row[2], meta, log)))

    seed = lambda ks: seed_lds(case.masks[case.ks.index(ks[0])]) if len(ks) == 1 else 0  # noqa: E731
    if case.kind == "dump":
        add(case.ks, n, 0, hf_plan(cus, n, stride, case.ks, seed(case.ks)))
    elif case.kind == "hll":  # run_hll: sub-batches that double with the reads seen, one launch per plane; a replicated case submits its buffer twice
        seen = 0
        for _ in range(2 if case.rep else 1):
            done = 0
            while done < n:
                m = min((max(16384, seen) + 63) & ~63, n - done)
                for k in case.ks:
                    add([k], m, done, hf_plan(cus, m, stride, [k], seed([k])))
                done, seen = done + m, seen + m
    else:
        cuts = [(0, n)]
        if case.kind == "sig":  # run_k1: a plane's value log holds every window of a launch
            L = stride if meta else read_len(case)
            per = max(L - min(case.ks) + 1, 1) if L >= min(case.ks) else 1
            m = (SIG_LOG_LIMIT - 16 * SIG_CHUNK) * 64 // (64 * per + SIG_CHUNK) & ~63
            cuts = [(a, min(m, n - a)) for a in range(0, n, m)]
        for first, cnt in cuts:
            for g in groups_of(case):
                for ks, plan in split_group(cus, cnt, stride, g, seed(g)):
                    add(ks, cnt, first, plan)
    return out


def expected_rows(case, cus=CUS):
    """{row of K1's table: launches of it} of the case (a fused list that does not fit is launched in parts, and a part of one k is another row)"""
    out = {}
    for x in launches(case, cus):
        out[x["row"]] = out.get(x["row"], 0) + 1
    return out


def expected_row(case, cus=CUS):
    """the row the case is there for: that of its last launch"""
    return launches(case, cus)[-1]["row"]


def claims(case, cus=CUS):
    """the regimes some launch of the case is in"""
    return frozenset().union(*[x["regimes"] for x in launches(case, cus)])


# ---- references ----
@functools.lru_cache(maxsize=None)
def plane_values(reads_key, mask):
    """(fs, rs, windows per read) of one plane over a read set, reads in read_set() order (strand_model.window_values)"""
    v = [sm.window_values(r, mask) for r in read_set(*reads_key)]
    fs = np.concatenate([x[0] for x in v]) if v else np.zeros(0, np.uint64)
    rs = np.concatenate([x[1] for x in v]) if v else np.zeros(0, np.uint64)
    cnt = np.array([x[0].size for x in v], dtype=np.int64)
    for a in (fs, rs, cnt):
        a.setflags(write=False)
    return fs, rs, cnt


@functools.lru_cache(maxsize=None)
def canon_values(reads_key, k):
    """(canonical values, windows per read) of plain k-mers over a read set (orc.hash_read)"""
    v = [orc.hash_read(r, k)[0] for r in read_set(*reads_key)]
    h, cnt = (np.concatenate(v) if v else np.zeros(0, np.uint64)), np.array([x.size for x in v], dtype=np.int64)
    h.setflags(write=False)
    cnt.setflags(write=False)
    return h, cnt


def windows(case, i):
    """clean windows per read of plane i"""
    m = case.masks[i]
    return canon_values(case.reads, len(m))[1] if plain(m) and not case.one else plane_values(case.reads, m)[2]


def picked(case, i, strand=None):
    strand, m = strand or case.strand, case.masks[i]
    if strand == "canonical" and plain(m):
        return canon_values(case.reads, len(m))[0]
    fs, rs, _ = plane_values(case.reads, m)
    return sm.pick(fs, rs, sm.STRANDS[strand])


@functools.lru_cache(maxsize=None)
def base_sketch(reads_key, masks, gap, strand, s_bits):
    """(t_Counter, F1) of the read set, once: canonical plain and -g planes from tests/orc.py, masks and strands from strand_model"""
    if strand == "canonical" and gap >= 0:
        tc, f1 = orc.sketch_reads(list(read_set(*reads_key)), [len(m) for m in masks], gap, R_BITS, s_bits)
    else:
        tc, f1 = sketch_from_values([sm.pick(*plane_values(reads_key, m)[:2], sm.STRANDS[strand]) for m in masks], R_BITS, s_bits)
    tc, f1 = np.array(tc), np.array(f1)
    tc.setflags(write=False)
    f1.setflags(write=False)
    return tc, f1


def sketch_of(case, strand=None):
    return base_sketch(case.reads, case.masks, case.gap, strand or case.strand, case.s_bits)


def prefix_sketch(case, extra):
    """the sketch of the first `extra` reads of the base set (the partial copy of a replicated case)"""
    reads = list(read_set(*case.reads))[:extra]
    if not case.one and case.gap >= 0:
        return orc.sketch_reads(reads, case.ks, case.gap, R_BITS, case.s_bits)
    return sketch_from_values([picked(case, i)[:int(windows(case, i)[:extra].sum())] for i in range(len(case.masks))], R_BITS, case.s_bits)


def expected_sketch(case, n_slots=None):
    """(t_Counter uint16, F1) the engine must return; n_slots: the slots of a replicated case"""
    tc, f1 = sketch_of(case)
    if not case.rep:
        return tc, f1
    m, extra = copies(case, n_slots)
    ptc, pf1 = prefix_sketch(case, extra) if extra else (0, 0)
    return ((tc.astype(np.uint64) * m + ptc) & 0xffff).astype(np.uint16), f1 * np.uint64(m) + pf1


def sampled_values(case, i, extra=None):
    """the values of plane i that ntComp samples (of the first `extra` reads only)"""
    v = picked(case, i)
    if extra is not None:
        v = v[:int(windows(case, i)[:extra].sum())]
    return v[nt_comp(v, 0, case.s_bits)[0] < 2]


def expected_signature(case, i, n_slots=None):
    """(hashes ascending, counts) of plane i; a replicated case: counts x copies, saturating at 2^32 - 1"""
    h, c = np.unique(sampled_values(case, i), return_counts=True)
    c = c.astype(np.uint64)
    if case.rep:
        m, extra = copies(case, n_slots)
        c = c * np.uint64(m)
        if extra:
            hx, cx = np.unique(sampled_values(case, i, extra), return_counts=True)
            c[np.searchsorted(h, hx)] += cx.astype(np.uint64)
    return h.astype(np.uint64), np.minimum(c, np.uint64(0xffffffff)).astype(np.uint32)


def expected_hll(case, n_slots=None):
    """(registers [planes, 2^n_bits], F1): a replicated case is submitted twice — registers of the base set, F1 x 2 x copies"""
    regs = np.stack([hll_model.registers(picked(case, i), case.n_bits) for i in range(len(case.masks))])
    f1 = np.array([picked(case, i).size for i in range(len(case.masks))], dtype=np.uint64)
    if case.rep:
        m, extra = copies(case, n_slots)
        px = np.array([int(windows(case, i)[:extra].sum()) for i in range(len(case.masks))], dtype=np.uint64)
        f1 = (f1 * np.uint64(m) + px) * np.uint64(2)
    return regs, f1


def expected_dump(case):
    """per read, the values of its clean windows in window order"""
    v, cnt = picked(case, 0), windows(case, 0)
    return np.split(v, np.cumsum(cnt)[:-1])


# ---- paths ----
def wave_batches(n_wb, grid, wpb):
    """the kernel's share arithmetic (cum(), kAgeShare) -> per wave of the launch (wb_begin, wb_end)"""
    share = {1: (1024,), 2: (530, 494), 3: (354, 342, 328), 4: (267, 263, 249, 245)}
    ranks = (wpb + 3) // 4

    def cum(w):
        return sum(min(max(w - 4 * r, 0), 4) * (share[ranks][r] if wpb % 4 == 0 else 1024 // ranks) for r in range(ranks))

    per_wg, total, out = (n_wb + grid - 1) // grid, cum(wpb), []
    for b in range(grid):
        g0 = min(b * per_wg, n_wb)
        g1 = min(g0 + per_wg, n_wb)
        for w in range(wpb):
            out.append((g0 + (g1 - g0) * cum(w) // total, g1 if w + 1 == wpb else g0 + (g1 - g0) * cum(w + 1) // total))
    return out


BASES = np.zeros(256, dtype=bool)
BASES[list(b"ACGTUacgtu")] = True


@functools.lru_cache(maxsize=None)
def _paths(case, grid, wpb, cus):
    lbl = set()
    reads, idx = read_set(*case.reads), slot_index(case)
    base_n = len(reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)[idx]
    dirty_pos = [np.flatnonzero(~BASES[np.frombuffer(reads[i], dtype=np.uint8)]) for i in idx]
    all_launches = launches(case, cus)
    x = all_launches[-1]
    n_slots = max(y["n_slots"] for y in all_launches)
    n_wb = (n_slots + 63) // 64
    k1_planes = [pi for pi in range(len(case.masks)) if not (x["row"][4] and k1h_takes(case, pi))]
    # sampled windows per slot of the base set and plane, by the reference (nthll: the candidates depend on the moving threshold, no count here)
    hits = None
    if case.kind in ("sketch", "sig"):
        hits = {}
        for pi in k1_planes:
            cnt, s = windows(case, pi), nt_comp(picked(case, pi), 0, case.s_bits)[0] < 2
            hits[pi] = np.bincount(np.repeat(np.arange(base_n), cnt), weights=s, minlength=base_n).astype(np.int64)[idx]
    # a replicated buffer repeats the base set: its first copy and its last (partial) wave-batch show every class
    scan = sorted(set(range(min(n_wb, base_n // 64 + 2))) | {n_wb - 1})
    for wb in scan:
        sl = np.arange(wb * 64, min(wb * 64 + 64, n_slots)) % base_n
        nvalid = sl.size
        for pi in k1_planes:
            m = case.masks[pi]
            k = len(m)
            endq = np.where(lens[sl] >= k, lens[sl], 0)
            maxq, minq = int(endq.max()), (int(endq.min()) if nvalid == 64 else 0)
            dirt = any(dirty_pos[s].size for s in sl)
            if case.kind == "dump":
                lbl.add("RESOLVE_FULL")
            elif hits:
                h = int(hits[pi][sl].sum())
                lbl.add("RESOLVE_FULL" if h >= 65 else "RESOLVE_REST" if h >= 1 else "NO_HIT")
            if maxq == 0:
                lbl.add("NOTHING")
                continue
            spaced_closed = not plain(m) and n_roll(m) == 0
            if minq != maxq or spaced_closed:
                if spaced_closed:
                    lbl.add("RAGGED_MASK")
                if nvalid < 64:
                    lbl.add("RAGGED_PARTIAL")
                elif minq != maxq:
                    lbl.add("RAGGED_LEN")
                e0 = min((k - 1) >> 2, maxq >> 2)
                lbl.add("RAGGED_ONE_BLOCK" if (maxq - 4 * e0 + 31) >> 5 == 1 else "RAGGED_BLOCKS")
                if ((endq > 0) & (endq < ((maxq >> 2) << 2))).any():
                    lbl.add("RAGGED_END_IN_GROUP")
                if (lens[sl] == 0).any():
                    lbl.add("RAGGED_ZERO_LEN")
                for s, e in zip(sl, endq):
                    if e and (dirty_pos[s] < k).any():
                        lbl.add("RAGGED_MARK_FILL")
                    if e and ((dirty_pos[s] >= k) & (dirty_pos[s] < e)).any():
                        lbl.add("RAGGED_MARK_MAIN")
                continue
            lbl.add("DIRTY" if dirt else "CLEAN")
            mark = dirt and any((dirty_pos[s] < k).any() for s in sl)
            lbl.add("START_K%d%s" % (k & 3, "_MARK" if mark else ""))
            L, A = maxq, (k + 3) & ~3
            if L <= A:
                lbl.add("SHORT")
            if L & 3:
                lbl.add("TAIL_STEPS")
                if L > A and (L >> 2) - A // 4 >= 7 and ((L >> 2) - A // 4 - 7) % 8 == 0:
                    lbl.add("FULL_BLOCK_TAIL")
    # per wave of the (one) launch over the whole batch: the hit log's regions and the signature's chunks
    if hits and len(all_launches) == 1:
        pos = np.arange(n_wb * 64)
        per_wb = np.stack([np.where(pos < n_slots, hits[pi][pos % base_n], 0).reshape(n_wb, 64).sum(axis=1) for pi in k1_planes])
        csum = np.concatenate([np.zeros((len(k1_planes), 1), dtype=np.int64), np.cumsum(per_wb, axis=1)], axis=1)
        waves = wave_batches(n_wb, grid, wpb)
        if any(b - a >= 2 for a, b in waves):
            lbl.add("WAVE_BATCHES_2")
        per_wave = np.stack([csum[:, b] - csum[:, a] for a, b in waves])  # [wave, plane]
        if case.kind == "sig" and (per_wave > SIG_CHUNK).any():
            lbl.add("CHUNK_ROLL")
        if "LOG" in x["regimes"]:
            cap, regions = plan_log(case)
            for g, tot in enumerate(per_wave.sum(axis=1)):
                own = len(range(g, regions, len(waves)))
                if own and tot > cap:
                    lbl.add("REGION_ROLL")
                if tot > own * cap:
                    lbl.add("LOG_EXHAUSTED")
        if case.kind == "sig" and x["row"][0] and "WAVE_BATCHES_2" in lbl:
            lbl.add("SIG_FUSED_CARRY")
    elif case.kind == "hll" and any(b - a >= 2 for y in all_launches for a, b in wave_batches((y["n_slots"] + 63) // 64, y["grid"], y["wpb"])):
        lbl.add("WAVE_BATCHES_2")
    return frozenset(lbl)


def plan_log(case):
    """ntc_plan.hip: plan_log -> (region_cap, regions) of the engine's hit log"""
    counters = len(case.masks) * (2 << R_BITS)
    cap = case.log_entries or min(1 << 30, max(1 << 18, 4 * counters))
    cap = max(cap, 1 << 14)
    region_cap = min(32768, max(256, cap // 8192))
    return region_cap, max(1, cap // region_cap)


def paths(case, grid=None, wpb=None, cus=CUS):
    """the labels the case reaches (module docstring); grid, wpb: the shape of its last launch (None: the ported plan's)"""
    x = launches(case, cus)[-1]
    return _paths(case, x["grid"] if grid is None else grid, x["wpb"] if wpb is None else wpb, cus)


# ---- the table ----
ONE = ("forward", "reverse")
G12, G32 = gap_mask(12, 2), gap_mask(32, 8)
SEEDS = ("1110011100111", "0" + "1" * 30 + "0", ("01" * 20)[:39] + "1")


def P(*ks):
    return tuple("1" * k for k in ks)


def full_block_tail_len(k):
    """the shortest L > 150 with L & 3 != 0 whose last full block of 32 recorded steps ends at the partial group"""
    A = (k + 3) & ~3
    return next(L for L in range(151, 400) if L & 3 and (L >> 2) - A // 4 >= 7 and ((L >> 2) - A // 4 - 7) % 8 == 0)


def _cases():
    out = []

    def add(name, family, masks, **kw):
        strands = ("canonical",) + ONE if family in ("plain", "spaced", "hll", "sig", "dump") else ("canonical",)
        for s in strands:
            out.append(Case(name=f"{family}-{name}-{s}", family=family, masks=tuple(masks), strand=s, **kw))

    B150, R156 = ("base", 150, 209), ("ragged", 156, 209)
    # plain rows, pref 10: every k & 3, the lists, SHORT, FULL_BLOCK_TAIL, sBits
    for k in (29, 30, 31, 32, 97):
        add(f"k{k}", "plain", P(k), s_bits=3)
        add(f"k{k}-tail", "plain", P(k), s_bits=3, reads=("base", full_block_tail_len(k), 209), stride=(full_block_tail_len(k) + 3) & ~3)
        for d in (0, 1, 3):
            add(f"k{k}-short{d}", "plain", P(k), s_bits=2, reads=("base", k + d, 1041), stride=(k + d + 3) & ~3)
    add("list4", "plain", P(16, 24, 32, 48), s_bits=3)
    add("list2", "plain", P(33, 64), s_bits=2)
    add("k32-s7", "plain", P(32), s_bits=7, reads=("base", 150, 515))
    add("k32-s11", "plain", P(32), s_bits=11, reads=("base", 150, 4099))
    add("list4-s7", "plain", P(16, 24, 32, 48), s_bits=7, reads=("base", 150, 515))
    # pref 16 rows (PREFETCH there), BLOCKING at 304, SMALL_BLOCK at 700 / 1000, META
    for L in (173, 205, 300):
        add(f"k31-L{L}", "plain", P(31), s_bits=3, reads=("base", L, 209), stride=(L + 3) & ~3)
        add(f"list4-L{L}", "plain", P(16, 24, 32, 48), s_bits=3, reads=("base", L, 209), stride=(L + 3) & ~3)
    add("k97-L300", "plain", P(97), s_bits=3, reads=("base", 300, 209), stride=304)
    for L in (700, 1000):
        add(f"k32-L{L}", "plain", P(32), s_bits=4, reads=("base", L, 329), stride=L)
    for L in (156, 173):
        add(f"k31-ragged{L}", "plain", P(31), s_bits=3, reads=("ragged", L, 209), submit="host")
        add(f"list4-ragged{L}", "plain", P(16, 24, 32, 48), s_bits=3, reads=("ragged", L, 209), submit="host")
    # tiled staging: K1's share of a mixed list, from the tiles
    for L, rag in ((150, 160), (200, 208)):
        for ks in ((32, 64), (32, 64, 96)):
            nm = "-".join(map(str, ks))
            add(f"{nm}-L{L}", "tiled", P(*ks), reads=("base", L, 2053), submit="tiles")
            add(f"{nm}-L{L}-full", "tiled", P(*ks), reads=("base", L, 4096), submit="tiles")
            add(f"{nm}-ragged{rag}", "tiled", P(*ks), reads=("raggedt", rag, 2053), submit="tiles_ragged")
            add(f"multi-{nm}-L{L}", "tiled", P(*ks), reads=("base", L, 4096), submit="tiles", rep=2)
    # NOTHING: wave-batches whose reads are all shorter than k (a ragged batch is packed longest first)
    R100 = ("ragged", 100, 1041)
    add("k97-ragged100", "plain", P(97), s_bits=2, reads=R100, submit="host")
    add("k31-k97-ragged100", "plain", P(31, 97), s_bits=2, reads=R100, submit="host")
    add("k97-ragged100", "sig", P(97), s_bits=2, kind="sig", reads=R100, submit="host")
    add("k97-ragged100", "hll", P(97), n_bits=16, kind="hll", reads=R100, submit="host")
    add("m97-ragged100", "spaced", ("1" * 48 + "0" + "1" * 48,), gap=-1, s_bits=2, reads=R100, submit="host")
    for ks in ((32, 64), (32, 64, 96)):  # BLOCKING on tiles
        add("-".join(map(str, ks)) + "-L300", "tiled", P(*ks), reads=("base", 300, 2053), submit="tiles")
    # spaced seeds
    add("g12", "spaced", (G12,), gap=2, s_bits=3)
    add("g32", "spaced", (G32,), gap=8, s_bits=3)
    add("seeds", "spaced", SEEDS, gap=-1, s_bits=3)
    S30, S31 = "1" * 10 + "0" * 5 + "1" * 15, "1" * 7 + "00" + "1" * 22
    add("spans", "spaced", (S30, S31), gap=-1, s_bits=3)
    add("seed-tail", "spaced", SEEDS[:1], gap=-1, s_bits=3, reads=("base", full_block_tail_len(13), 209), stride=(full_block_tail_len(13) + 3) & ~3)
    add("s31-short1", "spaced", (S31,), gap=-1, s_bits=2, reads=("base", 32, 1041), stride=32)
    add("seeds-L300", "spaced", SEEDS[:2], gap=-1, s_bits=3, reads=("base", 300, 209), stride=304)
    add("seeds-ragged", "spaced", SEEDS, gap=-1, s_bits=3, reads=R156, submit="host")
    # nthll
    for nb in (4, 16):
        add(f"klist-b{nb}", "hll", P(30, 31, 32, 97), n_bits=nb, kind="hll")
    add("seeds-b16", "hll", SEEDS, gap=-1, n_bits=16, kind="hll")
    for L in (205, 300):
        add(f"k32-L{L}", "hll", P(32), n_bits=16, kind="hll", reads=("base", L, 209), stride=(L + 3) & ~3)
        add(f"seed-L{L}", "hll", SEEDS[:1], gap=-1, n_bits=16, kind="hll", reads=("base", L, 209), stride=(L + 3) & ~3)
    add("k31-short1", "hll", P(31), n_bits=16, kind="hll", reads=("base", 32, 1041), stride=32)
    add("k32-ragged", "hll", P(32), n_bits=16, kind="hll", reads=R156, submit="host")
    add("seed-ragged", "hll", SEEDS[:1], gap=-1, n_bits=16, kind="hll", reads=R156, submit="host")
    # signatures
    for sb in (3, 7):
        n = 209 if sb == 3 else 515
        add(f"k31-s{sb}", "sig", P(31), s_bits=sb, kind="sig", reads=("base", 150, n))
        add(f"list4-s{sb}", "sig", P(16, 24, 32, 48), s_bits=sb, kind="sig", reads=("base", 150, n))
        add(f"seeds-s{sb}", "sig", SEEDS, gap=-1, s_bits=sb, kind="sig", reads=("base", 150, n))
    for L in (205, 300):
        add(f"k31-L{L}", "sig", P(31), s_bits=3, kind="sig", reads=("base", L, 209), stride=(L + 3) & ~3)
        add(f"list4-L{L}", "sig", P(16, 24, 32, 48), s_bits=3, kind="sig", reads=("base", L, 209), stride=(L + 3) & ~3)
        add(f"seed-L{L}", "sig", SEEDS[:1], gap=-1, s_bits=3, kind="sig", reads=("base", L, 209), stride=(L + 3) & ~3)
    add("k30-short1", "sig", P(30), s_bits=2, kind="sig", reads=("base", 31, 1041), stride=32)
    add("k31-ragged", "sig", P(31), s_bits=3, kind="sig", reads=R156, submit="host")
    add("list4-ragged", "sig", P(16, 24, 32, 48), s_bits=3, kind="sig", reads=R156, submit="host")
    add("seed-ragged", "sig", SEEDS[:1], gap=-1, s_bits=3, kind="sig", reads=R156, submit="host")
    # dumps: the regimes tests/test_strand_gpu.py and tests/test_seeds_gpu.py lack
    for L in (150, 205, 300):
        add(f"k31-L{L}", "dump", P(31), kind="dump", reads=("base", L, 165), stride=(L + 3) & ~3)
        add(f"seed-L{L}", "dump", SEEDS[:1], gap=-1, kind="dump", reads=("base", L, 165), stride=(L + 3) & ~3)
    # MULTI by replication, every non-dump row; hit-log geometries
    M150, MS150 = ("base", 150, 4099), ("base", 150, 323)
    add("multi-k31", "plain", P(31), s_bits=7, reads=M150, rep=2)
    add("multi-list4", "plain", P(16, 24, 32, 48), s_bits=7, reads=("base", 150, 1027), rep=2)
    add("multi-list4-L300", "plain", P(16, 24, 32, 48), s_bits=7, reads=("base", 300, 1027), stride=304, rep=2)
    add("multi-k31-L173", "plain", P(31), s_bits=7, reads=("base", 173, 1027), stride=176, rep=2)
    add("multi-list4-L173", "plain", P(16, 24, 32, 48), s_bits=7, reads=("base", 173, 1027), stride=176, rep=2)
    add("multi-g12", "spaced", (G12,), gap=2, s_bits=7, reads=MS150, rep=2)
    add("multi-seed", "spaced", SEEDS[:1], gap=-1, s_bits=7, reads=MS150, rep=2)
    add("multi-k32", "hll", P(32), n_bits=16, kind="hll", reads=M150, rep=2)
    add("multi-seed", "hll", SEEDS[:1], gap=-1, n_bits=16, kind="hll", reads=MS150, rep=2)
    add("multi-k31", "sig", P(31), s_bits=7, kind="sig", reads=M150, rep=2)
    add("multi-list4", "sig", P(16, 24, 32, 48), s_bits=7, kind="sig", reads=("base", 150, 1027), rep=2)
    add("multi-list4-L300", "sig", P(16, 24, 32, 48), s_bits=7, kind="sig", reads=("base", 300, 1027), stride=304, rep=2)
    add("multi-seed", "sig", SEEDS[:1], gap=-1, s_bits=7, kind="sig", reads=MS150, rep=2)
    for fam, masks, gap in (("plain", P(31), 0), ("plain", P(16, 24, 32, 48), 0), ("spaced", SEEDS[:1], -1), ("sig", P(31), 0)):
        kind = "sig" if fam == "sig" else "sketch"
        nm = "list4" if len(masks) > 1 else "one"
        add(f"log18-{nm}", fam, masks, gap=gap, s_bits=3, kind=kind, reads=("base", 150, 515), update="log", log_entries=1 << 18)
        add(f"log14-{nm}", fam, masks, gap=gap, s_bits=3, kind=kind, reads=("base", 150, 515), update="log", log_entries=1 << 14)
        add(f"multi-log-{nm}", fam, masks, gap=gap, s_bits=7, kind=kind, reads=MS150 if gap else M150, rep=1, update="log")
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(len(set(c.ks)) == len(c.ks) for c in CASES)  # (launches() finds a plane by its span)
