"""k1h_regs.py — what the K1h kernel body is laid out in: LDS geometry, the physical register map and the kernel arguments (gen_k1h.py).

Registers are assigned by hand: the kernel's live set leaves no room for an allocator (gen_k1h.py).  The VGPR map is a table of named ranges,
each with its owner; two ranges may share registers only if the pair is declared in V_SHARED with the reason why they are never live together —
check_register_map() (run at import and by tests/test_k1h_emulator.py) fails on any overlap that is not declared, and on a declared one that is
none any more.
"""

WAVES = 8                    # waves per workgroup = tiles in flight per CU: two per SIMD (round 5; six in round 4, when a wave's ring was three whole chunks)
QSLOT = 2048                 # one QUARTER of a packed chunk: 4 bases x 2048 reads = [8 rows][64 lanes] dwords, byte t of row i = the read 64 (i + 8 t) + lane
RQ_MAX = 9                   # quarter-slots of the ring: 4 j + 5 are in use, j = (k - 1) div 16 (what 4 windows span, see quarter_enter)
RING_BYTES = RQ_MAX * QSLOT  # 18 KiB (round 4: three packed chunks, 24 KiB)
QCAP = 128                   # queue items, kept as three arrays — hit word, reverse-strand mask (dwords), meta (16 bits: that is what lets 128 items fit) — of QCAP + one
QSTRIDE = QCAP + 1           # dummy slot: a lane with nothing to queue writes there, so the writes need no exec mask (an exec write costs ~2 issue slots).
                             # 128 items, not 64 (round 5): a pass for want of room then always finds 64 items (it ran with 49 on average, the queue could never hold a full
                             # pass AND a step), 154 passes per two tiles instead of 175 (tools: the queue simulation behind DESIGN 5)
Q_META_OFF = QSTRIDE * 8     # byte offset of the meta array behind the two dword arrays
WAREA = (RING_BYTES + QSTRIDE * 10 + 15) // 16 * 16  # 19728 bytes per wave
TABLE_OFF = WAVES * WAREA    # 153728: [2 strands][NG][64] dwords
LDS_BYTES = 160 * 1024


def n_groups(k):
    return (k + 2) // 3


def table_bytes(k):
    return 2 * n_groups(k) * 256


# ---- VGPRs -------------------------------------------------------------------------------------------------
V_LANE4, V_LANE16, V_QDUMMY, V_QBASE, V_WAVE4, V_ONE, V_EXP1, V_VMASK = range(0, 8)  # V_WAVE4: 4 x the wave's number in the launch
V_D0, V_D1, V_D2, V_DN, V_CMASK, V_TACC, V_CARRY0, V_CARRY1, V_SPARE1 = range(8, 17)
V_DMASK = 17       # reads of this block with a dirty piece in one of its three chunks (and valid): their candidates are SUSPECTS
V_WRAPF, V_WRAPR = V_SPARE1, 254  # second homes of the two state bits that wrap around in a walk step (walk_step)
V_F = 18           # F[31]   (register tuples — loads, 64-bit LDS items — must start at even registers on gfx90a+)
V_R = 49           # R[31]
V_H0 = 80          # chunk n-2 planes / P_next
V_H1 = 112
V_I = 144
V_RAW = 176        # 8 slots x 4
V_T = 208          # temps 208 .. 241: the ranges below
V_T0 = V_T + 4     # scratch of the walk / test / pack
V_TP = V_T + 8     # scratch of the resolve pass
N_VGPRS = 255

# name: (first register, how many, owner)
V_RANGES = {
    "fixed": (0, 18, "lane constants, masks, dirty words, tie accumulator, carried plane pair, F's wrap-around bit (V_LANE4 .. V_DMASK): live throughout"),
    "F": (V_F, 31, "forward-strand state planes"),
    "R": (V_R, 31, "reverse-strand state planes"),
    "H0": (V_H0, 32, "base planes of chunk n - 2; the pack's packed words land here as the walk leaves them"),
    "H1": (V_H1, 32, "base planes of chunk n - 1"),
    "I": (V_I, 32, "base planes of chunk n (quarter-major packed bytes until quarter_enter transposes them)"),
    "RAW": (V_RAW, 32, "8 slots x 4 registers of raw bytes in flight"),
    "items": (V_T, 8, "hit words of one step, test -> push: V_PX, V_TIEW, V_RX, V_SXF, V_SXR (a resolve pass run for want of room keeps them)"),
    "xpose": (V_T, 32, "temps of the 32 x 32 bit transpose: perm_rotate all 32, transpose_quarter the first 8"),
    "misc": (V_T0, 4, "address / mask scratch between the steps: prefix mask, tie and dirty store, ring write, epilogue"),
    "walk": (V_T0 + 1, 22, "function planes of one walk step"),
    "test": (V_T0 + 1, 13, "sample test of one step: flag planes a g b nz per strand, two temps, cf, cr, tie"),
    "pack": (V_T0 + 12, 18, "three sets of six: the scheduler interleaves neighbouring groups of the pack"),
    "pass": (V_TP, 26, "resolve pass (class PS)"),
    "push": (V_TP + 1, 4, "queue push: slot address, hit word, meta, meta address"),
    "vconst": (V_T0 + 30, 12, "constants that VOP3 instructions cannot take as literals (VCONST)"),
    "wrapr": (V_WRAPR, 1, "R's wrap-around bit"),
}
# intended overlaps: (range, the ranges it shares registers with, why the two are never live together)
V_SHARED = (
    ("xpose", "items misc walk test pack pass push", "the transpose runs at the end of a block and on entering a quarter, behind a drain: the queue is empty, no step is under way"),
    ("items", "misc walk test", "the suspect pairs are written behind the test, whose scratch they share; every item is pushed before the next step or tail step starts"),
    ("walk", "misc test pack pass push", "the function planes die with their walk step"),
    ("test", "misc pack pass push", "the test's planes are folded into the items before the first push (and any pass it calls); the pack comes behind the pushes"),
    ("pack", "pass", "a pack batch holds no call of the pass: passes run from a push or a drain"),
    ("pass", "push", "a pass for want of room returns to the push's first instruction, which recomputes its scratch"),
)


def vrange(name):
    """-> first register of the named range"""
    return V_RANGES[name][0]


def check_register_map(ranges=None, shared=None, n_vgprs=N_VGPRS):
    """every two VGPR ranges that share a register are declared to (and every declared pair does); nothing lies beyond the last VGPR"""
    ranges = V_RANGES if ranges is None else ranges
    shared = V_SHARED if shared is None else shared
    declared = {frozenset((a, b)) for a, bs, _why in shared for b in bs.split()}
    names = list(ranges)
    for name in names:
        lo, n, _owner = ranges[name]
        assert 0 <= lo and lo + n <= n_vgprs, f"VGPR range {name}: v{lo} .. v{lo + n - 1} lies outside v0 .. v{n_vgprs - 1}"
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (alo, an, _), (blo, bn, _) = ranges[a], ranges[b]
            overlap = alo < blo + bn and blo < alo + an
            if overlap and frozenset((a, b)) not in declared:
                raise AssertionError(f"VGPR ranges {a} (v{alo} .. v{alo + an - 1}) and {b} (v{blo} .. v{blo + bn - 1}) overlap and are not declared to share registers")
            if not overlap and frozenset((a, b)) in declared:
                raise AssertionError(f"VGPR ranges {a} and {b} are declared to share registers and do not")


V_PX = V_T         # forward candidates of the step (hit word)
V_TIEW = V_T + 1   # windows of the step whose strands tie on the top bits
V_RX = V_T + 2     # reverse candidates
V_SXF = V_T + 4    # the same for suspects
V_SXR = V_T + 6
V_XPOSE, V_MISC, V_WALK, V_TEST, V_PACK, V_PUSH = [vrange(x) for x in ("xpose", "misc", "walk", "test", "pack", "push")]
N_WALK = V_RANGES["walk"][1]


class PS:
    """registers of the resolve pass (range "pass")"""
    item = V_TP                 # (x, y): y = the item's meta (16 bits)
    y = V_TP + 1
    m, rest, col, a0, a1, a2 = [V_TP + 2 + i for i in range(6)]
    lo, hi, mid, tb, key, key1, t1 = [V_TP + 8 + i for i in range(7)]
    fld = [V_TP + 15 + g for g in range(11)]
    sflag = a0                  # (once the ring bytes are spent) 0: a hit to log, bit 0: suspect, bit 1: no hit


# constants that VOP3 instructions cannot take as literals (gfx9: one SGPR or inline constant per instruction, no 32-bit literal)
V_CMUL, V_CPERMLO, V_CPERMHI, V_CP16A, V_CP16B, V_CP8A, V_CP8B, V_CM4, V_CM2, V_CM1, V_CQMASK4, V_CBYTE = [vrange("vconst") + i for i in range(12)]
VCONST = ((V_CMUL, 0x00820820), (V_CPERMLO, 0x0c0c0703), (V_CPERMHI, 0x07030c0c), (V_CP16A, 0x05040100), (V_CP16B, 0x07060302),
          (V_CP8A, 0x06020400), (V_CP8B, 0x07030501), (V_CM4, 0x0f0f0f0f), (V_CM2, 0x33333333), (V_CM1, 0x55555555), (V_CQMASK4, (QCAP - 1) * 4), (V_CBYTE, 0x703))
assert V_CBYTE <= 254
assert PS.fld[-1] == V_TP + V_RANGES["pass"][1] - 1 and len(VCONST) == V_RANGES["vconst"][1]
check_register_map()

# ---- SGPRs: s0 .. S_BASE - 1 are left to the compiler (the asm statement's few inputs live there) ----------------
S_BASE = 26
_sn = [S_BASE]


def _salloc(n=1, align=1):
    while _sn[0] % align or (_sn[0] < 34 and _sn[0] + n > 32):  # s32 / s33 are the ABI's stack and frame pointer: reserved even in a kernel without a stack
        _sn[0] += 1
    r = _sn[0]
    _sn[0] += n
    return r


S_EXP0 = _salloc()
S_CHUNKB = _salloc()         # bytes of one tile's slots = C * 32768 (the product with the tile index is 64-bit)
S_DESC = _salloc(4, 4)       # tile being loaded
S_TILES = _salloc(2, 2)
S_SK = _salloc(2, 2)
S_SUS = _salloc(2, 2)        # this wave's region of the suspect list
S_DIRTY = _salloc(2, 2)
S_TIE = _salloc(2, 2)
S_LOGBASE = _salloc(2, 2)    # current log region
S_RET = _salloc(2, 2)
S_F1ACC = _salloc(2, 2)
S_TMP = _salloc(2, 2)        # 64-bit scratch
S_KARG = _salloc(2, 2)       # kept: the pointers needed once in a while (log, log_fill, f1) are re-read from the kernel arguments
S_F0, S_S0 = _salloc(), _salloc()  # first block this wave owns / walks
S_SUSOFF, S_SUSCAP = _salloc(), _salloc()  # bytes used / capacity of the suspect region
S_NTILES, S_C, S_L, S_NVLAST, S_KEYBASE, S_RMASK2, S_LOGREG, S_LOGCAP4 = [_salloc() for _ in range(8)]  # (loaded in this order)
S_NB, S_FEND = _salloc(), _salloc()
S_WF = _salloc()             # flat index (tile * NB + block) of the block being walked
S_LREG, S_LFILL4, S_USELOG = [_salloc() for _ in range(3)]
S_NWAVES = _salloc()
S_WT, S_WN = _salloc(), _salloc()      # block being walked
S_PT, S_PN, S_PREAL = _salloc(), _salloc(), _salloc()  # chunk being packed
S_QT, S_QN, S_QREAL = _salloc(), _salloc(), _salloc()  # chunk being loaded next
S_PSOFF, S_QSOFF = _salloc(), _salloc()
S_STEPMASK = _salloc()
S_RQ = [_salloc() for _ in range(RQ_MAX)]  # LDS addresses of the ring's quarter-slots in window order: S_RQ[i] holds byte i of the oldest window still to be resolved
S_QHEAD4, S_QTAIL4 = _salloc(), _salloc()
S_N, S_A, S_B, S_CC = _salloc(), _salloc(), _salloc(), _salloc()  # scalar scratch
S_SPARE = _salloc()
S_END = _sn[0]
assert S_END <= 100, S_END
# S_STEPMASK: bits 0 .. 15 the steps of this block that complete a window of every read; bits 16 .. 31 (ragged batches, K1hArgs.tails != NULL) the steps that
# end in the reads' last 16-base piece.  S_USELOG: bit 0 the hit log is in use, bit 8 the batch is ragged, bit 9 the queue is being emptied (read by the pass).
# (The compiler reserves s100 / s101 next to VCC, FLAT_SCRATCH and XNACK_MASK: nothing of the kernel may live there.)
F_USELOG, F_RAGGED, F_DRAIN = 0, 8, 9

S_TACC = (S_F1ACC, S_F1ACC + 1, S_SPARE, S_SUSOFF)  # timing build only (S_SUSCAP = the last time stamp): no F1, no suspects

# the asm statement's "s" operands, in order
INPUTS = ["karg_lo", "karg_hi", "wave_gid", "n_waves", "lds_wbase", "first_block", "end_block"]
# byte offsets in struct K1hArgs (ntc_kernels.hpp); the kernel reads them with scalar loads.  The generator writes them into ntc_k1h_gen_defs.inc as
# K1H_GEN_KARGS(X), from which ntc_sketch_k1h_body.hip checks every one against offsetof(K1hArgs, ...)
KARG = dict(tiles=0, log=8, log_fill=16, sketch0=24, f1=32, dirty=40, tie=48, n_tiles=56, n_chunks=60, read_len=64, nv_last=68, key_base=72,
            rmask2=76, log_regions=80, log_region_cap=84, table=88, blocks_per_wave=104, nb_magic=108, sus=112, sus_count=120, sus_cap=128, s_bits=96, tails=144,
            sk_dirty=160)
