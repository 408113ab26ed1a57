#!/usr/bin/env python3
"""gen_k1h.py — emits the K1h kernel body (ntc_sketch_k1h.hip): ONE wave per 2048-read tile does everything.

What it computes is ntRead + ntComp (ntcard.cpp:132-158) for one k of 12 .. 32 over a batch in the TILED slot layout
(include/ntcard_hip.h, ntc_submit_tiled_device): canonical ntHash of every window of k ACGTU bases (nthash.hpp:242-257,275-279),
ntComp's two sampling patterns on its top bits, one hit-log entry (= deferred ++t_Counter[...]) per sampled window, F1.

Why a second tiled kernel (round 4): K1c (ntc_sketch_ts.hip) splits a tile over four specialised waves; 36 % of its wave-cycles are
hand-shake waits and every role is a lone wave on its SIMD (one instruction per ~5 clk).  K1h removes the hand-shakes: a wave owns
a tile, streams it chunk by chunk (16 bases x 2048 reads), and nothing it does waits for another wave.  The price is a live set the
compiler cannot hold (62 state planes + 96 base planes + 32 registers of loads in flight), hence this generator: explicit physical
registers, the kernel body as one assembly string, and an emulator (k1h_asm.py) that runs the very same instruction list on the CPU.

Per chunk iteration (flat over the wave's tiles; block n of a tile = the 16 window ENDS e in [16 n - 16 + phi, 16 n + phi), phi =
(k - 1) mod 16, so that the 16 windows of a block all START in one chunk: the resolve pass then reads wave-uniform ring slots):
  * 16 walk steps, both strands bit-sliced (k1h_terms.py: one VGPR = one bit of the 31-bit hash half for 32 reads).  Per step: function
    planes of the incoming / outgoing base, 62 in-place state updates, then — only for steps that complete a window — the sample
    test.  With both strands in one wave the test is EXACT per strand: cf = this window is sampled and the forward strand is
    canonical, cr = ... reverse; cf & cr = the top bits tie (settled by K1f from the bytes).  Candidates go to an LDS queue as
    (32-read hit word, lane | strand | window offset).
  * interleaved with the walk: the NEXT chunk's raw bytes (8 x buffer_load_dwordx4 in flight) are packed to 2 bits per base into the
    registers of planes that have just left the window, validity (non-ACGTU bytes) per 16-byte piece -> one dirty bit per read.
  * resolve passes (subroutine, whenever the queue holds 64 items, and to empty it at the end of a block): lowest set bit of each
    item -> the read's packed words of three ring slots -> 64-bit window code -> 3 bases per look-up in a 32-bit closed-form table
    of the candidate's own strand (the canonical one): low rBits bits of the hash + the bit that tells the two samples apart ->
    counter index -> hit log (coalesced) or, without a log, the literal device atomic (ntcard.cpp:142-143).
  * end of block: packed words -> LDS ring, 32 x 32 bit transpose in place, register rotation by v_swap.
Reads with non-ACGTU bytes and top-bit ties are NOT resolved here: every candidate of a block whose three chunks hold a dirty piece
of that read is dropped, the dirty bits and the tie bits go to two arrays at fixed positions, and K1f (ntc_sketch_k1h.hip,
fixup_kernel) recomputes exactly those (read, block) pairs from the raw bytes with ntHashIterator's semantics
(ntHashIterator.hpp:59-86).  F1 here counts every window; K1f takes the invalid ones back.

Nothing is copied from the reference: the four seeds are its constants (nthash.hpp:25-28), everything else is derived (k1h_terms.py).

One strand (NTC_FLAG_STRAND_TILED): Gen(k, sb_class, gap, strand) with strand 1 (forward) or 2 (reverse) emits the same kernel for that strand alone — its 31
state planes in the walk, ONE candidate plane per window (flags_and_push_one), no tie plane or tie items, the tie words stored as zeros; forward candidates
ride in the item's xf word, reverse ones in xr, so the resolve pass and its table are those of the canonical kernel.  strand 0 emits the canonical list
unchanged.  STRAND_VARIANTS / `gen_k1h.py --strand` at the end of the file.

The generator in three modules: k1h_regs.py (LDS geometry, the checked register map, the kernel arguments), k1h_exp.py (the K1H_EXP timing
switches and their post-pass) and this one: class Gen, whose build() strings the kernel together from named stages.
"""
import sys

from k1h_terms import step_terms, ttbl, g_of, hseed, rol31, tt4, COMP, CODE2  # noqa: F401
from k1h_asm import Prog, v, s, vr, sr, schedule
from k1h_exp import SWITCHES, parse_exp, phase_fix
from k1h_regs import *  # noqa: F401,F403 (the register map is this module's vocabulary; tests and tools read KARG, WAVES, S_END, ... from here)


class Gen:
    def __init__(self, k, sb_class=7, gap=0, strand=0):
        assert 12 <= k <= 32 and 0 <= gap < k - 1 and strand in (0, 1, 2)
        self.k = k
        self.strand = strand                # 0: both strands, the canonical value; 1 forward / 2 reverse: that strand alone is walked, tested and pushed
        self.sb = sb_class
        self.gap = gap                      # spaced seed "1" x (k-g)/2 "0" x g "1" x rest (ntcard.cpp:407-413): the g middle positions do not enter the hash
        self.g0 = (k - gap) // 2            # first don't-care position
        self.g1 = self.g0 + gap - 1         # last one
        self.phi = (k - 1) % 16
        self.j = (k - 1) // 16      # window start chunk = n - 1 - j
        self.ng = n_groups(k)
        self.rq = 4 * self.j + 5    # quarter-slots of the ring in use: the 4 windows of a quarter start in one quarter of chunk n - 1 - j and end in chunk n
        self.nby = (k + 6) // 4     # bytes (quarters) of the ring a window can touch: k bases from base 0 .. 3 of its first quarter
        assert self.nby <= self.rq <= RQ_MAX
        self.p = Prog()
        self.uid = 0
        self.f_terms, self.r_terms = step_terms(k)
        # spaced seed (nthash.hpp:641-646: the don't-care positions' terms are XORed out of fh / rh): shifting the window by one base changes
        # two more terms per strand — the base that leaves the don't-care block at its low end comes in, the one that enters it at its high
        # end goes out:  F'[j] ^= S[j-(k-g0)](leave) ^ S[j-(k-1-g1)](enter),  R'[j] ^= Sc[j+1-g0](leave) ^ Sc[j-g1](enter)
        if gap:
            self.fg_terms = [(tt4(jj - (k - self.g0)), tt4(jj - (k - 1 - self.g1))) for jj in range(31)]
            self.rg_terms = [(tt4(jj + 1 - self.g0, True), tt4(jj - self.g1, True)) for jj in range(31)]
        self.cold = []                      # out-of-line fragments (emitted behind the chunk loop): the common path of a test falls through —
                                            # a taken branch costs a lone wave an instruction-buffer refill
        self.exp = parse_exp()              # timing experiments (K1H_EXP, k1h_exp.py; tools/k1h_variant.sh)

    def on(self, switch):
        """is the timing experiment `switch` (k1h_exp.SWITCHES) on?"""
        assert switch in SWITCHES, switch
        return switch in self.exp

    def lbl(self, base):
        self.uid += 1
        return f"{base}{self.uid}"

    # ---- small helpers: one emitter per sequence that recurs ----
    def bitop3(self, d, a, b, c, fn):
        self.p.i("v_bitop3_b32", d, a, b, c, mods=f"bitop3:0x{ttbl(fn):02x}")

    def call(self, target):
        """subroutine call: target returns with ret + 4"""
        self.p.i("s_getpc_b64", sr(S_RET, 2))
        self.p.i("s_branch", "@" + target)

    def ret(self):
        self.add64(S_RET, S_RET, 4)
        self.p.i("s_setpc_b64", sr(S_RET, 2))

    def add64(self, d, a, lo, hi=0):
        """s[d:d+1] = s[a:a+1] + hi:lo (operands)"""
        self.p.i("s_add_u32", s(d), s(a), lo)
        self.p.i("s_addc_u32", s(d + 1), s(a + 1), hi)

    def mul64(self, lo, hi, a, b):
        """s(hi):s(lo) = s(a) x s(b)"""
        self.p.i("s_mul_i32", s(lo), s(a), s(b))
        self.p.i("s_mul_hi_u32", s(hi), s(a), s(b))

    def karg_load(self, dst, name, n=2, wait=False):
        """s(dst) (n = 1) or s[dst:dst+1] <- the kernel argument `name`"""
        self.p.i("s_load_dwordx2" if n == 2 else "s_load_dword", sr(dst, 2) if n == 2 else s(dst), sr(S_KARG, 2), hex(KARG[name]))
        if wait:
            self.p.i("s_waitcnt", "lgkmcnt(0)")

    def unless_flag(self, bit, target):
        """branch to target if bit `bit` of S_USELOG (F_USELOG, F_RAGGED, F_DRAIN) is clear"""
        self.p.i("s_bitcmp1_b32", s(S_USELOG), bit)
        self.p.i("s_cbranch_scc0", "@" + target)

    def mbcnt(self, dst, lo, hi):
        """v(dst) = set bits of the 64-bit mask hi:lo (operands) below the lane"""
        self.p.i("v_mbcnt_lo_u32_b32", v(dst), lo, 0)
        self.p.i("v_mbcnt_hi_u32_b32", v(dst), hi, v(dst))

    def f1_add(self, n):
        """F1 += s(n) (the timing build keeps its clocks there)"""
        if not self.on("timers"):
            self.add64(S_F1ACC, S_F1ACC, s(n))

    def valid_reads(self, dst):
        """s(dst) = valid reads of the tile being walked: all 2048 but in a partial last tile"""
        p = self.p
        p.i("s_add_u32", s(dst), s(S_WT), 1)
        p.i("s_cmp_eq_u32", s(dst), s(S_NTILES))
        p.i("s_cselect_b32", s(dst), s(S_NVLAST), 2048)

    def prefix_mask(self, dst, n, signed):
        """v(dst) bit m = (64 m + lane < s(n)): cnt = clamp((n - lane + 63) >> 6, 0, 32) low bits set (n <= 2048).  signed: n - lane may be
        negative (n = 0 .. lane: no bit); unsigned: n >= 1 and lane <= 63, never negative.  Scratch: V_MISC, V_MISC + 1"""
        p = self.p
        T = V_MISC
        p.i("v_lshrrev_b32", v(T), 2, v(V_LANE4))
        p.i("v_sub_u32", v(T), s(n), v(T))                      # n - lane
        p.i("v_add_u32", v(T), 63, v(T))
        if signed:
            p.i("v_ashrrev_i32", v(T), 6, v(T))
            p.i("v_max_i32", v(T), 0, v(T))
        else:
            p.i("v_lshrrev_b32", v(T), 6, v(T))                 # groups m with 64 m + lane < n
        p.i("v_min_u32", v(T), 32, v(T))
        p.i("v_cmp_gt_u32_e32", "vcc", 32, v(T))
        p.i("v_lshlrev_b32", v(T + 1), v(T), v(V_ONE))
        p.i("v_add_u32", v(T + 1), -1, v(T + 1))
        p.i("v_cndmask_b32_e64", v(dst), -1, v(T + 1), "vcc")

    def block_masks(self):
        """V_CMASK / V_DMASK of the block from V_D0 .. V_D2 and V_VMASK: candidates are dropped (become suspects) wherever one of the block's
        three chunks holds a dirty piece of the read.  Scratch: V_MISC"""
        p = self.p
        p.i("v_or3_b32", v(V_MISC), v(V_D0), v(V_D1), v(V_D2))
        self.bitop3(v(V_CMASK), v(V_MISC), v(V_VMASK), v(V_VMASK), lambda x, y, z: (1 ^ x) & y)
        p.i("v_and_b32", v(V_DMASK), v(V_MISC), v(V_VMASK))

    def load_slot(self, i):
        """raw slot i <- 1024 bytes at soffset S_A (slots 0 .. 3) / S_B (4 .. 7) of the tile in S_DESC"""
        if not self.on("noload"):
            self.p.i("buffer_load_dwordx4", vr(V_RAW + 4 * i, 4), v(V_LANE16), sr(S_DESC, 4), s(S_A if i < 4 else S_B), mods=f"offen offset:{(i & 3) * 1024} nt")

    def load_slots(self):
        """the eight loads of one batch, in slot order (pack_batch counts on that order)"""
        for i in range(8):
            self.load_slot(i)

    def shift_planes(self):
        """(H0, H1) <- (H1, I)"""
        for i in range(32):
            self.p.i("v_mov_b32", v(V_H0 + i), v(V_H1 + i))
        for i in range(32):
            self.p.i("v_mov_b32", v(V_H1 + i), v(V_I + i))

    def queue_put(self, slot, mslot, word, zr, meta, meta_or=None):
        """one queue item (word, zr, meta) per lane of vcc, S_A = their number (a lane outside vcc writes the dummy slot).  slot, mslot: scratch;
        meta_or: v(meta) = meta_or | 4 x lane on the way"""
        p = self.p
        self.mbcnt(slot, "vcc_lo", "vcc_hi")
        p.i("v_lshl_add_u32", v(slot), v(slot), 2, s(S_QTAIL4))
        p.i("v_and_b32", v(slot), v(V_CQMASK4), v(slot))
        if meta_or is not None:
            p.i("v_or_b32", v(meta), hex(meta_or), v(V_LANE4))
        p.i("v_cndmask_b32_e64", v(slot), v(V_QDUMMY), v(slot), "vcc")     # V_QDUMMY = 4 QCAP: the dummy slot
        p.i("v_lshrrev_b32", v(mslot), 1, v(slot))                          # (the meta array is 16 bits wide)
        p.i("v_add_u32", v(mslot), v(V_QBASE), v(mslot))
        p.i("v_add_u32", v(slot), v(V_QBASE), v(slot))
        p.i("ds_write2_b32", v(slot), v(word), v(zr), mods=f"offset0:0 offset1:{QSTRIDE}")
        p.i("ds_write_b16", v(mslot), v(meta), mods=f"offset:{Q_META_OFF}")
        p.i("s_lshl2_add_u32", s(S_QTAIL4), s(S_A), s(S_QTAIL4))

    def probe(self, sec):
        """timing build (K1H_EXP=timers): the clocks since the last probe go to section `sec` (0 walk + test + push, 1 pack, 2 resolve
        passes, 3 end of block); the four sums are added to f1[1 .. 4] at the end (bench.py --k1h-timers).  F1 itself is not kept."""
        if not self.on("timers"):
            return
        p = self.p
        p.i("s_memtime", sr(S_TMP, 2))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_sub_u32", s(S_N), s(S_TMP), s(S_SUSCAP))
        p.i("s_add_u32", s(S_TACC[sec]), s(S_TACC[sec]), s(S_N))
        p.i("s_mov_b32", s(S_SUSCAP), s(S_TMP))

    # ---- poly-A start state: the hash of k A s, the track every tile starts on ----
    def poly_a(self, strand):
        h = 0
        for t in range(self.k):
            if self.gap and self.g0 <= t <= self.g1:
                continue
            h ^= rol31(hseed("A"), self.k - 1 - t) if strand == "F" else rol31(hseed(COMP["A"]), t)
        return h

    # ---- one walk step -------------------------------------------------------------------------------------
    def plane_back(self, a, d):
        """register of plane bit 0 of the base d positions behind the one step a takes in (d = 0: the incoming base, d = k: the outgoing one)"""
        q = self.phi + a - d                 # position relative to the start of chunk n - 1
        if q >= 16:
            return V_I + 2 * (q - 16)
        if q >= 0:
            return V_H1 + 2 * q
        if q >= -16:
            return V_H0 + 2 * (q + 16)
        assert q == -17 and self.j == 1      # (n - 3, 15): saved before its registers took packed words
        return V_CARRY0

    def planes_of_step(self, a):
        """registers of the incoming / outgoing base planes of step a"""
        i0, o0 = self.plane_back(a, 0), self.plane_back(a, self.k)
        return i0, i0 + 1, o0, o0 + 1

    def fn_plane(self, cache, t4, b0, b1, tpool):
        """function plane of a 4-bit truth table over (b0, b1): -> (register or None, invert)"""
        if t4 == 0x0:
            return None, 0
        if t4 == 0xf:
            return None, 1
        if t4 == 0b1010:
            return b0, 0
        if t4 == 0b0101:
            return b0, 1
        if t4 == 0b1100:
            return b1, 0
        if t4 == 0b0011:
            return b1, 1
        inv = 0
        if t4 & 1:
            t4 ^= 0xf
            inv = 1
        if t4 not in cache:
            r = tpool.pop()
            if t4 == 0b1000:
                self.p.i("v_and_b32", v(r), v(b0), v(b1))
            elif t4 == 0b1110:
                self.p.i("v_or_b32", v(r), v(b0), v(b1))
            elif t4 == 0b0110:
                self.p.i("v_xor_b32", v(r), v(b0), v(b1))
            else:
                g = g_of(t4)
                self.bitop3(v(r), v(b0), v(b1), v(b1), lambda x, y, z: g(x, y))
            cache[t4] = r
        return cache[t4], inv

    def emit_update(self, dst, prev, x, y, inv):
        if x is None and y is None:
            if inv:
                self.p.i("v_not_b32", v(dst), v(prev))
            elif dst != prev:
                self.p.i("v_mov_b32", v(dst), v(prev))
        elif x is None or y is None:
            z = x if y is None else y
            if inv:
                self.bitop3(v(dst), v(prev), v(z), v(z), lambda a, b, c: 1 ^ a ^ b)
            else:
                self.p.i("v_xor_b32", v(dst), v(prev), v(z))
        else:
            self.bitop3(v(dst), v(prev), v(x), v(y), (lambda a, b, c: 1 ^ a ^ b ^ c) if inv else (lambda a, b, c: a ^ b ^ c))

    def emit_tail_step(self):
        """subroutine (S_B = 4 d).  Ragged batch: the step ends at base 16 (C - 1) + d of the reads.  n = tails[tile][d] reads of the tile are that long — a
        prefix of it (longest first): the candidate masks shrink to it (they only ever shrink until the tile ends: the steps in the last piece come in the
        order of d) and F1 takes n windows."""
        p = self.p
        p.label("tailsub")
        self.karg_load(S_TMP, "tails")
        p.i("s_lshl_b32", s(S_A), s(S_WT), 6)
        p.i("s_add_u32", s(S_A), s(S_A), s(S_B))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_load_dword", s(S_A), sr(S_TMP, 2), s(S_A))
        p.i("s_waitcnt", "lgkmcnt(0)")
        self.f1_add(S_A)
        self.prefix_mask(V_MISC + 1, S_A, signed=True)          # (lane >= n: no read of the lane is that long)
        p.i("v_and_b32", v(V_VMASK), v(V_VMASK), v(V_MISC + 1))
        self.block_masks()
        self.ret()

    def walk_step(self, a):
        i0, i1, o0, o1 = self.planes_of_step(a)
        tpool = [V_WALK + i for i in range(N_WALK)][::-1]  # function planes
        cin, cout, clv, cen = {}, {}, {}, {}
        if self.gap:
            l0 = self.plane_back(a, self.k - self.g0)       # leaves the don't-care block (window index g0 -> g0 - 1)
            e0 = self.plane_back(a, self.k - 1 - self.g1)   # enters it (g1 + 1 -> g1)
        plan = {}
        strands = (("F", self.f_terms, getattr(self, "fg_terms", None)), ("R", self.r_terms, getattr(self, "rg_terms", None)))
        if self.strand:
            strands = strands[self.strand - 1:self.strand]   # one strand: the other one's planes are neither planned nor updated (its registers are never read)
        for strand, terms, gterms in strands:
            for jj in range(31):
                tin, tout = terms[jj]
                x, xi = self.fn_plane(cin, tin, i0, i1, tpool)
                y, yi = self.fn_plane(cout, tout, o0, o1, tpool)
                inv = xi ^ yi
                ops = [z for z in (x, y) if z is not None]
                if self.gap:
                    tl, te = gterms[jj]
                    u, ui = self.fn_plane(clv, tl, l0, l0 + 1, tpool)
                    w, wi = self.fn_plane(cen, te, e0, e0 + 1, tpool)
                    inv ^= ui ^ wi
                    ops += [z for z in (u, w) if z is not None]
                plan[strand, jj] = (ops, inv)

        def update(dst, prev, ops, inv):
            # dst = prev ^ ops... ^ inv, three inputs per instruction
            ops = list(ops)
            cur = prev
            first = True
            while first or ops:
                first = False
                take, ops = ops[:2], ops[2:]
                last = not ops
                self.emit_update(dst, cur, take[0] if take else None, take[1] if len(take) > 1 else None, inv if last else 0)
                cur = dst
        # The rotation is in place — F'[j] = F[j-1] ^ terms from the top, R'[j] = R[j+1] ^ terms from the bottom — but for the bit that wraps around (F's bit 0 takes
        # F's old bit 30, R's bit 30 R's old bit 0): that one alternates between its home register and a second one (V_WRAPF / V_WRAPR), written FIRST, while the
        # old value it needs is still there: no copy (round 5; two v_mov per step before).  Even steps find the bit at home and leave it in the second register,
        # odd steps the other way round; a block has 16 steps, so every block starts and ends at home.
        if self.strand != 2:
            f0_old, f0_new = (V_F + 0, V_WRAPF) if a % 2 == 0 else (V_WRAPF, V_F + 0)
            update(f0_new, V_F + 30, *plan["F", 0])
            for jj in range(30, 1, -1):
                update(V_F + jj, V_F + jj - 1, *plan["F", jj])
            update(V_F + 1, f0_old, *plan["F", 1])
        if self.strand != 1:
            r30_old, r30_new = (V_R + 30, V_WRAPR) if a % 2 == 0 else (V_WRAPR, V_R + 30)
            update(r30_new, V_R + 0, *plan["R", 30])
            for jj in range(0, 29):
                update(V_R + jj, V_R + jj + 1, *plan["R", jj])
            update(V_R + 29, r30_old, *plan["R", 29])

    # ---- sample test of one strand: planes a (top bits == sample-1 pattern), g (>=), b (== sample-0 pattern), nz ----
    def strand_flags(self, base, out, top=None):
        """base: first register of the strand's state (top: the register that holds its bit 30 right now, walk_step); out: dict of result registers a, g, b, nz;
        temps t1, t2"""
        t7, b6, b5, b4, b3, b2, b1, b0 = [v(base + 30 - i) for i in range(8)]
        if top is not None:
            t7 = v(top)
        ra, rg, rb, rnz, t1, t2 = [v(out[x]) for x in ("a", "g", "b", "nz", "t1", "t2")]
        if self.sb == 7:
            self.bitop3(t1, b6, b5, b4, lambda x, y, z: x & y & z)
            self.bitop3(t1, t1, b3, b2, lambda x, y, z: x & y & z)          # bits 6..2 all set
            self.bitop3(ra, t7, t1, b1, lambda x, y, z: (1 ^ x) & y & z)     # top 7 bits == 0111111
            self.bitop3(rg, t7, t1, b1, lambda x, y, z: x | (y & z))         # top 7 bits >= 0111111
            self.bitop3(t1, t7, b6, b5, lambda x, y, z: x | y | z)
            self.bitop3(t2, b4, b3, b2, lambda x, y, z: x | y | z)
            self.bitop3(t1, t1, t2, b1, lambda x, y, z: 1 ^ (x | y | z))     # top 7 bits == 0
            self.p.i("v_and_b32", rb, t1, b0)                                # top 8 bits == 00000001
            self.bitop3(rnz, t1, b0, b0, lambda x, y, z: (1 ^ x) | y)        # top 8 bits >= 1
        else:
            # s_bits >= 8: 8-bit prefixes of the patterns: 0x7f (sample 1) and 0x00 (sample 0); the pass checks the rest
            self.bitop3(t1, b6, b5, b4, lambda x, y, z: x & y & z)
            self.bitop3(t1, t1, b3, b2, lambda x, y, z: x & y & z)
            self.bitop3(t1, t1, b1, b0, lambda x, y, z: x & y & z)          # low 7 of the 8 all set
            self.bitop3(ra, t7, t1, t1, lambda x, y, z: (1 ^ x) & y)         # == 0x7f
            self.p.i("v_or_b32", rg, t7, t1)                                 # >= 0x7f
            self.bitop3(t1, t7, b6, b5, lambda x, y, z: x | y | z)
            self.bitop3(t2, b4, b3, b2, lambda x, y, z: x | y | z)
            self.bitop3(t1, t1, t2, b1, lambda x, y, z: x | y | z)
            self.bitop3(rb, t1, b0, b0, lambda x, y, z: 1 ^ (x | y))         # == 0x00
            # nz: any value is >= 0 — handled by the caller (cf = (a & g') | b)

    def strand_candidates(self, base, out, top=None):
        """one strand (self.strand): the candidate plane of the strand whose state starts at register `base` (top: as strand_flags) -> v(out) = a | b, the top bits
        match sample 1's pattern or sample 0's (s_bits >= 8: their 8-bit prefixes).  No g / nz planes: there is no other strand to compare with.  Temps: T + 8, T + 9, T + 10 (flags_and_push_one puts `out` at T + 11): all inside the "test" range, whose g / nz / cf / cr / tie
        planes a one-strand kernel does not have"""
        t7, b6, b5, b4, b3, b2, b1, b0 = [v(base + 30 - i) for i in range(8)]
        if top is not None:
            t7 = v(top)
        t1, t2, t3 = v(V_TEST + 8), v(V_TEST + 9), v(V_TEST + 10)
        self.bitop3(t1, b6, b5, b4, lambda x, y, z: x & y & z)
        self.bitop3(t1, t1, b3, b2, lambda x, y, z: x & y & z)                # bits 6 .. 2 all set
        self.bitop3(t2, t7, b6, b5, lambda x, y, z: x | y | z)
        self.bitop3(t3, b4, b3, b2, lambda x, y, z: x | y | z)
        if self.sb == 7:
            self.bitop3(t1, t7, t1, b1, lambda x, y, z: (1 ^ x) & y & z)       # a: top 7 bits == 0111111
            self.bitop3(t2, t2, t3, b1, lambda x, y, z: 1 ^ (x | y | z))       # top 7 bits == 0
            self.bitop3(v(out), t1, t2, b0, lambda x, y, z: x | (y & z))       # a | b, b: top 8 bits == 00000001
        else:
            self.bitop3(t1, t1, b1, b0, lambda x, y, z: x & y & z)            # low 7 of the 8 all set
            self.bitop3(t2, t2, t3, b1, lambda x, y, z: x | y | z)
            self.bitop3(t2, t2, b0, b0, lambda x, y, z: 1 ^ (x | y))           # b: == 0x00
            self.bitop3(v(out), t7, t1, t2, lambda x, y, z: ((1 ^ x) & y) | z)  # a | b, a: == 0x7f

    def flags_and_push_one(self, a):
        """one strand: the candidate plane of step a, then the pushes — candidates of clean reads, suspects (the candidates under V_DMASK).  No tie plane, no
        tie items, V_TACC stays 0 (end_of_block stores all-zero tie words).  Forward candidates ride in xf with xr = 0, reverse ones in xr with xf = 0: the
        resolve pass picks the strand's half of the table from the item's zr word, as for a canonical item"""
        p = self.p
        cand = V_TEST + 11
        if self.strand == 1:
            self.strand_candidates(V_F, cand)
        else:
            self.strand_candidates(V_R, cand, top=V_WRAPR if a % 2 == 0 else V_R + 30)  # (behind an even step R's bit 30 sits in its second register)
        hit, sx, zero = (V_PX, V_SXF, V_RX) if self.strand == 1 else (V_RX, V_SXR, V_PX)
        p.i("v_and_b32", v(hit), v(cand), v(V_CMASK))
        p.i("v_mov_b32", v(zero), 0)                           # (the other strand's word of both pushes)
        sus = not self.on("timers")
        if sus:
            p.i("v_and_b32", v(sx), v(cand), v(V_DMASK))       # suspects: candidates of reads with a dirty piece near by (K1f knows the bytes)
        self.push_items(a, *((hit, zero) if self.strand == 1 else (zero, hit)), 0)
        if sus:
            nosus = self.lbl("nosus")
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(sx))
            p.i("s_cbranch_vccz", "@" + nosus)                 # (the common case: no suspect in this step)
            self.push_items(a, *((sx, zero) if self.strand == 1 else (zero, sx)), 1)
            p.label(nosus)

    def flags_and_push(self, a):
        """candidate planes of step a (exact per strand), tie plane, then the two pushes"""
        if self.strand:
            return self.flags_and_push_one(a)
        p = self.p
        T = V_TEST
        fo = dict(a=T + 0, g=T + 1, b=T + 2, nz=T + 3, t1=T + 8, t2=T + 9)
        ro = dict(a=T + 4, g=T + 5, b=T + 6, nz=T + 7, t1=T + 8, t2=T + 9)
        self.strand_flags(V_F, fo)
        self.strand_flags(V_R, ro, top=V_WRAPR if a % 2 == 0 else V_R + 30)  # (behind an even step R's bit 30 sits in its second register)
        cf, cr, tie = T + 10, T + 11, T + 12
        if self.sb == 7:
            p.i("v_and_b32", v(T + 8), v(fo["b"]), v(ro["nz"]))
            self.bitop3(v(cf), v(fo["a"]), v(ro["g"]), v(T + 8), lambda x, y, z: (x & y) | z)
            p.i("v_and_b32", v(T + 8), v(ro["b"]), v(fo["nz"]))
            self.bitop3(v(cr), v(ro["a"]), v(fo["g"]), v(T + 8), lambda x, y, z: (x & y) | z)
        else:
            self.bitop3(v(cf), v(fo["a"]), v(ro["g"]), v(fo["b"]), lambda x, y, z: (x & y) | z)
            self.bitop3(v(cr), v(ro["a"]), v(fo["g"]), v(ro["b"]), lambda x, y, z: (x & y) | z)
        p.i("v_and_b32", v(tie), v(cf), v(cr))
        self.bitop3(v(V_PX), v(cf), v(V_CMASK), v(tie), lambda x, y, z: x & y & (1 ^ z))
        self.bitop3(v(V_RX), v(cr), v(V_CMASK), v(tie), lambda x, y, z: x & y & (1 ^ z))
        sus = not self.on("timers")
        if sus:
            # suspects: candidates of reads with a dirty piece near by — resolved like the others, then parked for K1f, which knows the bytes
            # ... and windows whose strands tie on the top bits: items of their own, marked as ties (K1f re-derives a tie's hash from the bytes, so
            # the strand it is queued under does not matter; every other suspect keeps K1h's verdict and only has its dirty pieces looked at)
            p.i("v_and_b32", v(V_TIEW), v(tie), v(V_VMASK))   # (kept in a register a resolve pass does not touch)
            self.bitop3(v(V_SXF), v(cf), v(V_DMASK), v(tie), lambda x, y, z: x & y & (1 ^ z))
            self.bitop3(v(V_SXR), v(cr), v(V_DMASK), v(tie), lambda x, y, z: x & y & (1 ^ z))
            p.i("v_or_b32", v(V_TACC), v(V_TACC), v(V_TIEW))  # (the tie array serves K1f's slow path only)
        else:
            self.bitop3(v(V_TACC), v(V_TACC), v(tie), v(V_CMASK), lambda x, y, z: x | (y & z))
        self.push_items(a, V_PX, V_RX, 0)
        if sus:
            nosus, notdirty = self.lbl("nosus"), self.lbl("notdirty")
            p.i("v_or3_b32", v(T + 3), v(V_SXF), v(V_SXR), v(V_TIEW))
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(T + 3))
            p.i("s_cbranch_vccz", "@" + nosus)                 # (the common case: no suspect in this step)
            p.i("v_or_b32", v(T + 3), v(V_SXF), v(V_SXR))
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(T + 3))
            p.i("s_cbranch_vccz", "@" + notdirty)
            self.push_items(a, V_SXF, V_SXR, 1)
            p.label(notdirty)
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(V_TIEW))
            tiep = self.lbl("tiepush")
            p.i("s_cbranch_vccnz", "@" + tiep)                 # (rare: two windows per block — out of line)
            p.label(nosus)

            def cold_tie(tiep=tiep, nosus=nosus, a=a):
                p.label(tiep)
                self.push_items(a, V_TIEW, V_TIEW, 1, tie=1)
                p.i("s_branch", "@" + nosus)
            self.cold.append(cold_tie)

    def push_items(self, a, xf, xr, suspect, tie=0):
        """queue the hit words of step a (xf: forward-strand candidates, xr: reverse; a read is never in both — ties are masked out or ride in
        xf alone): ONE item per lane = (xf | xr, meta, xr); resolve passes first while the queue lacks room"""
        p = self.p
        slot, word, meta, mslot = [V_PUSH + i for i in range(4)]
        chk, go = self.lbl("chk"), self.lbl("go")
        p.label(chk)
        p.i("v_or_b32", v(word), v(xf), v(xr))
        p.i("v_cmp_ne_u32_e32", "vcc", 0, v(word))
        p.i("s_bcnt1_i32_b64", s(S_A), "vcc")
        p.i("s_sub_u32", s(S_N), s(S_QTAIL4), s(S_QHEAD4))
        p.i("s_lshr_b32", s(S_N), s(S_N), 2)
        p.i("s_add_u32", s(S_N), s(S_N), s(S_A))
        p.i("s_cmp_le_u32", s(S_N), QCAP)
        full = self.lbl("qfull")
        p.i("s_cbranch_scc0", "@" + full)                        # (rare: about one step in three runs a pass first)

        def cold_pass(full=full, chk=chk):
            p.label(full)
            self.call("pass")                                    # (keeps the range "items": the four hit words)
            p.i("s_branch", "@" + chk)
        self.cold.append(cold_pass)
        p.label(go)                                              # (nothing branches here; the label stays: it ends a scheduling region, and the output is pinned)
        # meta bits 0 .. 7: 4 x lane (added by queue_put)
        self.queue_put(slot, mslot, word, xr, meta, meta_or=((2 * a) << 9) | (suspect << 15) | (tie << 8))

    # ---- pack one group of 64 pieces: RAW slot i -> packed word in register dst; then reload the slot ----
    def pack_group(self, i, dst):
        p = self.p
        r = V_RAW + 4 * i
        t = [V_PACK + 6 * (i % 3) + x for x in range(6)]  # three sets of scratch registers: the scheduler interleaves neighbouring groups
        # 2 x code of every byte: (ascii >> 1) & 3 = A 0, C 1, T / U 2, G 3 — the multiply-gather's input AND the index of the validity look-up:
        # the letter that code stands for (A, C, T, G), XORed with the byte, is zero or the case bit for exactly the bytes ACGTacgt.  (Round 4 looked
        # the letter up by byte & 7, which told U from T at the price of four more v_and per 16 bases; now a U is "dirty": its windows are K1f's,
        # which knows that U is a base — exact, slower for reads that are RNA.)
        x, e = t[4], t[5]
        for q in range(4):
            p.i("v_and_b32", v(t[q]), "0x06060606", v(r + q))
        for q in range(4):
            p.i("v_perm_b32", v(e), s(S_EXP0), v(V_EXP1), v(t[q]))
            if q == 0:
                p.i("v_xor_b32", v(x), v(e), v(r + q))
            else:
                self.bitop3(v(x), v(e), v(r + q), v(x), lambda a, b, c: (a ^ b) | c)
            if self.on("nomul"):
                p.i("v_lshlrev_b32", v(t[q]), 3, v(t[q]))
            else:
                p.i("v_mul_lo_u32", v(t[q]), v(t[q]), v(V_CMUL))
        p.i("v_perm_b32", v(t[0]), v(t[1]), v(t[0]), v(V_CPERMLO))
        p.i("v_perm_b32", v(t[2]), v(t[3]), v(t[2]), v(V_CPERMHI))
        p.i("v_or_b32", v(dst), v(t[0]), v(t[2]))
        p.i("v_and_b32", v(x), "0xdfdfdfdf", v(x))
        if self.on("nocarry"):
            p.i("v_or_b32", v(V_DN), v(V_DN), v(x))
        else:
            p.i("v_add_co_u32", v(t[5]), "vcc", -1, v(x))          # carry = (x != 0)
            p.i("v_addc_co_u32", v(V_DN), "vcc", v(V_DN), v(V_DN), "vcc")  # dirty bits, group m ends up at bit 31 - m
        self.load_slot(i)

    def issue_batch(self, b, soff_base):
        """loads of batch b (groups 8 b .. 8 b + 7) of the chunk at soffset soff_base: S_A / S_B as scratch soffsets"""
        p = self.p
        p.i("s_add_u32", s(S_A), s(soff_base), b * 8192)
        p.i("s_add_u32", s(S_B), s(soff_base), b * 8192 + 4096)
        self.load_slots()

    def pack_batch(self, b):
        """pack batch b of the chunk P into H0[8 b ..]; reload every slot with batch b + 1 of P, or — behind batch 3 — with batch 0 of
        the chunk Q (S_A / S_B hold the two soffsets: the caller of batch 3 has pointed S_DESC / S_CC at Q, or at any valid chunk)"""
        p = self.p
        skip, real = self.lbl("pk_skip"), self.lbl("pk_real")
        self.probe(0)
        if b < 3:
            p.i("s_add_u32", s(S_A), s(S_PSOFF), (b + 1) * 8192)
        else:
            p.i("s_mov_b32", s(S_A), s(S_CC))
        p.i("s_add_u32", s(S_B), s(S_A), 4096)
        p.i("s_cmp_eq_u32", s(S_PREAL), 1)
        notreal = self.lbl("pk_none")
        p.i("s_cbranch_scc0", "@" + notreal)

        def cold_none(notreal=notreal, skip=skip, b=b):
            p.label(notreal)
            for i in range(8):  # a chunk that does not exist: 'A's
                p.i("v_mov_b32", v(V_H0 + 8 * b + i), 0)
            if b == 3:          # the next chunk's first loads all the same
                self.load_slots()
            p.i("s_branch", "@" + skip)
        self.cold.append(cold_none)
        p.label(real)
        # Eight loads are in flight, issued in slot order, and loads return in order: when at most four vector-memory operations are outstanding
        # the first four slots have arrived — and again, behind their four reloads, the other four.  vmcnt(0) would also wait for every STORE a
        # resolve pass has just issued (hit log, suspects: stores count in vmcnt on gfx9 and take a microsecond to be acknowledged).
        p.i("s_waitcnt", "vmcnt(4)")
        if self.on("nopack"):
            p.i("s_branch", "@" + skip)
        for i in range(8):
            if i == 4:
                p.i("s_waitcnt", "vmcnt(4)")
            self.pack_group(i, V_H0 + 8 * b + i)
        p.label(skip)
        self.probe(1)

    # ---- 32 x 32 bit transpose of the packed words in H0 into the planes I, in two parts (round 5) ----
    # The two byte-level stages (J = 16, 8: v_perm) run at the end of the block and leave I QUARTER-MAJOR: I[8 q + i] holds, in byte t, the packed
    # byte (4 bases) of quarter q of the read 64 (i + 8 t) + lane — exactly what one quarter-slot of the ring stores.  The three bit-level stages of
    # quarter q (J = 4, 2, 1 stay inside the 8 registers of a quarter, and inside a byte) run in quarter_enter(q), right behind the ring write and
    # before the walk takes in the first base of that quarter: the packed bytes of a chunk wait in the registers they will be planes in, so the ring
    # in LDS never holds more than the 4 j + 5 quarters the 4 windows of a quarter span (round 4: three whole chunks, 24 KiB -> 18 KiB per wave).
    def perm_rotate(self):
        """(H0, H1, I) <- (H1, I, quarter-major bytes of the packed words in H0): the first stage reads H0 into the temps, which frees H0 for H1's planes
        and H1 for I's; the second stage lands in I"""
        p = self.p
        A = [V_H0 + i for i in range(32)]
        B = [V_XPOSE + i for i in range(32)]
        O = [V_I + i for i in range(32)]
        for kk in range(32):  # J = 16: A -> B
            if kk & 16 == 0:
                p.i("v_perm_b32", v(B[kk]), v(A[kk + 16]), v(A[kk]), v(V_CP16A))
                p.i("v_perm_b32", v(B[kk + 16]), v(A[kk + 16]), v(A[kk]), v(V_CP16B))
        self.shift_planes()
        for kk in range(32):  # J = 8: B -> O
            if kk & 8 == 0:
                p.i("v_perm_b32", v(O[kk]), v(B[kk + 8]), v(B[kk]), v(V_CP8A))
                p.i("v_perm_b32", v(O[kk + 8]), v(B[kk + 8]), v(B[kk]), v(V_CP8B))

    def transpose_quarter(self, q):
        """I[8 q .. 8 q + 7]: quarter-major bytes -> the 8 planes of the bases 4 q .. 4 q + 3 (temps: V_XPOSE .. V_XPOSE + 7)"""
        p = self.p
        O = [V_I + 8 * q + i for i in range(8)]
        n = 0
        for J, msk in ((4, V_CM4), (2, V_CM2), (1, V_CM1)):  # in place: O[k] = bfi(m, x, y << J), O[k+J] = bfi(m, x >> J, y)
            for kk in range(8):
                if kk & J == 0:
                    x, y = O[kk], O[kk + J]
                    b0, b1 = V_XPOSE + 2 * (n % 4), V_XPOSE + 2 * (n % 4) + 1  # (four pairs of temps: the pairs of a stage are independent of each other)
                    n += 1
                    p.i("v_lshlrev_b32", v(b0), J, v(y))
                    p.i("v_lshrrev_b32", v(b1), J, v(x))
                    # (a bit-select as v_bitop3: two waves of a SIMD overlap those, v_bfi_b32 they take turns for)
                    self.bitop3(v(x), v(msk), v(x), v(b0), lambda m, a, b: (m & a) | ((1 ^ m) & b))
                    self.bitop3(v(y), v(msk), v(b1), v(y), lambda m, a, b: (m & a) | ((1 ^ m) & b))

    def drain(self):
        """resolve passes until the queue is empty"""
        p = self.p
        drain, drained = self.lbl("drain"), self.lbl("drained")
        p.i("s_bitset1_b32", s(S_USELOG), F_DRAIN)             # "the queue is being emptied", read by the pass
        p.label(drain)
        p.i("s_cmp_eq_u32", s(S_QTAIL4), s(S_QHEAD4))
        p.i("s_cbranch_scc1", "@" + drained)
        self.call("pass")
        p.i("s_branch", "@" + drain)
        p.label(drained)
        p.i("s_bitset0_b32", s(S_USELOG), F_DRAIN)

    def quarter_enter(self, q):
        """before step 4 q of block n.  The 4 windows of the coming quarter start in quarter q of chunk n - 1 - j and end, at the latest, in quarter q of
        chunk n: 4 j + 5 quarters.  Quarter q of chunk n takes the slot of quarter q - 1 of chunk n - 1 - j, which only the windows of the steps behind
        us needed — so the queue is emptied first (q = 0: the end of the block has done that).  A resolve pass therefore only ever sees candidates of
        ONE quarter, and S_RQ[0 .. 4 j + 4] are the slots of the bytes of their windows, in order."""
        p = self.p
        if q:
            self.drain()
            self.probe(0)
        p.i("s_mov_b32", s(S_A), s(S_RQ[0]))
        for i in range(self.rq - 1):
            p.i("s_mov_b32", s(S_RQ[i]), s(S_RQ[i + 1]))
        p.i("s_mov_b32", s(S_RQ[self.rq - 1]), s(S_A))
        p.i("v_add_u32", v(V_MISC + 2), s(S_A), v(V_LANE4))
        for i in range(0, 8, 2):  # (offsets in units of 64 dwords: the slot's rows are 256 bytes apart)
            p.i("ds_write2st64_b32", v(V_MISC + 2), v(V_I + 8 * q + i), v(V_I + 8 * q + i + 1), mods=f"offset0:{i} offset1:{i + 1}")
        self.transpose_quarter(q)
        self.probe(3)

    # ---- the resolve pass (subroutine), in six stages; its registers: class PS (k1h_regs.py) ------------------------
    def emit_pass(self):
        self.pass_take_items()
        self.pass_window()
        self.pass_key()
        self.pass_log()
        self.pass_suspects()
        self.pass_logswitch()

    def pass_take_items(self):
        """queue -> lanes.  Leaves: exec = the lanes with an item; per lane PS.m = the read group of the candidate being resolved (lowest set bit of the
        hit word), PS.y = the item's meta, PS.tb = its strand; S_CC = the number of lanes.  What is left of a hit word is back in the queue."""
        p = self.p
        m, rest, col, tb, t1 = PS.m, PS.rest, PS.col, PS.tb, PS.t1
        p.label("pass")
        self.probe(0)
        # A resolving wave goes first on its SIMD: the pass is chains of LDS round trips and slow-class VALU instructions (v_bfe, v_lshl_add, v_perm
        # class: no overlap with the other wave's instructions, profiles/r05_ubench_op_classes.txt), the other wave of the SIMD is most likely walking
        # (full-rate v_bitop3 that fills any gap).  -4 % hash time (profiles/r05_k1h_priority_ab.txt); s_setprio around every run of slow-class
        # instructions gives the same, raising the WALK's priority nothing.
        if not self.on("noprio"):
            p.i("s_setprio", 3)
        if self.on("nopass"):
            p.i("s_mov_b32", s(S_QHEAD4), s(S_QTAIL4))
            self.ret()
        # Items -> lanes, in rounds: the first round takes min(64, count) items.  A word with more than one candidate goes back to the END of the queue
        # with its lowest bit cleared; when the round has taken everything the queue held, those words are the only items left and the lanes that
        # are still idle take them in the next round (and so on for third candidates).  Without this a queue that has to be EMPTIED — before every
        # quarter of a block, quarter_enter — would end in passes of a handful of second and third candidates: 13.9 passes per block measured
        # against 8.6 with whole-chunk ring slots; with it a quarter's ~110 items are two passes.
        x, zr = PS.lo, PS.hi                                  # the item's hit word and reverse-strand mask (until the requeue below: lo / hi are free until the window's bytes are in)
        y = PS.y                                              # its meta (16 bits)
        p.i("s_mov_b32", s(S_CC), 0)                          # lanes filled so far
        p.label("passload")
        p.i("s_sub_u32", s(S_N), s(S_QTAIL4), s(S_QHEAD4))
        p.i("s_lshr_b32", s(S_N), s(S_N), 2)
        p.i("s_sub_u32", s(S_B), 64, s(S_CC))
        p.i("s_min_u32", s(S_N), s(S_N), s(S_B))
        p.i("s_bfm_b64", "exec", s(S_N), s(S_CC))
        p.i("s_cmp_eq_u32", s(S_N), 64)
        p.i("s_cselect_b64", "exec", -1, "exec")
        p.i("s_lshl_b32", s(S_B), s(S_CC), 2)
        p.i("s_sub_u32", s(S_B), s(S_QHEAD4), s(S_B))        # lane l takes item l - filled
        p.i("v_add_u32", v(t1), s(S_B), v(V_LANE4))
        p.i("v_and_b32", v(t1), v(V_CQMASK4), v(t1))
        p.i("v_lshrrev_b32", v(m), 1, v(t1))
        p.i("v_add_u32", v(m), v(V_QBASE), v(m))
        p.i("v_add_u32", v(t1), v(V_QBASE), v(t1))
        p.i("ds_read2_b32", vr(x, 2), v(t1), mods=f"offset0:0 offset1:{QSTRIDE}")
        p.i("ds_read_u16", v(y), v(m), mods=f"offset:{Q_META_OFF}")
        p.i("s_lshl2_add_u32", s(S_QHEAD4), s(S_N), s(S_QHEAD4))
        p.i("s_add_u32", s(S_CC), s(S_CC), s(S_N))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("v_ffbl_b32", v(m), v(x))
        p.i("v_add_u32", v(rest), -1, v(x))
        p.i("v_and_b32", v(rest), v(rest), v(x))
        p.i("v_lshrrev_b32", v(tb), v(m), v(zr))
        p.i("v_and_b32", v(tb), 1, v(tb))                     # strand of the read being resolved
        # ---- what is left of each word goes to the back of the queue (exec = the items of this round; a spent word goes to the dummy slot) ----
        p.i("v_cmp_ne_u32_e32", "vcc", 0, v(rest))
        p.i("s_bcnt1_i32_b64", s(S_A), "vcc")
        self.queue_put(t1, col, rest, zr, y)
        self.unless_flag(F_DRAIN, "passloaded")               # another round?  only when the queue is being emptied (drain: a pass run for want of room
        #                                                       leaves the words it puts back to the next one, which costs nothing) ...
        p.i("s_cmp_lt_u32", s(S_CC), 64)                      # ... with idle lanes ...
        p.i("s_cbranch_scc0", "@passloaded")
        p.i("s_cmp_lg_u32", s(S_QTAIL4), s(S_QHEAD4))         # ... and items (then the queue holds nothing but the words this round has put back)
        p.i("s_cbranch_scc1", "@passload")
        p.label("passloaded")
        p.i("s_bfm_b64", "exec", s(S_CC), 0)
        p.i("s_cmp_eq_u32", s(S_CC), 64)
        p.i("s_cselect_b64", "exec", -1, "exec")

    def pass_window(self):
        """the candidate's window from the ring.  Reads PS.m, PS.y, PS.tb, S_RQ; leaves its 2-bit codes in PS.hi:PS.lo (base 0 in the lowest bits) and the
        LDS address of its strand's table in PS.tb"""
        p = self.p
        m, col, a0, lo, hi, tb, t1, fld, y = PS.m, PS.col, PS.a0, PS.lo, PS.hi, PS.tb, PS.t1, PS.fld, PS.y
        # the window's bytes: byte i lies in quarter-slot S_RQ[i], row m & 7, lane, byte m >> 3 (every byte is loaded into a register of its own,
        # zero-extended: a d16 load keeps or clears the other half of its register depending on the ECC mode of the part)
        nby = self.nby
        addr = fld[:nby]                                      # (address registers now, fields later)
        byt = [a0, PS.a1, PS.a2, lo, hi, PS.key, PS.key1, fld[9], fld[10]][:nby]
        p.i("v_and_b32", v(col), 0xff, v(y))                  # 4 x lane
        p.i("v_lshl_or_b32", v(a0), v(m), 11, v(m))
        p.i("v_lshrrev_b32", v(a0), 3, v(a0))
        p.i("v_and_or_b32", v(col), v(a0), v(V_CBYTE), v(col))  # (m & 7) << 8 | 4 lane | m >> 3
        for i in range(nby):
            p.i("v_add_u32", v(addr[i]), s(S_RQ[i]), v(col))
        for i in range(nby):
            p.i("ds_read_u8", v(byt[i]), v(addr[i]))
        p.i("v_bfe_u32", v(t1), v(y), 9, 3)                   # shift = 2 x (window start within its quarter)
        p.i("v_mul_u32_u24", v(tb), hex(self.ng * 256), v(tb))
        p.i("v_add_u32", v(tb), TABLE_OFF, v(tb))             # the strand's table
        p.i("s_waitcnt", "lgkmcnt(0)")

        def word(bs):
            """bs[0] = the bytes bs (registers, zero-extended) as one dword, lowest first"""
            if len(bs) >= 2:
                p.i("v_lshl_or_b32", v(bs[0]), v(bs[1]), 8, v(bs[0]))
            if len(bs) == 4:
                p.i("v_lshl_or_b32", v(bs[2]), v(bs[3]), 8, v(bs[2]))
            if len(bs) >= 3:
                p.i("v_lshl_or_b32", v(bs[0]), v(bs[2]), 16, v(bs[0]))
            return bs[0]
        w0 = word(byt[0:4])
        w1 = word(byt[4:8]) if nby > 4 else None
        w2 = byt[8] if nby > 8 else None
        if w1 is None:
            p.i("v_lshrrev_b32", v(lo), v(t1), v(w0))         # (k <= 13: the window lies in four bytes)
        else:
            p.i("v_alignbit_b32", v(lo), v(w1), v(w0), v(t1))  # bases 0 .. 15 of the window
            if self.k > 16:
                if w2 is None:
                    p.i("v_lshrrev_b32", v(hi), v(t1), v(w1))
                else:
                    p.i("v_alignbit_b32", v(hi), v(w2), v(w1), v(t1))  # bases 16 .. 31

    def pass_key(self):
        """table look-ups.  Reads PS.hi:PS.lo, PS.tb, PS.y; leaves the counter index in PS.key and in PS.sflag 0: a hit to log, bit 0: suspect, bit 1: no hit"""
        p = self.p
        lo, hi, mid, tb, key, fld, y = PS.lo, PS.hi, PS.mid, PS.tb, PS.key, PS.fld, PS.y
        # 3 bases per look-up: field g = bits [6 g, 6 g + 6) of hi:lo
        for g in range(self.ng):
            bit = 6 * g
            nb = min(3, self.k - 3 * g) * 2
            if bit + nb <= 32:
                src, off = lo, bit
            elif bit >= 32:
                src, off = hi, bit - 32
            else:
                if bit == 30:
                    p.i("v_alignbit_b32", v(mid), v(hi), v(lo), 30)
                src, off = mid, bit - 30
            p.i("v_bfe_u32", v(fld[g]), v(src), off, nb)
            p.i("v_lshl_add_u32", v(fld[g]), v(fld[g]), 2, v(tb))
        for g in range(self.ng):
            p.i("ds_read_b32", v(fld[g]), v(fld[g]), mods=f"offset:{g * 256}")
        p.i("s_waitcnt", "lgkmcnt(0)")
        words = list(fld[: self.ng])
        while len(words) > 1:
            if len(words) >= 3:
                a, b, c = words[:3]
                self.bitop3(v(a), v(a), v(b), v(c), lambda q, r, t: q ^ r ^ t)
                words = words[3:] + [a]
            else:
                a, b = words
                p.i("v_xor_b32", v(a), v(a), v(b))
                words = [a]
        w = words[0]
        p.i("v_and_b32", v(key), s(S_RMASK2), v(w))          # low rBits bits + the sample bit right above them
        p.i("v_add_u32", v(key), s(S_KEYBASE), v(key))
        sflag = PS.sflag                                      # (the ring words are spent)
        p.i("v_bfe_u32", v(sflag), v(y), 15, 1)
        if self.sb != 7:
            # s_bits >= 8: the walk only saw the 8-bit prefixes of ntComp's patterns; the table word carries the s_bits - 7 hash bits below them
            # (bits 55 .. 63 - s_bits, above the sample bit).  Sample 1 (0 1..1) needs all but the lowest of them set, sample 0 (0..0 1)
            # exactly the lowest; S_SPARE = 2^(s_bits - 7) - 1
            smp, ext = PS.a1, PS.a2
            p.i("s_bcnt1_i32_b32", s(S_B), s(S_RMASK2))      # r_bits + 1
            p.i("v_lshrrev_b32", v(ext), s(S_B), v(w))
            p.i("s_sub_u32", s(S_B), s(S_B), 1)
            p.i("v_lshrrev_b32", v(smp), s(S_B), v(w))
            p.i("v_and_b32", v(smp), 1, v(smp))
            p.i("v_or_b32", v(mid), 1, v(ext))
            p.i("v_cmp_ne_u32_e64", sr(S_TMP, 2), s(S_SPARE), v(mid))   # sample 1 fails
            p.i("v_cmp_ne_u32_e32", "vcc", 1, v(ext))                   # sample 0 fails
            p.i("v_cndmask_b32_e64", v(mid), 0, 2, sr(S_TMP, 2))
            p.i("v_cndmask_b32_e64", v(ext), 0, 2, "vcc")
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(smp))
            p.i("v_cndmask_b32_e64", v(mid), v(ext), v(mid), "vcc")     # 2 where the candidate's own pattern fails
            p.i("v_or_b32", v(sflag), v(sflag), v(mid))

    def pass_log(self):
        """clean hits (PS.sflag == 0): PS.key -> the hit log, or — no log — ntComp's increment as a device atomic.  Leaves vcc = the suspects"""
        p = self.p
        lo, key, key1, t1, fld, sflag = PS.lo, PS.key, PS.key1, PS.t1, PS.fld, PS.sflag
        nolog, logged = self.lbl("nolog"), self.lbl("logged")
        p.label("logswitch_back")
        if self.sb == 7:
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(sflag))       # vcc = suspects
        else:
            p.i("v_and_b32", v(t1), 1, v(sflag))
            p.i("v_cmp_ne_u32_e32", "vcc", 0, v(t1))
        p.i("v_cmp_eq_u32_e64", sr(S_TMP, 2), 0, v(sflag))    # S_TMP = hits to log
        p.i("s_bcnt1_i32_b64", s(S_B), sr(S_TMP, 2))
        self.unless_flag(F_USELOG, nolog)
        p.i("s_lshl2_add_u32", s(S_A), s(S_B), s(S_LFILL4))
        p.i("s_cmp_le_u32", s(S_A), s(S_LOGCAP4))
        p.i("s_cbranch_scc0", "@logswitch")
        self.mbcnt(t1, s(S_TMP), s(S_TMP + 1))
        p.i("v_lshl_add_u32", v(t1), v(t1), 2, s(S_LFILL4))
        p.i("s_mov_b64", "exec", sr(S_TMP, 2))
        p.i("global_store_dword", v(t1), v(key), sr(S_LOGBASE, 2))
        p.i("s_mov_b32", s(S_LFILL4), s(S_A))
        p.i("s_branch", "@" + logged)
        p.label(nolog)
        p.label("direct")
        p.i("s_mov_b64", "exec", sr(S_TMP, 2))
        p.i("v_mov_b32", v(key1), 0)
        p.i("v_lshl_add_u64", vr(lo, 2), vr(key, 2), 2, sr(S_SK, 2))
        p.i("global_atomic_add", vr(lo, 2), v(V_ONE), "off")
        # (round 6) the sketch is no longer what the last reset or apply left: the engine's "direct atomics happened" word — the first apply behind a reset
        # WRITES its counts instead of adding them (ntc_apply.hip, count_kernel) unless this word says otherwise.  Rare path: engines without a log
        # (their pointer is NULL) and waves that ran out of log regions.
        skipflag = self.lbl("skipflag")
        self.karg_load(S_TMP, "sk_dirty", wait=True)
        p.i("s_cmp_eq_u64", sr(S_TMP, 2), 0)
        p.i("s_cbranch_scc1", "@" + skipflag)
        p.i("v_mov_b32", v(fld[2]), 0)
        p.i("global_store_dword", v(fld[2]), v(V_ONE), sr(S_TMP, 2))
        p.label(skipflag)
        p.label(logged)

    def pass_suspects(self):
        """suspects (vcc): (key, tile, read | window << 11, marks) -> this wave's region of the suspect list; then the pass returns, exec = all lanes"""
        p = self.p
        m, key, t1, fld, sflag, y = PS.m, PS.key, PS.t1, PS.fld, PS.sflag, PS.y
        nosus, susfull = self.lbl("nosus"), self.lbl("susfull")
        p.i("s_cbranch_vccz", "@" + nosus)
        p.i("s_mov_b64", "exec", "vcc")
        p.i("s_bcnt1_i32_b64", s(S_B), "vcc")
        p.i("s_lshl_b32", s(S_B), s(S_B), 4)
        p.i("s_add_u32", s(S_A), s(S_SUSOFF), s(S_B))
        p.i("s_cmp_le_u32", s(S_A), s(S_SUSCAP))
        p.i("s_cbranch_scc0", "@" + susfull)
        self.mbcnt(t1, "vcc_lo", "vcc_hi")
        p.i("v_lshl_add_u32", v(t1), v(t1), 4, s(S_SUSOFF))
        sx = fld[1]                                           # four consecutive registers from an even one: the entry
        assert sx % 2 == 0
        p.i("v_mov_b32", v(sx), v(key))
        p.i("v_mov_b32", v(sx + 1), s(S_WT))
        p.i("s_sub_u32", s(S_B), s(S_WN), 1 + self.j)          # the block's windows start in chunk n - 1 - j
        p.i("s_lshl_b32", s(S_B), s(S_B), 4)
        p.i("v_bfe_u32", v(sx + 2), v(y), 10, 4)
        p.i("v_add_u32", v(sx + 2), s(S_B), v(sx + 2))
        p.i("v_bfe_u32", v(sx + 3), v(y), 2, 6)               # lane
        p.i("v_lshl_or_b32", v(sx + 3), v(m), 6, v(sx + 3))   # read of the tile = 64 m + lane
        p.i("v_lshl_or_b32", v(sx + 2), v(sx + 2), 11, v(sx + 3))
        # marks: 2 = the candidate's own pattern fails below the walk's 8-bit prefix (s_bits >= 8: no hit, whatever its bytes); 4 = a tie (K1f re-derives
        # both strands from the bytes); bits 4 .. 6 = the read's dirty bits in the block's three chunks n - 2 .. n (the dirty words live in the lane the
        # item came from: fetched across lanes) — with them K1f reads nothing but the entry and the window's dirty pieces
        dl, d0, d1, d2 = fld[5], fld[6], fld[7], fld[8]
        p.i("s_mov_b64", sr(S_TMP, 2), "exec")
        p.i("s_mov_b64", "exec", -1)                           # (a lane that is switched off would hand out nothing)
        p.i("v_and_b32", v(dl), 0xff, v(y))                   # 4 x the item's lane
        dsrc = (V_D0, V_D1, V_D2) if self.j == 1 else (V_D1, V_D2)   # the chunks the window starts in and the ones behind it
        dregs = (d0, d1, d2)[:len(dsrc)]
        for dj, src in zip(dregs, dsrc):
            p.i("ds_bpermute_b32", v(dj), v(dl), v(src))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_mov_b64", "exec", sr(S_TMP, 2))
        p.i("v_and_b32", v(sx + 3), 2, v(sflag))
        p.i("v_bfe_u32", v(dl), v(y), 8, 1)
        p.i("v_lshl_or_b32", v(sx + 3), v(dl), 2, v(sx + 3))
        for j, dj in enumerate(dregs):
            p.i("v_lshrrev_b32", v(dj), v(m), v(dj))
            p.i("v_and_b32", v(dj), 1, v(dj))
            p.i("v_lshl_or_b32", v(sx + 3), v(dj), 4 + j, v(sx + 3))
        p.i("global_store_dwordx4", v(t1), vr(sx, 4), sr(S_SUS, 2))
        p.i("s_nop", 1)                                       # (a 128-bit store reads its data a little after it issues)
        p.label(susfull)                                      # no room: the count runs past the capacity, which K1f reads as "walk everything"
        p.i("s_mov_b32", s(S_SUSOFF), s(S_A))
        p.label(nosus)
        p.i("s_mov_b64", "exec", -1)
        p.i("s_waitcnt", "lgkmcnt(0)")
        self.probe(2)
        if not self.on("noprio"):
            p.i("s_setprio", 0)
        self.ret()

    def pass_logswitch(self):
        """rare, out of line: the log region is full — this wave's next region, or device atomics from here on; back to pass_log with exec restored"""
        p = self.p
        p.label("logswitch")
        p.i("s_mov_b64", "vcc", "exec")
        self.store_log_fill()
        p.i("s_add_u32", s(S_LREG), s(S_LREG), s(S_NWAVES))
        p.i("s_cmp_lt_u32", s(S_LREG), s(S_LOGREG))
        ok = self.lbl("lsw_ok")
        p.i("s_cbranch_scc1", "@" + ok)
        p.i("s_bitset0_b32", s(S_USELOG), F_USELOG)           # out of regions: ntComp's increment as device atomics from here on
        p.i("s_mov_b64", "exec", "vcc")
        p.i("s_branch", "@logswitch_back")
        p.label(ok)
        self.load_log_region()
        p.i("s_mov_b64", "exec", "vcc")
        p.i("s_branch", "@logswitch_back")

    def store_log_fill(self):
        """log_fill[LREG] = LFILL (one lane); scratch: PS.fld[1], PS.fld[2] (free wherever this is called: they hold look-up fields or nothing)"""
        p = self.p
        T = PS.fld[1]
        p.i("s_mov_b64", "exec", 1)
        p.i("s_lshl_b32", s(S_B), s(S_LREG), 2)
        p.i("s_lshr_b32", s(S_CC), s(S_LFILL4), 2)
        p.i("v_mov_b32", v(T), s(S_B))
        p.i("v_mov_b32", v(T + 1), s(S_CC))
        self.karg_load(S_TMP, "log_fill", wait=True)
        p.i("global_store_dword", v(T), v(T + 1), sr(S_TMP, 2))
        p.i("s_mov_b64", "exec", -1)

    def load_log_region(self):
        """LFILL4 and the buffer descriptor of region LREG"""
        p = self.p
        p.i("s_lshl_b32", s(S_B), s(S_LREG), 2)
        self.karg_load(S_TMP, "log_fill")
        self.karg_load(S_LOGBASE, "log")
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_load_dword", s(S_LFILL4), sr(S_TMP, 2), s(S_B))
        self.mul64(S_TMP, S_TMP + 1, S_LREG, S_LOGCAP4)
        self.add64(S_LOGBASE, S_LOGBASE, s(S_TMP), s(S_TMP + 1))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_lshl_b32", s(S_LFILL4), s(S_LFILL4), 2)

    # ---- scalar helpers: chunk cursor ----------------------------------------------------------------------
    def cursor_next(self, t, n, real):
        """(t, n) -> the next chunk of the wave's flat sequence; real = it exists (n < C and t < n_tiles)"""
        p = self.p
        same = self.lbl("cur")
        p.i("s_add_u32", s(n), s(n), 1)
        p.i("s_cmp_lt_u32", s(n), s(S_NB))
        p.i("s_cbranch_scc1", "@" + same)
        p.i("s_mov_b32", s(n), 0)
        p.i("s_add_u32", s(t), s(t), 1)
        p.label(same)
        p.i("s_cmp_lt_u32", s(n), s(S_C))
        p.i("s_cselect_b32", s(real), 1, 0)
        p.i("s_cmp_lt_u32", s(t), s(S_NTILES))
        p.i("s_cselect_b32", s(real), s(real), 0)

    def set_desc(self, t):
        """S_DESC = slots of tile t"""
        self.mul64(S_TMP, S_TMP + 1, t, S_CHUNKB)
        self.add64(S_DESC, S_TILES, s(S_TMP), s(S_TMP + 1))

    # ---- the whole kernel body: build() strings the stages below together ----------------------------------------------
    def build(self, emu=False):
        p = self.p
        # inputs -> fixed registers (operands %0 .. are the compiler's; the emulator finds them in s0 ..)
        self.inp = {name: (s(i) if emu else f"%{i}") for i, name in enumerate(INPUTS)}
        self.prologue()
        self.log_setup()
        self.first_share()
        p.label("iter")
        self.chunk_loop()
        self.end_of_block()
        self.advance()
        self.new_tile()
        self.block_setup()
        p.i("s_branch", "@iter")
        for frag in self.cold:                                   # out-of-line: the rare sides of the loop's tests
            frag()
        self.cold = []
        self.epilogue()
        self.emit_pass()
        self.emit_tail_step()
        p.label("end")
        if not self.on("nosched"):
            schedule(p)
        phase_fix(p, self.exp)
        return p

    def prologue(self):
        """the asm statement's inputs and the kernel arguments -> S_KARG, S_WT (the wave's number, until the first block), S_NWAVES, the pointers S_TILES ..
        S_SUS (this wave's region), the geometry S_NTILES .. S_LOGCAP4 (x 4), S_SUSCAP (bytes), S_CHUNKB, S_NB; S_USELOG = the ragged bit; S_DESC's constant
        half; VCONST and the lane constants V_LANE4 .. V_EXP1; the ring's slots S_RQ and an empty queue; F1 = 0"""
        p = self.p
        inp, phi = self.inp, self.phi
        p.i("s_mov_b32", s(S_KARG), inp["karg_lo"])
        p.i("s_mov_b32", s(S_KARG + 1), inp["karg_hi"])
        p.i("s_mov_b32", s(S_WT), inp["wave_gid"])
        p.i("s_lshl_b32", s(S_A), s(S_WT), 2)
        p.i("v_mov_b32", v(V_WAVE4), s(S_A))
        p.i("s_mov_b32", s(S_NWAVES), inp["n_waves"])
        p.i("s_mov_b32", s(S_RQ[0]), inp["lds_wbase"])
        for reg, name in ((S_TILES, "tiles"), (S_SK, "sketch0"), (S_DIRTY, "dirty"), (S_TIE, "tie"), (S_SUS, "sus")):
            self.karg_load(reg, name)
        for reg, name in ((S_NTILES, "n_tiles"), (S_C, "n_chunks"), (S_L, "read_len"), (S_NVLAST, "nv_last"), (S_KEYBASE, "key_base"), (S_RMASK2, "rmask2"),
                          (S_LOGREG, "log_regions"), (S_LOGCAP4, "log_region_cap"), (S_SUSCAP, "sus_cap")):
            self.karg_load(reg, name, n=1)
        p.i("s_waitcnt", "lgkmcnt(0)")
        self.karg_load(S_TMP, "tails", wait=True)
        p.i("s_cmp_lg_u64", sr(S_TMP, 2), 0)
        p.i("s_cselect_b32", s(S_USELOG), 1 << F_RAGGED, 0)   # (bit F_USELOG joins it below)
        p.i("s_lshl_b32", s(S_LOGCAP4), s(S_LOGCAP4), 2)
        p.i("s_lshl_b32", s(S_SUSCAP), s(S_SUSCAP), 4)         # bytes
        self.mul64(S_A, S_B, S_WT, S_SUSCAP)
        self.add64(S_SUS, S_SUS, s(S_A), s(S_B))
        p.i("s_mov_b32", s(S_SUSOFF), 0)
        p.i("s_mov_b32", s(S_EXP0), "0xff47ff54")         # validity look-up, codes 2 and 3: T, G
        if self.sb != 7:
            self.karg_load(S_SPARE, "s_bits", n=1, wait=True)
            p.i("s_sub_u32", s(S_SPARE), s(S_SPARE), 7)
            p.i("s_bfm_b32", s(S_SPARE), s(S_SPARE), 0)       # 2^(s_bits - 7) - 1
        for reg, val in VCONST:
            p.i("v_mov_b32", v(reg), hex(val))
        p.i("s_mov_b32", s(S_DESC + 2), "0x7fffffff")          # records: a tile's slots (C x 32 KiB) always fit
        p.i("s_mov_b32", s(S_DESC + 3), "0x00020000")
        p.i("s_lshl_b32", s(S_CHUNKB), s(S_C), 15)             # bytes of one tile
        # lane constants
        self.mbcnt(V_LANE4, -1, -1)
        p.i("v_lshlrev_b32", v(V_LANE16), 4, v(V_LANE4))
        p.i("v_lshlrev_b32", v(V_LANE4), 2, v(V_LANE4))
        p.i("v_mov_b32", v(V_ONE), 1)
        p.i("v_mov_b32", v(V_EXP1), "0xff43ff41")         # codes 0 and 1: A, C
        p.i("s_add_u32", s(S_A), s(S_RQ[0]), RING_BYTES)
        p.i("v_mov_b32", v(V_QBASE), s(S_A))
        p.i("v_mov_b32", v(V_QDUMMY), QCAP * 4)
        for i in range(1, self.rq):
            p.i("s_add_u32", s(S_RQ[i]), s(S_RQ[0]), i * QSLOT)
        p.i("s_mov_b32", s(S_QHEAD4), 0)
        p.i("s_mov_b32", s(S_QTAIL4), 0)
        p.i("s_mov_b64", sr(S_F1ACC, 2), 0)
        if self.on("timers"):
            p.i("s_mov_b32", s(S_SPARE), 0)
        # geometry: W = L - k + 1, NB = ((L - 1 + 16 - phi) >> 4) + 1
        p.i("s_add_u32", s(S_NB), s(S_L), 15 - phi)
        p.i("s_lshr_b32", s(S_NB), s(S_NB), 4)
        p.i("s_add_u32", s(S_NB), s(S_NB), 1)

    def log_setup(self):
        """hit log: this wave's first region.  Reads S_WT (the wave's number), S_LOGREG; leaves S_LREG, S_LFILL4, S_LOGBASE and bit F_USELOG of S_USELOG"""
        p = self.p
        p.i("s_cmp_lg_u32", s(S_LOGREG), 0)
        p.i("s_cselect_b32", s(S_A), 1, 0)
        p.i("s_mov_b32", s(S_LREG), s(S_WT))
        p.i("s_mov_b32", s(S_LFILL4), 0)
        p.i("s_cmp_lt_u32", s(S_LREG), s(S_LOGREG))
        p.i("s_cselect_b32", s(S_A), s(S_A), 0)
        p.i("s_or_b32", s(S_USELOG), s(S_USELOG), s(S_A))
        nolog0 = self.lbl("nolog0")
        self.unless_flag(F_USELOG, nolog0)
        self.load_log_region()
        p.label(nolog0)

    def first_share(self):
        """the wave's share of the blocks and its first loads.  Leaves S_F0, S_FEND (the blocks it owns), S_S0 (the first it walks), S_WF = S_S0 - 1, the
        cursors P (chunk to pack: S_PT, S_PN, S_PREAL, S_PSOFF) and Q (to load next), S_DESC -> P's tile with P's first batch of loads in flight,
        S_WN = -1 and an empty step mask (the first iteration is a dummy: it walks nothing and packs P), V_DN = V_TACC = V_CMASK = 0"""
        p = self.p
        inp = self.inp
        # This wave's share: the blocks of all tiles form one sequence (tile * NB + block); the wave owns [first_block, end_block) of it (the
        # kernel's prologue shares a workgroup's blocks out by where its waves sit: a wave alone on its SIMD gets through more than one of a pair)
        # — tiles are split wherever a boundary falls (19 tiles per CU over 6 waves are 4 rounds of whole tiles but 3.2 of blocks).
        # A wave that starts inside a tile first walks up to two blocks it does not own, masked: they fill the window (k - 1 <= 31 bases).
        self.karg_load(S_B, "nb_magic", n=1)
        p.i("s_mul_i32", s(S_CC), s(S_NTILES), s(S_NB))          # blocks of the batch
        p.i("s_mov_b32", s(S_F0), inp["first_block"])
        p.i("s_min_u32", s(S_FEND), inp["end_block"], s(S_CC))
        p.i("s_waitcnt", "lgkmcnt(0)")
        p.i("s_cmp_lt_u32", s(S_F0), s(S_FEND))
        p.i("s_cbranch_scc0", "@done")                           # nothing to walk: F1 += 0, no suspects
        p.i("s_mul_hi_u32", s(S_PT), s(S_F0), s(S_B))            # tile = F0 / NB with nb_magic = floor(2^32 / NB): never too large,
        p.i("s_mul_i32", s(S_A), s(S_PT), s(S_NB))
        p.i("s_sub_u32", s(S_PN), s(S_F0), s(S_A))               # block = F0 - tile NB ...
        fix, fixed = self.lbl("divfix"), self.lbl("divok")
        p.label(fix)
        p.i("s_cmp_lt_u32", s(S_PN), s(S_NB))
        p.i("s_cbranch_scc1", "@" + fixed)
        p.i("s_sub_u32", s(S_PN), s(S_PN), s(S_NB))              # ... corrected upwards
        p.i("s_add_u32", s(S_PT), s(S_PT), 1)
        p.i("s_branch", "@" + fix)
        p.label(fixed)
        p.i("s_min_u32", s(S_A), s(S_PN), 2)
        p.i("s_sub_u32", s(S_PN), s(S_PN), s(S_A))
        p.i("s_sub_u32", s(S_S0), s(S_F0), s(S_A))               # the first block walked
        p.i("s_sub_u32", s(S_WF), s(S_S0), 1)
        p.i("s_cmp_lt_u32", s(S_PN), s(S_C))
        p.i("s_cselect_b32", s(S_PREAL), 1, 0)
        p.i("s_mov_b32", s(S_QT), s(S_PT))
        p.i("s_mov_b32", s(S_QN), s(S_PN))
        self.cursor_next(S_QT, S_QN, S_QREAL)
        p.i("s_mov_b32", s(S_WN), -1)                           # the dummy iteration: nothing to walk
        p.i("s_mov_b32", s(S_STEPMASK), 0)
        self.set_desc(S_PT)
        p.i("s_lshl_b32", s(S_PSOFF), s(S_PN), 15)
        p.i("s_lshl_b32", s(S_QSOFF), s(S_QN), 15)
        p.i("v_mov_b32", v(V_DN), 0)
        p.i("v_mov_b32", v(V_TACC), 0)
        p.i("v_mov_b32", v(V_CMASK), 0)
        nofirst = self.lbl("nofirst")
        p.i("s_cmp_eq_u32", s(S_PREAL), 1)
        p.i("s_cbranch_scc0", "@" + nofirst)
        self.issue_batch(0, S_PSOFF)
        p.label(nofirst)

        if self.on("timers"):
            p.i("s_memtime", sr(S_TMP, 2))
            p.i("s_waitcnt", "lgkmcnt(0)")
            p.i("s_mov_b32", s(S_SUSCAP), s(S_TMP))
            p.i("s_mov_b64", sr(S_F1ACC, 2), 0)

    def chunk_loop(self):
        """the 16 steps of block W = (S_WT, S_WN): walk, test + push where S_STEPMASK says so, and between them the pack of chunk P into H0 (its loads
        replaced by the next batch's, at last by chunk Q's first).  Reads the state planes, H0 / H1 / I, the block's masks; leaves candidates in the queue,
        ties in V_TACC, P's packed words in H0 and its dirty bits in V_DN"""
        p = self.p
        for a in range(16):
            if a % 4 == 0:
                self.quarter_enter(a // 4)
            self.walk_step(a)
            # ("tailstep" names nothing: the call is kept because it numbers the labels behind it, and the output is pinned)
            skip, notstep, dostep, _reserved = self.lbl("nostep"), self.lbl("notstep"), self.lbl("dostep"), self.lbl("tailstep")
            p.i("s_bitcmp1_b32", s(S_STEPMASK), a)
            p.i("s_cbranch_scc0", "@" + notstep)
            if self.on("noflags"):
                p.i("s_branch", "@" + skip)
            p.label(dostep)
            self.flags_and_push(a)
            p.label(skip)

            def cold_tail(a=a, skip=skip, notstep=notstep, dostep=dostep):
                # a step the mask leaves out (a filling block, the steps behind the read) — or, in a ragged batch, one that ends in the reads' last piece
                p.label(notstep)
                p.i("s_bitcmp1_b32", s(S_STEPMASK), 16 + a)
                p.i("s_cbranch_scc0", "@" + skip)
                p.i("s_mov_b32", s(S_B), 4 * ((self.phi + a) & 15))   # the step ends at base 16 (C - 1) + d of the reads: d x 4
                self.call("tailsub")
                p.i("s_branch", "@" + dostep)
            self.cold.append(cold_tail)
            if a in (4, 8, 12):
                self.pack_batch(a // 4 - 1)
            if a == 15:
                if self.j == 1:  # the plane pair that leaves the window at the first step of the next block
                    p.i("v_mov_b32", v(V_CARRY0), v(V_H0 + 30))
                    p.i("v_mov_b32", v(V_CARRY1), v(V_H0 + 31))
                # the loads behind batch 3 belong to chunk Q: its tile's descriptor (P's loads are all issued); a chunk that does not
                # exist is replaced by the first chunk of the tile the descriptor points at (loaded, never packed)
                noq = self.lbl("noq")
                p.i("s_mov_b32", s(S_CC), 0)
                p.i("s_cmp_eq_u32", s(S_QREAL), 1)
                p.i("s_cbranch_scc0", "@" + noq)
                self.set_desc(S_QT)
                p.i("s_mov_b32", s(S_CC), s(S_QSOFF))
                p.label(noq)
                self.pack_batch(3)

    def end_of_block(self):
        """empties the queue (the next quarter_enter recycles the oldest quarter-slot of the ring); V_TACC -> tie[] and 0; V_DN -> dirty[]; the planes rotate:
        (H0, H1, I) <- (H1, I, P's packed words as quarter-major bytes) and (V_D0, V_D1, V_D2, V_DN) <- (V_D1, V_D2, V_DN, 0)"""
        p = self.p
        self.drain()
        self.probe(0)
        # -- tie bits of this block -> tie[(WT * NB + WN) * 64 + lane]
        notie = self.lbl("notie")
        p.i("s_add_u32", s(S_A), s(S_WF), 1)                    # (the dummy iteration of a wave that starts at block 0 has WF = -1)
        p.i("s_cmp_gt_u32", s(S_A), s(S_F0))
        p.i("s_cbranch_scc0", "@" + notie)
        p.i("s_lshl_b32", s(S_A), s(S_WF), 8)
        p.i("v_add_u32", v(V_MISC), s(S_A), v(V_LANE4))
        p.i("global_store_dword", v(V_MISC), v(V_TACC), sr(S_TIE, 2))
        p.label(notie)
        p.i("v_mov_b32", v(V_TACC), 0)
        # -- chunk P: dirty bits -> dirty[(PT * C + PN) * 64 + lane], packed words -> quarter-major bytes in I (ring and planes: quarter_enter)
        p.i("v_bfrev_b32", v(V_DN), v(V_DN))
        nopk = self.lbl("nopk")
        p.i("s_cmp_eq_u32", s(S_PREAL), 1)
        p.i("s_cbranch_scc0", "@" + nopk)
        p.i("s_mul_i32", s(S_A), s(S_PT), s(S_C))
        p.i("s_add_u32", s(S_A), s(S_A), s(S_PN))
        p.i("s_lshl_b32", s(S_A), s(S_A), 8)
        p.i("v_add_u32", v(V_MISC), s(S_A), v(V_LANE4))
        p.i("global_store_dword", v(V_MISC), v(V_DN), sr(S_DIRTY, 2))
        # -- rotate: planes (H0, H1, I) <- (H1, I, new), dirty words
        self.perm_rotate()
        rotated = self.lbl("rotated")
        p.i("s_branch", "@" + rotated)
        p.label(nopk)                                           # no chunk P (behind a tile's last one): its planes are all 'A'
        self.shift_planes()
        for i in range(32):
            p.i("v_mov_b32", v(V_I + i), 0)
        p.label(rotated)
        p.i("v_mov_b32", v(V_D0), v(V_D1))
        p.i("v_mov_b32", v(V_D1), v(V_D2))
        p.i("v_mov_b32", v(V_D2), v(V_DN))
        p.i("v_mov_b32", v(V_DN), 0)

    def advance(self):
        """the cursors move on: W <- P, P <- Q, Q <- next(Q); the kernel ends (-> done) behind the wave's last block"""
        p = self.p
        p.i("s_mov_b32", s(S_WT), s(S_PT))
        p.i("s_mov_b32", s(S_WN), s(S_PN))
        p.i("s_add_u32", s(S_WF), s(S_WF), 1)
        p.i("s_cmp_lt_u32", s(S_WF), s(S_FEND))
        p.i("s_cbranch_scc0", "@done")
        p.i("s_mov_b32", s(S_PT), s(S_QT))
        p.i("s_mov_b32", s(S_PN), s(S_QN))
        p.i("s_mov_b32", s(S_PREAL), s(S_QREAL))
        p.i("s_mov_b32", s(S_PSOFF), s(S_QSOFF))
        self.cursor_next(S_QT, S_QN, S_QREAL)
        p.i("s_lshl_b32", s(S_QSOFF), s(S_QN), 15)

    def new_tile(self):
        """if W is block 0 of a tile (or the wave's first block, inside one): the state planes F, R start on the poly-A track, H0 / H1 / the carried pair and
        V_D0 / V_D1 are cleared, V_VMASK = the tile's valid reads"""
        p = self.p
        notile, newtile = self.lbl("notile"), self.lbl("newtile")
        p.i("s_cmp_eq_u32", s(S_WN), 0)
        p.i("s_cbranch_scc1", "@" + newtile)
        p.i("s_cmp_eq_u32", s(S_WF), s(S_S0))                    # (or the wave's first block, inside a tile)
        p.i("s_cbranch_scc0", "@" + notile)
        p.label(newtile)
        hf, hr = self.poly_a("F") if self.strand != 2 else None, self.poly_a("R") if self.strand != 1 else None
        for jj in range(31):
            if hf is not None:
                p.i("v_mov_b32", v(V_F + jj), -1 if (hf >> jj) & 1 else 0)
            if hr is not None:
                p.i("v_mov_b32", v(V_R + jj), -1 if (hr >> jj) & 1 else 0)
        for i in range(32):
            p.i("v_mov_b32", v(V_H0 + i), 0)
            p.i("v_mov_b32", v(V_H1 + i), 0)
        p.i("v_mov_b32", v(V_CARRY0), 0)
        p.i("v_mov_b32", v(V_CARRY1), 0)
        p.i("v_mov_b32", v(V_D0), 0)
        p.i("v_mov_b32", v(V_D1), 0)
        self.valid_reads(S_A)
        self.prefix_mask(V_VMASK, S_A, signed=False)
        p.label(notile)

    def block_setup(self):
        """per block W: V_CMASK / V_DMASK; S_STEPMASK = the steps that complete a window (bits 16 .. 31: of a ragged batch's last piece, emit_tail_step);
        F1 += the block's windows of every valid read"""
        p = self.p
        k, phi = self.k, self.phi
        self.block_masks()
        # steps of this block that complete a window: e = 16 (n - 1) + phi + a in [k - 1, L - 1]
        p.i("s_lshl_b32", s(S_A), s(S_WN), 4)
        p.i("s_add_i32", s(S_A), s(S_A), phi - 16)              # e0
        p.i("s_sub_i32", s(S_B), k - 1, s(S_A))
        p.i("s_max_i32", s(S_B), s(S_B), 0)                     # first valid step
        p.i("s_sub_i32", s(S_CC), s(S_L), s(S_A))
        p.i("s_sub_i32", s(S_CC), s(S_CC), 1)
        p.i("s_min_i32", s(S_CC), s(S_CC), 15)                  # last valid step
        p.i("s_sub_i32", s(S_CC), s(S_CC), s(S_B))
        p.i("s_add_i32", s(S_CC), s(S_CC), 1)                   # how many
        p.i("s_max_i32", s(S_CC), s(S_CC), 0)
        p.i("s_bfm_b32", s(S_STEPMASK), s(S_CC), s(S_B))
        p.i("s_cmp_ge_u32", s(S_WF), s(S_F0))                    # a block walked only to fill the window completes nothing
        p.i("s_cselect_b32", s(S_STEPMASK), s(S_STEPMASK), 0)
        p.i("s_cselect_b32", s(S_CC), s(S_CC), 0)
        # Ragged batch (round 5; ntRead takes any std::string, ntcard.cpp:173-189): the reads of a batch are 16 C - 15 .. 16 C bases long (read_len = 16 C) and
        # every tile's reads are sorted by length, longest first, so "the reads with a window ending at base 16 (C - 1) + d" are a PREFIX of the tile —
        # tails[tile][d] of them.  The steps that end in the last piece (e >= 16 (C - 1)) leave the step mask for the tail mask: their code (emit_tail_step,
        # out of line) narrows the candidate masks to that prefix and counts tails[tile][d] windows into F1 instead of one per read.
        noragged = self.lbl("noragged")
        self.unless_flag(F_RAGGED, noragged)
        p.i("s_sub_u32", s(S_B), s(S_C), 1)
        p.i("s_lshl_b32", s(S_B), s(S_B), 4)
        p.i("s_sub_i32", s(S_B), s(S_B), s(S_A))                 # first step that ends in the last piece (e0 + a >= 16 (C - 1))
        p.i("s_max_i32", s(S_B), s(S_B), 0)
        p.i("s_min_i32", s(S_B), s(S_B), 16)
        p.i("s_bfm_b32", s(S_B), s(S_B), 0)                      # the steps before it
        p.i("s_andn2_b32", s(S_A), s(S_STEPMASK), s(S_B))        # (e0 is spent)
        p.i("s_and_b32", s(S_STEPMASK), s(S_STEPMASK), s(S_B))
        p.i("s_bcnt1_i32_b32", s(S_CC), s(S_STEPMASK))
        p.i("s_lshl_b32", s(S_A), s(S_A), 16)
        p.i("s_or_b32", s(S_STEPMASK), s(S_STEPMASK), s(S_A))
        p.label(noragged)
        # F1 (ntcard.cpp:154): every window of every valid read counts here (K1f takes the invalid ones back)
        self.valid_reads(S_A)
        p.i("s_mul_i32", s(S_B), s(S_A), s(S_CC))
        self.f1_add(S_B)
        self.probe(3)

    def epilogue(self):
        """done: F1 (ntcard.cpp:154) and this wave's number of suspects leave by one lane (the timing build: its four section clocks); the log region's fill
        goes to log_fill; every store is waited for"""
        p = self.p
        p.label("done")
        T = V_MISC
        self.karg_load(S_TMP, "f1", wait=True)
        p.i("s_mov_b64", "exec", 1)
        p.i("v_mov_b32", v(T + 2), s(S_TMP))
        p.i("v_mov_b32", v(T + 3), s(S_TMP + 1))
        if self.on("timers"):
            p.i("v_mov_b32", v(T + 1), 0)
            for sec in range(4):
                p.i("v_mov_b32", v(T), s(S_TACC[sec]))
                p.i("global_atomic_add_x2", vr(T + 2, 2), vr(T, 2), "off", mods=f"offset:{8 * (1 + sec)}")
        else:
            p.i("v_mov_b32", v(T), s(S_F1ACC))
            p.i("v_mov_b32", v(T + 1), s(S_F1ACC + 1))
            p.i("global_atomic_add_x2", vr(T + 2, 2), vr(T, 2), "off")
            # suspects of this wave: their number (or all ones: the region overflowed, K1f falls back to walking every dirty block)
            self.karg_load(S_TMP, "sus_count")
            p.i("s_lshr_b32", s(S_A), s(S_SUSOFF), 4)
            p.i("s_cmp_le_u32", s(S_SUSOFF), s(S_SUSCAP))
            p.i("s_cselect_b32", s(S_A), s(S_A), -1)
            p.i("s_waitcnt", "lgkmcnt(0)")
            p.i("v_mov_b32", v(T), s(S_A))
            p.i("global_store_dword", v(V_WAVE4), v(T), sr(S_TMP, 2))
        p.i("s_mov_b64", "exec", -1)
        nofill = self.lbl("nofill")
        self.unless_flag(F_USELOG, nofill)
        self.store_log_fill()
        p.label(nofill)
        p.label("exit")
        p.i("s_waitcnt", "vmcnt(0) lgkmcnt(0)")
        p.i("s_branch", "@end")


def render_inc(k, sb, gap=0, strand=0):
    g = Gen(k, sb, gap, strand)
    prog = g.build()
    lines = prog.render(label_fmt=".Lk1h_{}_%=")
    body = "\n".join('\t"' + ln.replace('"', '\\"') + '\\n"' for ln in lines)
    what, name = (f"sBits class {sb}", f"K1H_ASM_K{k}_G{gap}_S{sb}") if strand == 0 else (f"sBits class {sb}, strand {strand}", f"K1H_ASM_K{k}_G{gap}_S{sb}_T{strand}")
    return f"// GENERATED by gen_k1h.py (k = {k}, gap = {gap}, {what}): {prog.n_insts()} instructions\n#define {name} \\\n" + \
        "\n".join(ln + " \\" for ln in body.split("\n")) + "\n\n"


# (k, gap) the library is built with: every plain k of 12 .. 32, and ntcard's -g seed in the two forms SURVEY 8(d) names for BASELINE config 5
# (k = 12 / gap 2: round 4; k = 32 / gap 8: round 5)
VARIANTS = tuple((k, 0) for k in range(12, 33)) + ((12, 2), (32, 8))
PARTS = 4                      # the kernels are spread over this many objects (k % PARTS) so that `make -j` compiles them side by side
# the one-strand kernels (NTC_FLAG_STRAND_TILED): every (k, gap) above for strand 1 (forward) and 2 (reverse), in include files and objects of their own
# (`gen_k1h.py --strand`: ntc_k1h_strand_gen.inc, compiled from the same ntc_sketch_k1h_body.hip with -DK1H_STRAND) beside the canonical parts
STRAND_VARIANTS = tuple((k, g, st) for st in (1, 2) for k, g in VARIANTS)
STRAND_PARTS = 8


def strand_part(k, strand):
    return (strand - 1) * (STRAND_PARTS // 2) + k % (STRAND_PARTS // 2)


def write_strand(out):
    defs = out.replace(".inc", "_defs.inc")
    with open(defs, "w") as f:
        f.write("// ntc_k1h_strand_gen_defs.inc — GENERATED by gen_k1h.py --strand (do not edit): the list of one-strand kernel variants\n")
        f.write(f"#define K1H_STRAND_GEN_PARTS {STRAND_PARTS}\n")
        f.write("#define K1H_STRAND_VARIANTS_ALL(X) " + " ".join(f"X({k}, {g}, {st})" for k, g, st in STRAND_VARIANTS) + "\n")
        for part in range(STRAND_PARTS):
            f.write(f"#define K1H_STRAND_VARIANTS_P{part}(X) " + " ".join(f"X({k}, {g}, {st})" for k, g, st in STRAND_VARIANTS if strand_part(k, st) == part) + "\n")
    with open(out, "w") as f:
        f.write("// ntc_k1h_strand_gen.inc — GENERATED by gen_k1h.py --strand (do not edit): one assembly string per (k, gap, sBits class, strand)\n")
        for k, gap, st in STRAND_VARIANTS:
            for sb in (7, 8):
                f.write(f"#if K1H_PART == {strand_part(k, st)}\n")
                f.write(render_inc(k, sb, gap, st))
                f.write("#endif\n")
    print("wrote", out, "and", defs)



if __name__ == "__main__":
    try:
        parse_exp()
    except ValueError as e:
        sys.exit(str(e))
    if len(sys.argv) > 1 and sys.argv[1] == "--strand":
        write_strand(sys.argv[2] if len(sys.argv) > 2 else "ntc_k1h_strand_gen.inc")
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else "ntc_k1h_gen.inc"
    defs = out.replace(".inc", "_defs.inc")
    with open(defs, "w") as f:
        f.write("// ntc_k1h_gen_defs.inc — GENERATED by gen_k1h.py (do not edit): geometry and the list of kernel variants\n")
        f.write(f"#define K1H_GEN_WAVES {WAVES}\n#define K1H_GEN_WAREA {WAREA} // LDS bytes per wave: ring + queue\n#define K1H_GEN_PARTS {PARTS}\n")
        f.write("#define K1H_VARIANTS_ALL(X) " + " ".join(f"X({k}, {g})" for k, g in VARIANTS) + "\n")
        for part in range(PARTS):
            f.write(f"#define K1H_VARIANTS_P{part}(X) " + " ".join(f"X({k}, {g})" for k, g in VARIANTS if k % PARTS == part) + "\n")
        # the byte offsets the generated code reads its arguments at (k1h_regs.KARG): ntc_sketch_k1h_body.hip checks each against struct K1hArgs
        f.write("#define K1H_GEN_KARGS(X) " + " ".join(f"X({name}, {off})" for name, off in KARG.items()) + "\n")
    with open(out, "w") as f:
        f.write("// ntc_k1h_gen.inc — GENERATED by gen_k1h.py (do not edit): one assembly string per (k, gap, sBits class)\n")
        for k, gap in VARIANTS:
            for sb in (7, 8):
                f.write(f"#if K1H_PART == {k % PARTS}\n")
                f.write(render_inc(k, sb, gap))
                f.write("#endif\n")
    print("wrote", out, "and", defs)
