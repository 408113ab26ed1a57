// ntc_sketch_hf.hip — K1 "H-filter": the production ntHash -> sample -> count kernel for gfx950.
//
// Profiling of the straightforward lane-per-read kernel (since retired; profiles/r01_v2_lane_per_read) showed
// it to be bound by the number of wave instructions issued, not by HBM, LDS or latency.  This
// variant therefore does the minimum per k-mer and moves everything that is only needed for the
// ~2^(1-sBits) sampled k-mers out of the per-base loop:
//
//   * the sampling decision of ntComp (ntcard.cpp:135-138) only looks at the top sBits+1 bits of
//     min(fh, rh); those bits live in the 31-bit rotating half H of the hash (nthash.hpp:186-217), and
//     H rolls independently of the 33-bit half.  The per-base loop therefore rolls ONLY the two H
//     halves (3 VALU ops each, one ds_read_b64 of seed terms) and tests min(fHd, rHd);
//   * a lane that sees a sampled window just shifts a 1 into a mask register (one v_addc): no branch, no
//     memory traffic;
//   * every 32 steps the wave queues the sampled (lane, step) pairs (one register per lane, filled through
//     ds_permute) and, 64 pairs at a time, recomputes the full 64-bit forward and reverse hashes of those windows
//     from the closed form
//     fh = XOR_i srol^(k-1-i)(seed(c_i)), rh = XOR_i srol^i(comp(c_i))      (nthash.hpp:220-239)
//     with a ceil(k/2) x 16 table of pre-rotated seed PAIRS in LDS (two bases per lookup), takes the canonical
//     min (nthash.hpp:275-279) and updates the sketch.  Full 64-bit compare: exact, no tie special case;
//   * equal-length waves start from the same closed form instead of rolling the k-1 window-filling steps; up to
//     four values of k share one launch (the batch is staged and decoded once); spaced seeds roll the spaced
//     value itself; nthll swaps the sample test for a register threshold.  LDS holds nothing but the decoded
//     slots and the tables, which is what lets 16 waves of 150 bp reads share a CU.
//
// The kernel, behind its stages, reads as their sequence: LDS layout and table load (lds_setup), the wave's share of the batches (wave_share),
// staging (stage_batch), per-lane geometry and wave class (read_geometry, k_begin), the walk (walk), the compaction queue (compact), the resolve round with its
// four sinks (resolve_round: HitLog::emit or the atomic, sink_hll, sink_dump, sig_append), the epilogue.  A stage takes the launch arguments, the per-wave
// state (Wave) and the per-k state (KState) as parameters; the compile-time choices travel as one tag type (Cfg).
//
// Semantics reproduced: ntRead (ntcard.cpp:147-158), ntHashIterator (ntHashIterator.hpp:59-86),
// NTMC64 (nthash.hpp:381-390,467-492), ntComp (ntcard.cpp:132-145).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstring>

#include "ntc_kernels.hpp"
#include "ntc_tile_bits.hpp"

namespace ntc {

#ifdef NTC_HF_CLOCKS // timing experiment (tools/ab_build.sh <name> -DNTC_HF_CLOCKS): first / last clock (100 MHz) of every wave of the LAST launch
__device__ unsigned long long g_hf_clocks[2 * 8192];
} // namespace ntc
extern "C" int ntc_dbg_hf_clocks(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ntc::g_hf_clocks), sizeof(unsigned long long) * 2 * 8192); }
namespace ntc {
#endif

namespace {

using tilebits::alignbit;
using tilebits::alignbyte;
using tilebits::ballot; // (of a bool, without the int round trip hipcc's ballot() goes through: saves 2 VALU ops per use)
using tilebits::mbcnt;
using tilebits::perm;
using tilebits::rfl;
using tilebits::rfl64;
using tilebits::v4u32;

// LDS by integer offset: lets a table address be formed with one v_and_or_b32 / SDWA v_or (index | aligned base)
typedef __attribute__((address_space(3))) const v4u32* lds_v4_ptr;
typedef __attribute__((address_space(3))) unsigned char* lds_byte_ptr;
__device__ __forceinline__ uint32_t lds_off(const void* p) { return (uint32_t)(uintptr_t)(lds_byte_ptr)p; }
__device__ __forceinline__ v4u32 lds_read4(uint32_t off) { return *(lds_v4_ptr)(uintptr_t)off; }
typedef uint32_t v2u32 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const v2u32* lds_v2_ptr;
typedef __attribute__((address_space(3))) const uint32_t* lds_u32_ptr;
__device__ __forceinline__ uint32_t lds_read1(uint32_t off) { return *(lds_u32_ptr)(uintptr_t)off; }
__device__ __forceinline__ v2u32 lds_read2(uint32_t off) { return *(lds_v2_ptr)(uintptr_t)off; } // one strand: the first half of an entry
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// Closed-form table addresses of 4 window bases w = [c0 c1 c2 c3] (code<<6 per byte): pair (c0,c1) -> a0, (c2,c3) -> a1.
// Entry offset of a pair is c_even<<6 | c_odd<<4; `tp` is the 256-byte aligned LDS offset of the table of this pair
// position (the next position's table follows 256 B later).  5 VALU instead of the 9 hipcc derives from the C form.
__device__ __forceinline__ void pair_addresses(uint32_t w, uint32_t tp, uint32_t& a0, uint32_t& a1)
{
	uint32_t m_even = 0x00c000c0u, m_odd = 0x00300030u, tp1 = tp + 256u;
	uint32_t hi, y;
	asm("v_lshrrev_b32_e32 %0, 10, %1" : "=v"(hi) : "v"(w));
	asm("v_and_b32_e32 %0, %1, %2" : "=v"(y) : "s"(m_even), "v"(w));
	asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(y) : "v"(hi), "s"(m_odd), "v"(y));
	asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(a0) : "v"(y), "s"(tp));
	asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(a1) : "v"(y), "s"(tp1));
}

// v_perm tables indexed by (byte & 7): 1:A 3:C 7:G 4:T 5:U, 0/2/6: not a base (nthash.hpp:16,32 trick)
constexpr uint32_t kExpS0 = 0x47ff5554u; // 'G', ff, 'U', 'T'
constexpr uint32_t kExpS1 = 0x43ff41ffu; // 'C', ff, 'A', ff
constexpr uint32_t kIn6S0 = 0x8000c0c0u; // code<<6 : G=2, -, U=3, T=3
constexpr uint32_t kIn6S1 = 0x40000000u; //           C=1, -, A=0, -

// x << 1 as a full-rate v_add_u32 (hipcc canonicalises x + x back into the half-rate v_lshlrev_b32)
__device__ __forceinline__ uint32_t dbl(uint32_t x)
{
	uint32_t r;
	asm("v_add_u32_e32 %0, %1, %1" : "=v"(r) : "v"(x));
	return r;
}

// decode one dword of raw bytes -> code<<6 per byte, bit 0 set on bytes that are not ACGTU/acgtu
__device__ __forceinline__ uint32_t decode4(uint32_t w, uint32_t& badacc)
{
	const uint32_t sel = w & 0x07070707u;
	const uint32_t bad = (perm(kExpS0, kExpS1, sel) ^ w) & 0xdfdfdfdfu;
	uint32_t code = perm(kIn6S0, kIn6S1, sel);
	if (bad != 0u) {
		badacc = 1u; // noted on the rare path only
		const uint32_t nz = (((bad & 0x7f7f7f7fu) + 0x7f7f7f7fu) | bad) & 0x80808080u;
		code = (code & ~(nz >> 1) & ~nz) | (nz >> 7); // dirty byte: code 0, mark bit 0
	}
	return code;
}

// a {forward, reverse} H-half entry of tabH / tabG / the seed blob; one strand: its first word only (ds_read_b32)
template <bool kOne>
__device__ __forceinline__ uint2 ld_h(const unsigned char* p)
{
	if constexpr (kOne)
		return make_uint2(*reinterpret_cast<const uint32_t*>(p), 0u);
	else
		return *reinterpret_cast<const uint2*>(p);
}

constexpr bool mode_spaced(int mode) { return (mode & 1) != 0; }
constexpr bool mode_hll(int mode) { return mode >= 2; }

// The compile-time choices of an instantiation, as the stages see them (kMulti, kPref and kTiled concern the kernel's glue and the staging only).
// mode: 0 plain k-mers, 1 spaced seed (any mask; ntcard's -g seed is the one-run case), 2 nthll, 3 nthll under a spaced seed — separate instantiations keep
// each one's register budget free of the other modes' state (the spaced-seed walks cost the plain kernel 5 spilled VGPRs otherwise).  The nthll modes drop the
// sample bounds, the flipped bit and the hit log; they add the threshold word and the register update of the resolve stage, and combine with `one`
// dump: validation build (ntc_hash_dump_k1_device): the filter lets EVERY window through, so the resolve stage
// re-derives the full canonical hash of every window with the production code path, and writes it out instead of
// sampling it (what ntHashIterator / stHashIterator enumerate, ntHashIterator.hpp:59-86, stHashIterator.hpp:60-87)
// one: ONE strand instead of the canonical value (HfK::strand 1 forward, 2 reverse): the walk rolls, looks up and tests one H half (no second
// rolling update, no min), the resolve stage XORs one strand's 64-bit terms (8 of an entry's 16 bytes) and skips the strand compare.  Both strands
// share the instantiation: the host puts the wanted strand's words in the first half of every table entry (nthash_tables.hpp: strand_t2,
// strand_seed_plan), and the only thing the kernel takes from HfK::strand is the shift of its rotate — x' = rot(x) ^ T with
// rot = v_alignbit(x, x << 1, 31) (rotl31, NTF64) or (x, x << 1, 2) (rotr31, NTR64 with its terms pre-rotated), both in the (H << 1) | H[30] layout
// sig: NTC_FLAG_SIGNATURE — the resolve stage also appends the 64-bit value of every sampled k-mer to the plane's value log (HfArgs::sig_log), in chunks
// a wave books with one cursor atomic each; instantiations of their own, so that the others carry neither the registers nor a branch for it
template <int kMode, bool kDump, bool kOne, bool kSig>
struct Cfg {
	static constexpr bool spaced = mode_spaced(kMode), hll = mode_hll(kMode), dump = kDump, one = kOne, sig = kSig;
};

// wave classes: CLEAN (equal lengths, no dirty byte), DIRTY (equal lengths, some non-ACGTU byte),
// RAGGED (lanes end at different steps, e.g. the last partial batch or a ragged host batch)
constexpr int CLEAN = 0, DIRTY = 1, RAGGED = 2;
// Table offsets (one byte per base: in<<6 | out<<4) of the 4 steps of a group at step q0.
//   FILL : every step has q < k     -> outgoing base is the virtual 'A' (code 0)
//   MIXED: the group straddles k    -> mask the steps with q < k
//   MAIN : every step has q >= k
constexpr int FILL = 0, MIXED = 1, MAIN = 2;
constexpr int32_t kShut = 0x7fffffff; // KState::nextok of a lane that emits nothing (any more)

// ---- state ----------------------------------------------------------------------------------------------------------------------------------------
// Where things are in LDS.  Nothing but the tables and the decoded slots lives there: hit masks and the compaction queue stay in registers, so that a
// CU's 160 KiB hold 16 waves of 150 bp reads (4 per SIMD) instead of 12.
// dynamic LDS: [closed-form tables of every fused k][gap table][16 B pad][waves x 64 slots].  The tables come first:
// with 1280 B of static LDS in front they start 256-byte aligned, so `index | base` addresses them.  The gap table of a
// spaced seed is SeedPlan::blob: XOR-out pair tables, the toggle tables beyond pair 0, the XOR-out position words.
struct Lds {
	unsigned char* t1_base;          // closed-form pair tables
	const unsigned char *tabH, *tabG; // static LDS: per-(in,out) seed terms of the H halves {Tf.Hd, Tr.Hd}, 16-byte stride (offset = idx byte); tabG: spaced seed, rolling form
	// spaced seed (stRead, ntcard.cpp:160-171): per pair of don't-care positions, the H halves of the terms to XOR out
	unsigned char* gapT;
	const unsigned char* rollT; // toggle tables of pairs 1 .. nroll-1 (pair 0: tabG)
	const uint32_t* dcw;        // [ngp] d | d' << 16
	uint32_t ngp, nroll, seed_extra, stride;
	unsigned char* wdata;      // the wave's 64 decoded slots
	const unsigned char* mine; // this lane's
};

// Sample 0 of ntComp wants the top sBits+1 bits of min(fh,rh) to be 0..01.  Both strands are carried with
// that one bit flipped (folded into the step table: x' = x ^ c rolls with the term t ^ c ^ rotl(c)), so the
// test becomes min(f',r') < c: a superset (extra: one strand 0..01 while the other is 0..00, p = 2^-2(sBits+1)),
// made exact by the resolve stage, which re-derives everything from the bases.  Sample 1 looks at the bits
// above c only and is unaffected.  nthll compares against a moving threshold and runs unflipped: the threshold is a power of two >= 2
// (hll_threshold_kernel), so `value < thr` reads bits 31 .. 1 of the walk's word — H itself, the hash's bits 63 .. 33 — and never bit 0, the copy of H[30].
// One strand: both rotates keep the (H << 1) | H[30] layout (rotl31 and rotr31 of H with the copy refreshed, see Cfg::one), so the same compare holds for
// the forward and the reverse walk; canonical: min(f, r) < thr is "either strand below", a superset of "the smaller 64-bit value below".
struct Sample {
	uint32_t flipc, flipx, rot_sh; // the flipped bit, what it adds to a step term, the one-strand rotate
	uint32_t lo0, hll_thr, s_bits, rmask, rbuck; // lo0, lo1: sample windows on the top bits (ntcard.cpp:135-138); VGPR-resident on purpose (SGPR sources
	int32_t lo1;                                 // halve the VALU rate)
	template <class C>
	__device__ __forceinline__ void init(const HfArgs& a)
	{
		flipc = C::hll ? 0u : 1u << (31 - a.s_bits);
		// (one strand: x' = rot(x) ^ T for both, so the flipped bit rolls with T ^ c ^ rot(c); sBits 2 .. 24 keeps c and rot(c) inside bits 30 .. 6)
		flipx = flipc ^ (C::one && a.ks[0].strand == 2u ? flipc >> 1 : flipc << 1);
		rot_sh = C::one && a.ks[0].strand == 2u ? 2u : 31u;
		if constexpr (C::one) asm volatile("" : "+v"(rot_sh)); // VGPR-resident like the sample bounds below
		lo0 = 1u << (31 - a.s_bits);
		lo1 = (int32_t)(((1u << (a.s_bits - 1)) - 1u) << (32 - a.s_bits));
		asm volatile("" : "+v"(lo0), "+v"(lo1));
		s_bits = a.s_bits;
		hll_thr = a.hll_bits ? *a.hll_thr : 0u;
		asm volatile("" : "+v"(hll_thr));
		rmask = (1u << a.r_bits) - 1u, rbuck = 1u << a.r_bits;
	}
};

// Hit log: ntComp's `++t_Counter[...]` (ntcard.cpp:142-143) is not executed here.  The wave appends the counter
// index of every sampled k-mer to its private log regions gwave, gwave + W, ... (W = waves of this launch) with one
// coalesced store per resolve round; ntc_apply.hip adds them to the sketch later (counting commutes).  A wave
// that runs out of regions falls back to the direct atomic, which is exact as well.  All of it is wave-uniform.
struct HitLog {
	bool use;
	uint32_t step, reg, fill; // the wave's regions are reg, reg + step, ...; fill: entries in the current one
	template <class C>
	__device__ __forceinline__ void open(const HfArgs& a, int lane, uint32_t gwave, uint32_t nwaves)
	{
		use = !C::hll && a.log_regions != 0 && (a.log_mode == nullptr || rfl(*a.log_mode) == 0u);
		step = nwaves, reg = gwave, fill = 0;
		if (use && reg < a.log_regions) fill = rfl(a.log_fill[reg]);
		if (!C::hll && !use && a.sk_dirty != nullptr && lane == 0) *a.sk_dirty = 1u; // direct atomics from here on (the device mode word, or no regions)
	}
	__device__ __forceinline__ void emit(const HfArgs& a, int lane, bool hit, uint32_t key)
	{
		const uint64_t m = ballot(hit);
		if (m == 0) return;
		const uint32_t c = (uint32_t)__popcll(m);
		while (reg < a.log_regions && c > a.log_region_cap - fill) { // region full: book its fill, take this wave's next one
			if (lane == 0) a.log_fill[reg] = fill;
			reg += step;
			fill = reg < a.log_regions ? rfl(a.log_fill[reg]) : 0u;
		}
		if (reg < a.log_regions) {
			if (hit) a.log[(uint64_t)reg * a.log_region_cap + fill + mbcnt(m)] = key;
			fill += c;
		} else if (hit) {
			atomicAdd(a.sketch0 + key, 1u);
			if (a.sk_dirty) *a.sk_dirty = 1u; // (out of log regions: the sketch is no longer what the last reset / apply left, ntc_apply.hip count_kernel)
		}
	}
	__device__ __forceinline__ void close(const HfArgs& a, int lane) { if (use && lane == 0 && reg < a.log_regions) a.log_fill[reg] = fill; }
};

// What lasts for the whole launch of one wave.
struct Wave {
	int lane;
	bool can_prefetch; // the batch's staging runs through the register prefetch (wave priorities follow it, see the kernel)
	Lds L; Sample S; HitLog log;
	uint64_t slot0; // the staged batch: first slot, slots in it, some byte of it is no base; this lane's read: length, window limit, inside the batch
	uint32_t nvalid, len, wlim;
	bool dirty, in_batch;
};

// One k of the list over one staged batch: the plane, the walk's registers, the compaction queue.
struct KState {
	uint32_t ki, k, tp;         // tp: LDS offset of this k's closed-form tables (256-byte aligned, wave-uniform)
	const unsigned char* tabHb; // this k's step terms
	uint32_t* sketch;
	uint32_t key_base, shb; // shb: byte phase of the outgoing-base stream
	unsigned long long *sig_log, *sig_cur; // Cfg::sig: the plane's value log and cursor, the wave's place in its current chunk of the log, the entries left
	uint64_t sig_at;                       // of the chunk (wave-uniform), the values logged for this batch
	uint32_t sig_room, sig_vals;
	int32_t endq, maxq, nextok; // steps q in [0, endq) of this lane; the wave's longest; emission allowed from step nextok on
	uint32_t fHd, rHd;          // H halves in the walk layout (H << 1) | H[30], sample bit flipped
	uint32_t hmask, f1_lane;    // sampled steps of the current 32-step block, its last step at bit 0; DIRTY / RAGGED: clean windows of this lane (rare path)
	uint64_t f1_wave;
	uint32_t pend, npend; // the queue: entry i lives in lane i
};

// ---- stage: LDS layout and table load ---------------------------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void lds_setup(const HfArgs& a, uint32_t n_k, unsigned char* smem, uint32_t (*tabH)[kMainSlots * 4], uint32_t* tabG, int wave, Wave& W, uint32_t (&t1_off)[kMaxFusedK + 1])
{
	Lds& L = W.L;
	L.stride = a.stride, t1_off[0] = 0;
	for (uint32_t j = 0; j < (uint32_t)kMaxFusedK; ++j)
		t1_off[j + 1] = t1_off[j] + (j < n_k ? ((a.ks[j].k + 1u) >> 1) * 256u : 0u);
	L.seed_extra = C::spaced ? a.seed_extra : 0u, L.nroll = C::spaced ? a.seed_nroll : 0u, L.ngp = (a.gap + 1u) >> 1;
	const uint32_t tables_bytes = t1_off[kMaxFusedK] + L.ngp * 256u + L.seed_extra;
	// waves per block: chosen by the host so that one CU holds as many waves as its 160 KiB of LDS allow
	// (every wave parks its 64 slots in LDS; the closed-form table is shared by the block)
	L.wdata = smem + tables_bytes + 16 + (size_t)wave * 64u * L.stride;
	L.mine = L.wdata + (size_t)W.lane * L.stride;
	L.t1_base = smem;
	if ((lds_off(smem) & 255u) != 0u) __builtin_trap(); // the static tables are sized to keep this aligned
	L.gapT = L.t1_base + t1_off[kMaxFusedK], L.rollT = L.gapT + L.ngp * 256u;
	L.dcw = reinterpret_cast<const uint32_t*>(L.rollT + (L.nroll > 1u ? L.nroll - 1u : 0u) * 256u);
	L.tabH = reinterpret_cast<const unsigned char*>(tabH), L.tabG = reinterpret_cast<const unsigned char*>(tabG);
	// the load (the block synchronises behind it): step terms with the sample bit's flip folded in, pair tables, the seed blob
	const int tid = threadIdx.x;
	const uint32_t flipx = W.S.flipx;
	for (uint32_t j = 0; j < n_k; ++j) {
		for (int i = tid; i < kMainSlots * 4; i += (int)blockDim.x) {
			const int slot = i >> 2, w = i & 3;
			tabH[j][i] = w < 2 ? (a.ks[j].tabh[slot][w] ^ flipx) : 0u;
		}
		const uint4* src = reinterpret_cast<const uint4*>(a.ks[j].t1);
		uint4* dst = reinterpret_cast<uint4*>(L.t1_base + t1_off[j]);
		for (uint32_t i = tid; i < (t1_off[j + 1] - t1_off[j]) / 16u; i += blockDim.x)
			dst[i] = src[i];
	}
	if (a.gap != 0)
		for (int i = tid; i < kMainSlots * 4; i += (int)blockDim.x)
			tabG[i] = (i & 3) < 2 ? a.tabg[i >> 2][i & 3] : 0u;
	const uint4* gsrc = reinterpret_cast<const uint4*>(a.gapt);
	for (uint32_t i = tid; i < L.ngp * 16u + L.seed_extra / 16u; i += blockDim.x)
		reinterpret_cast<uint4*>(L.gapT)[i] = gsrc[i];
}

// ---- stage: the wave's share of the batches ---------------------------------------------------------------------------------------------------------
// A contiguous share of its workgroup's contiguous share of the launch's wave-batches, weighed by the wave's AGE on its SIMD.
// Before, wave g took the batches g, g + W, g + 2 W, ... — the same number for every wave — and the SIMDs, which issue their older waves first, finished the
// waves of a workgroup in the order of their age: 2090 / 2161 / 2255 us into a 2.33 ms launch with three waves per SIMD (config 4), 806 / 820 / 865 / 877 into
// 0.92 ms with four (per-wave clocks of a -DNTC_HF_CLOCKS build, profiles/r06_k1_wave_clocks.txt); the youngest ran on alone at the end.  Waves 4 r .. 4 r + 3 of
// a workgroup are the r-th on their SIMDs; the weights are the speeds those clocks showed, in 1 / 1024 of a SIMD's batches.
__device__ __forceinline__ uint32_t age_share_before(uint32_t w, uint32_t wpb) // the shares of the waves in front of wave w, in 1 / 1024 of a SIMD's batches
{
	static constexpr uint16_t kAgeShare[5][4] = { { 0, 0, 0, 0 }, { 1024, 0, 0, 0 }, { 530, 494, 0, 0 }, { 354, 342, 328, 0 }, { 267, 263, 249, 245 } };
	const uint32_t ranks = (wpb + 3u) / 4u; // (1 .. 4)
	uint32_t c = 0;
	for (uint32_t r = 0; r < ranks; ++r) {
		const uint32_t in_rank = w > 4u * r ? (w - 4u * r < 4u ? w - 4u * r : 4u) : 0u; // waves of rank r in front of w
		c += in_rank * (wpb % 4u == 0u ? kAgeShare[ranks][r] : 1024u / ranks);
	}
	return c;
}
__device__ __forceinline__ void wave_share(uint64_t n_wb, uint32_t wpb, uint32_t wave, uint64_t& wb_begin, uint64_t& wb_end)
{
	const uint64_t per_wg = (n_wb + gridDim.x - 1) / gridDim.x;
	const uint64_t g0 = (uint64_t)blockIdx.x * per_wg < n_wb ? (uint64_t)blockIdx.x * per_wg : n_wb;
	const uint64_t g1 = g0 + per_wg < n_wb ? g0 + per_wg : n_wb;
	const uint32_t total = age_share_before(wpb, wpb);
	wb_begin = rfl64(g0 + (g1 - g0) * age_share_before(wave, wpb) / total);
	wb_end = rfl64(wave + 1u == wpb ? g1 : g0 + (g1 - g0) * age_share_before(wave + 1u, wpb) / total);
}

// ---- stage: staging of a batch, global -> LDS, with register prefetch of the next batch ------------------------------------------------------------
// kPref: 1 KiB chunks of the NEXT batch a wave keeps in flight in registers (10 covers slots of up to 160 B at 16 waves
// per CU; 16 covers 256 B slots, whose LDS footprint allows 12 waves at most, hence the smaller launch bound)
// A TILED batch (a.tiled: the k of a list that K1h is not built for are hashed here from the same tiles, without a re-layout pass): the wave's
// 64 reads are 64 consecutive 16-byte pieces of every chunk row of their tile, so round c of the staging is ONE coalesced 1 KiB load — piece c of read
// `lane` — parked at lane * stride + 16 c: the same LDS picture as a row-slot batch of stride 16 n_chunks.  The slots behind a batch's last read exist
// (a tile buffer always holds whole tiles), so a partial last wave loads like a full one and masks its lanes afterwards.
// (kTiled is an instantiation of its own: as a run-time flag the two addressing forms cost every variant 150 - 330 B of scratch per lane)
// batch wb -> the wave's decoded slots (W.slot0, W.nvalid, W.dirty); the loads of batch wb_next (n_wb: none) go out behind it.  load(wb, c0) fetches the
// chunks c0 .. of a batch into the prefetch registers, store(c0, badacc) decodes and parks them (the kernel's two lambdas)
template <int kPref, bool kTiled, class Load, class Store>
__device__ __forceinline__ void stage_batch(const HfArgs& a, Wave& W, uint64_t wb, uint64_t wb_next, uint64_t n_wb, Load&& load, Store&& store)
{
	const uint32_t lane = (uint32_t)W.lane;
	W.slot0 = wb * 64;
	W.nvalid = (uint32_t)((a.n_slots - W.slot0) < 64 ? (a.n_slots - W.slot0) : 64);
	uint32_t badacc = 0;
	__builtin_amdgcn_wave_barrier();
	if ((W.nvalid == 64 || kTiled) && W.can_prefetch) {
		store(0, badacc);
		if (wb_next < n_wb && (kTiled || wb_next * 64 + 64 <= a.n_slots)) load(wb_next, 0);
	} else if (W.nvalid == 64 || kTiled) {
		for (uint32_t c0 = 0; c0 < (64u * W.L.stride + 1023u) >> 10; c0 += kPref) {
			load(wb, c0);
			store(c0, badacc);
		}
	} else { // the ragged tail: a partial last batch of row slots
		const unsigned char* src = a.slots + W.slot0 * W.L.stride;
		const uint32_t bytes = W.nvalid * W.L.stride;
		for (uint32_t off = lane * 16u; off < bytes; off += 1024u)
			for (uint32_t o = off; o < bytes && o < off + 16u; o += 4)
				*reinterpret_cast<uint32_t*>(W.L.wdata + o) = decode4(*reinterpret_cast<const uint32_t*>(src + o), badacc);
	}
	__builtin_amdgcn_wave_barrier();
	if (kTiled && lane >= W.nvalid) badacc = 0; // (a lane stages its own read there: what lies behind the batch's last read is nobody's)
	W.dirty = rfl(ballot(badacc != 0u) != 0 ? 1 : 0) != 0;
}

// ---- stage: per-lane geometry and wave class --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void read_geometry(const HfArgs& a, Wave& W)
{
	W.len = a.read_len, W.wlim = a.read_len;
	W.in_batch = (uint32_t)W.lane < W.nvalid;
	if (a.meta != nullptr && W.in_batch) {
		const uint32_t m = a.meta[W.slot0 + W.lane];
		W.len = m & 0xffffu, W.wlim = m >> 16;
	}
}

// k number ki of the list over the staged batch: the plane's words, the lane's steps, the walk's start; returns the wave class
template <class C>
__device__ __forceinline__ int k_begin(const HfArgs& a, const Wave& W, uint32_t ki, uint32_t t1_off, uint64_t sig_at, uint32_t sig_room, KState& K)
{
	K.ki = ki, K.k = a.ks[ki].k;
	K.tp = rfl(lds_off(W.L.t1_base + t1_off));
	K.tabHb = W.L.tabH + ki * (kMainSlots * 16u);
	K.sketch = a.ks[ki].sketch, K.key_base = a.ks[ki].key_base;
	if constexpr (C::sig) K.sig_log = a.sig_log[ki], K.sig_cur = a.sig_cursor[ki], K.sig_at = sig_at, K.sig_room = sig_room, K.sig_vals = 0;
	K.shb = (0u - K.k) & 3u, K.f1_wave = 0;
	K.endq = (int32_t)(W.len < W.wlim + K.k - 1 ? W.len : W.wlim + K.k - 1);
	if (!W.in_batch || W.len < K.k) K.endq = 0;
	int32_t maxq = K.endq, minq = K.endq;
	for (int o = 32; o > 0; o >>= 1) {
		const int32_t omax = __shfl_xor(maxq, o), omin = __shfl_xor(minq, o);
		maxq = omax > maxq ? omax : maxq;
		minq = omin < minq ? omin : minq;
	}
	K.maxq = __builtin_amdgcn_readfirstlane(maxq), minq = __builtin_amdgcn_readfirstlane(minq);
	// The walk starts from the H halves of the hash of k virtual 'A's and feeds 'A' as the outgoing
	// base of the first k steps, so ONE step body serves window filling and steady state.
	K.fHd = a.ks[ki].init_f ^ W.S.flipc, K.rHd = a.ks[ki].init_r ^ W.S.flipc;
	K.nextok = K.endq > 0 ? (int32_t)K.k - 1 : kShut;
	K.hmask = 0, K.f1_lane = 0, K.pend = 0, K.npend = 0;
	// (a mask with more toggle pairs than the rolling form takes walks every wave as RAGGED: the closed-form XOR-out)
	return minq != K.maxq || (C::spaced && W.L.nroll == 0u) ? RAGGED : (W.dirty ? DIRTY : CLEAN);
}

// ---- the closed form over the pair tables, written once ---------------------------------------------------------------------------------------------
// XOR of pair-table entries: both strands or one, both 64-bit words or (kHigh) the high words only — the walk's start wants nothing but the H halves
template <bool kOne, bool kHigh>
struct PairAcc {
	uint32_t flo = 0, fhi = 0, rlo = 0, rhi = 0;
	// the words of an entry that count: one strand, the wanted strand's 64-bit term is its first half, of which word 1 is the high half
	static __device__ __forceinline__ v4u32 entry(uint32_t a)
	{
		if constexpr (kOne && kHigh)
			return v4u32{0u, lds_read1(a + 4u), 0u, 0u};
		else if constexpr (kOne)
			return v4u32{lds_read2(a).x, lds_read2(a).y, 0u, 0u};
		else
			return lds_read4(a);
	}
	__device__ __forceinline__ void add2(uint32_t a0, uint32_t a1) // the two pairs of a 4-base step
	{
		const v4u32 t0 = entry(a0), t1 = entry(a1);
		if constexpr (!kHigh) flo = xor3(flo, t0.x, t1.x);
		fhi = xor3(fhi, t0.y, t1.y);
		if constexpr (!kHigh && !kOne) rlo = xor3(rlo, t0.z, t1.z);
		if constexpr (!kOne) rhi = xor3(rhi, t0.w, t1.w);
	}
	__device__ __forceinline__ void add(uint32_t a0) // one pair of the 1..3-base tail
	{
		const v4u32 t0 = entry(a0);
		flo ^= t0.x, fhi ^= t0.y, rlo ^= t0.z, rhi ^= t0.w;
	}
};

// The k code bytes at dp (kAligned) or `sh` bytes behind it (one funnel shift per word), 4 bases = 2 pair lookups per iteration, no branch inside; then
// the 1..3 bases left: a base beyond k contributes nothing because the odd-k table drops the b term.  note(i, w): the 4 code bytes of window positions
// i .. i + 3 as they pass (bytes beyond k cleared).
template <bool kOne, bool kHigh, bool kAligned, class Note>
__device__ __forceinline__ PairAcc<kOne, kHigh> closed_form(const uint32_t* dp, uint32_t sh, uint32_t k, uint32_t tp, Note&& note)
{
	PairAcc<kOne, kHigh> h;
	uint32_t cur = kAligned ? 0u : dp[0];
	uint32_t i = 0;
	for (; i < (k & ~3u); i += 4) {
		uint32_t w;
		if constexpr (kAligned) {
			w = dp[i >> 2];
		} else {
			const uint32_t nxt = dp[(i >> 2) + 1];
			w = alignbyte(nxt, cur, sh);
			cur = nxt;
		}
		note(i, w);
		uint32_t a0, a1;
		pair_addresses(w, tp, a0, a1);
		h.add2(a0, a1);
		tp += 512u;
	}
	if (k & 3u) {
		const uint32_t w = kAligned ? dp[i >> 2] : alignbyte(dp[(i >> 2) + 1], cur, sh);
		note(i, w & (0xffffffffu >> (8 * (4 - (k & 3u)))));
		uint32_t a0, a1;
		pair_addresses(w, tp, a0, a1);
		h.add(a0);
		if ((k & 3u) == 3u) h.add(a1);
	}
	return h;
}

// ---- stage: the resolve round and its sinks ---------------------------------------------------------------------------------------------------------
// validation build: the value of window `win` of read `row`
__device__ __forceinline__ void sink_dump(const HfArgs& a, uint64_t row, uint32_t win, uint32_t hi, uint32_t lo)
{
	if (win < a.dump_win) {
		a.dump[row * a.dump_win + win] = ((uint64_t)hi << 32) | lo;
		atomicOr(a.dump_valid + row * ((a.dump_win + 31u) >> 5) + (win >> 5), 1u << (win & 31u));
	}
}
// nthll's ntComp (nthll.cpp:92-97): bucket = low bits, value = leading zeros of the rest
__device__ __forceinline__ void sink_hll(const HfArgs& a, uint32_t* regs, uint32_t hi, uint32_t lo)
{
	const uint32_t bmask = (1u << a.hll_bits) - 1u, lo_rest = lo & ~bmask;
	if ((hi | lo_rest) != 0u) {
		const uint32_t run0 = hi ? (uint32_t)__builtin_clz(hi) : 32u + (uint32_t)__builtin_clz(lo_rest);
		atomicMax(regs + (lo & bmask), run0);
	}
}
// The sampled values of a round, behind one another in the wave's current CHUNK of the plane's value log.  A chunk is booked with one
// cursor atomic (one per resolve round on the one address cost K1 about 3 ms per 18 M values, profiles/signature.txt).  A round that does
// not fit the rest of the chunk fills it and goes on in the next one, so a wave leaves nothing unused but the rest of its LAST chunk,
// which it zeroes on its way out — no sampled value is 0, the insert pass skips zeros
__device__ __forceinline__ void sig_append(const HfArgs& a, Wave& W, KState& K, bool hit, unsigned long long v)
{
	const uint64_t m = ballot(hit);
	if (m == 0) return;
	const uint32_t c = (uint32_t)__popcll(m), pos = mbcnt(m);
	uint32_t skip = 0; // values of this round that went into the chunk just filled
	if (c > K.sig_room) {
		skip = K.sig_room;
		if (hit && pos < skip && K.sig_at + pos < a.sig_cap) K.sig_log[K.sig_at + pos] = v;
		unsigned long long b = 0;
		if (W.lane == 0) b = atomicAdd(K.sig_cur, (unsigned long long)a.sig_chunk);
		K.sig_at = rfl64(b);
		K.sig_room = a.sig_chunk; // (>= 64: what is left of a round always fits a fresh chunk)
	}
	const uint64_t at = K.sig_at + (pos - skip);
	if (hit && pos >= skip && at < a.sig_cap) K.sig_log[at] = v;
	K.sig_at += c - skip, K.sig_room -= c - skip, K.sig_vals += c;
}

// 64 (lane, step) pairs at a time (entry e of this lane, `count` of them in the wave): recompute the full hashes from the bases, then the sinks
template <class C>
__device__ __forceinline__ void resolve_round(const HfArgs& a, Wave& W, KState& K, uint32_t e, uint32_t count)
{
	// entry -> window start in LDS (any lane's slot), then the closed form over k bases
	const bool act = (uint32_t)W.lane < count;
	const uint32_t src_lane = e >> 16, q = e & 0xffffu;
	const uint32_t base = act ? src_lane * W.L.stride + q + 1u - K.k : 0u; // byte offset of the window in wdata
	uint32_t dirty = 0; // bit 0 of a byte: not ACGTU
	const auto h = closed_form<C::one, false, false>(reinterpret_cast<const uint32_t*>(W.L.wdata + (base & ~3u)), base & 3u, K.k, K.tp,
	                                                 [&](uint32_t, uint32_t w) { dirty |= w; });
	bool hit = false;
	uint32_t key = 0, rel = 0; // rel: counter index inside this k's plane pair; key: index in the engine's whole sketch (hit-log keys)
	uint32_t sig_hi = 0, sig_lo = 0; // Cfg::sig: the value itself
	if (act && (dirty & 0x01010101u) == 0u) { // a window with a non-ACGTU byte yields no k-mer (ntHashIterator.hpp:59-86)
		const bool rev = !C::one && ((h.rhi < h.fhi) | ((h.rhi == h.fhi) & (h.rlo < h.flo))); // nthash.hpp:275-279 (one strand: no choice to make)
		const uint32_t hi = rev ? h.rhi : h.fhi, lo = rev ? h.rlo : h.flo;
		if constexpr (C::dump) {
			sink_dump(a, W.slot0 + src_lane, q + 1u - K.k, hi, lo);
		} else if constexpr (C::hll) {
			sink_hll(a, K.sketch, hi, lo);
		} else {
			// ntComp (ntcard.cpp:132-145) on the canonical value; sample 1 wins when both match
			const bool c1 = (hi >> (32 - W.S.s_bits)) == ((1u << (W.S.s_bits - 1)) - 1u);
			const bool c0 = (hi >> (31 - W.S.s_bits)) == 1u;
			hit = c0 | c1;
			rel = (lo & W.S.rmask) + (c1 ? W.S.rbuck : 0u);
			key = K.key_base + rel;
			if constexpr (C::sig) sig_hi = hi, sig_lo = lo;
		}
	}
	if constexpr (C::sig) sig_append(a, W, K, hit, ((unsigned long long)sig_hi << 32) | sig_lo);
	if constexpr (!C::hll && !C::dump) {
		if (W.log.use)
			W.log.emit(a, W.lane, hit, key); // the increment itself happens later (ntc_apply.hip)
		else if (hit)
			atomicAdd(K.sketch + rel, 1u); // not sketch0 + key: without a log the sketch may hold more than 2^32 counters (32-bit keys would alias)
	}
}

// ---- stage: the compaction queue --------------------------------------------------------------------------------------------------------------------
// End of a 32-step block: queue the block's sampled steps as (lane, step) pairs.  The queue is ONE register
// per lane (entry i of the queue lives in lane i); each pass moves one pair per lane with a forward
// permute through the LDS crossbar (no LDS memory): a lane with a hit sends it to slot npend + rank, the
// others send a dummy to the remaining slots so that the destinations form a permutation.  When 64 are
// queued they are resolved; pairs beyond 64 are already sitting in the low lanes of the permute result.
template <class C>
__device__ __forceinline__ void compact(const HfArgs& a, Wave& W, KState& K, int32_t last) // `last` = the step recorded at bit 0 of hmask
{
	if (W.can_prefetch) __builtin_amdgcn_s_setprio(3);
	uint32_t cur = K.hmask;
	uint32_t np = rfl(K.npend); // wave-uniform: the queue fill lives on the scalar unit
	for (;;) {
		const uint64_t m = ballot(cur != 0u);
		if (m == 0) break;
		const uint32_t c = (uint32_t)__popcll(m);
		const bool hit = cur != 0u;
		uint32_t bit;
		asm("v_ffbl_b32 %0, %1" : "=v"(bit) : "v"(cur)); // lowest set bit (all ones for 0: the pair is a dummy then)
		cur &= cur - 1u;
		const uint32_t pos = mbcnt(m);
		const uint32_t entry = ((uint32_t)W.lane << 16) | (((uint32_t)last - bit) & 0xffffu);
		const uint32_t dest = (hit ? pos : c + (uint32_t)W.lane - pos) + np; // a permutation of 0..63 (mod 64)
		const uint32_t recv = (uint32_t)__builtin_amdgcn_ds_permute((int)(dest << 2), (int)entry);
		K.pend = (uint32_t)W.lane >= np ? recv : K.pend;
		np += c;
		if (np >= 64u) {
			resolve_round<C>(a, W, K, K.pend, 64u);
			K.pend = recv, np -= 64u;
		}
	}
	K.hmask = 0, K.npend = np;
	if (W.can_prefetch) __builtin_amdgcn_s_setprio(2);
}

// ---- stage: the walk --------------------------------------------------------------------------------------------------------------------------------
// one rolling step of the H halves with the step terms t; spaced seed, rolling form (kGap): two more terms per strand, g
template <bool kOne, bool kGap>
__device__ __forceinline__ void roll(KState& K, const Sample& S, const uint2 t, const uint2 g)
{
	if constexpr (kOne) { // the one strand lives in fHd, whichever it is: rotl31 / rotr31 by rot_sh, then ^ T (the host rotated the reverse terms)
		const uint32_t r = alignbit(K.fHd, dbl(K.fHd), S.rot_sh);
		K.fHd = kGap ? xor3(r, t.x, g.x) : r ^ t.x;
	} else {
		const uint32_t r = alignbit(K.fHd, dbl(K.fHd), 31); // rotl31 in the (H<<1)|H[30] layout, then ^ Tf
		K.fHd = kGap ? r ^ t.x ^ g.x : r ^ t.x;
		const uint32_t xh = kGap ? K.rHd ^ t.y ^ g.y : K.rHd ^ t.y; // reverse strand: ^ Tr, then rotr31
		K.rHd = alignbit(xh >> 1, xh, 1);
	}
}
// a dirty byte at step q closes the current run of clean windows [nextok, q) and reopens at q+k
__device__ __forceinline__ void on_mark(KState& K, int32_t q)
{
	if (K.nextok != kShut) {
		if (q > K.nextok) K.f1_lane += (uint32_t)(q - K.nextok);
		K.nextok = q + (int32_t)K.k;
	}
}
__device__ __forceinline__ void on_end(KState& K, int32_t q) // RAGGED: the lane's last step was q-1
{
	if (q >= K.endq && K.nextok != kShut) {
		if (K.endq > K.nextok) K.f1_lane += (uint32_t)(K.endq - K.nextok);
		K.nextok = kShut;
	}
}
__device__ __forceinline__ void on_marks(KState& K, int32_t q0, uint32_t mk) // the marks (bit 0 of a byte) of the 4 code bytes of steps q0 .. q0 + 3
{
	while (mk != 0u) {
		on_mark(K, q0 + (int32_t)((uint32_t)__builtin_ctz(mk) >> 3));
		mk &= mk - 1u;
	}
}

// Sampled steps are recorded without a branch: every step from the first non-FILL group on shifts
// the lane's mask left and shifts the wave's "sampled" condition in as carry (one v_addc_co_u32);
// after 32 steps the mask is compacted into the resolve queue.  The block's last step sits at bit 0.
template <bool kDump>
__device__ __forceinline__ void push(uint32_t& hmask, uint64_t m)
{
	if constexpr (kDump) {
		// the validation build's m is ballot(true), i.e. EXEC itself: with a tied in/out operand the compiler wrote the carry-out over EXEC
		// (v_addc_co_u32_e64 v, exec, v, v, exec), which switched off every lane whose mask had no carry — in a DIRTY wave, after the
		// first recorded step.  Carry in from m, carry out to a register of its own.
		uint64_t co;
		asm volatile("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(hmask), "=&s"(co) : "s"(m));
	} else {
		asm volatile("v_addc_co_u32_e64 %0, %1, %0, %0, %1" : "+v"(hmask), "+s"(m));
	}
}
template <class C, int wc>
__device__ __forceinline__ void record(const Wave& W, KState& K, int32_t q, bool emitting)
{
	uint64_t m = 0;
	if (emitting) {
		uint32_t fs = K.fHd, rs = K.rHd;
		if constexpr (C::spaced && wc == RAGGED) {
			// NTMSM64 (nthash.hpp:641-646,665-670): XOR the don't-care bases' rotated seeds back out, two positions per lookup
			const unsigned char* gp = W.L.mine + (q - (int32_t)K.k + 1);
			for (uint32_t p = 0; p < W.L.ngp; ++p) {
				const uint32_t dw = W.L.dcw[p];
				const uint32_t off = (gp[dw & 0xffffu] & 0xc0u) | ((gp[dw >> 16] >> 2) & 0x30u);
				const uint2 g = ld_h<C::one>(W.L.gapT + p * 256u + off);
				fs ^= g.x, rs ^= g.y;
			}
		}
		const uint32_t mn = C::one ? fs : (fs < rs ? fs : rs); // top bits of min(fh,rh) (of the spaced-seed values when gapped); one strand: of that strand
		if constexpr (C::dump)
			m = ballot(true);
		else if constexpr (C::hll)
			m = ballot(mn < W.S.hll_thr); // nthll: only a hash with enough leading zeros can raise a register
		else
			m = ballot(mn < W.S.lo0) | ballot((int32_t)mn >= W.S.lo1); // two v_cmp + s_or_b64 (mn carries the flipped bit)
		if constexpr (wc == RAGGED) m &= ballot(K.nextok <= q); // DIRTY: windows over a dirty byte are dropped by the resolve stage
	}
	push<C::dump>(K.hmask, m);
}

template <int kind>
__device__ __forceinline__ uint32_t group_idx(const Lds& L, const KState& K, int32_t q0, uint32_t& ain)
{
	ain = *reinterpret_cast<const uint32_t*>(L.mine + q0);
	if (kind == FILL) return ain & 0xc0c0c0c0u;
	uint32_t aout = 0;
	if (kind == MAIN || q0 + 3 >= (int32_t)K.k) {
		const uint32_t* p = reinterpret_cast<const uint32_t*>(L.mine + ((q0 - (int32_t)K.k) & ~3));
		// one funnel shift aligns the outgoing bytes to the group AND moves their codes from bits 7:6 to 5:4
		// (what spills over from the neighbouring bytes lands in bits 7:6 / 3:0..: 7:6 are replaced below, the
		// low nibble of a code byte holds nothing but its mark in bit 0, which is shifted out of the byte)
		aout = alignbit(p[1], p[0], 8u * K.shb + 2u);
		if (kind == MIXED && q0 < (int32_t)K.k) aout &= 0xffffffffu << (8 * ((int32_t)K.k - q0));
	}
	// bits 7:6 of every byte from ain (incoming code), bits 5:4 from the shifted outgoing code: one v_bfi_b32
	constexpr uint32_t M = 0xc0c0c0c0u;
	uint32_t idx4 = (ain & M) | (aout & ~M);
	asm volatile("" : "+v"(idx4)); // keep it ONE v_bfi_b32: stops hipcc from re-deriving byte 0 with three more ops
	return idx4;
}
struct Tab4 { uint2 t[4]; };
template <bool kOne>
__device__ __forceinline__ void issue(const unsigned char* tab, uint32_t idx4, Tab4& T)
{
	T.t[0] = ld_h<kOne>(tab + (idx4 & 0xffu));
	T.t[1] = ld_h<kOne>(tab + ((idx4 >> 8) & 0xffu));
	T.t[2] = ld_h<kOne>(tab + ((idx4 >> 16) & 0xffu));
	T.t[3] = ld_h<kOne>(tab + (idx4 >> 24));
}
// Spaced seed, equal lengths (the spaced value itself rolls): the terms of the bases whose term toggles during the 4 steps of the group at q0, two
// per lookup (SeedPlan: the boundaries of the mask's runs of '0's, and the window's ends where such a run touches them); ntcard's -g seed: one pair,
// the bases leaving / entering its don't-care block
template <bool kOne>
__device__ __forceinline__ void toggle_terms(const HfArgs& a, const Lds& L, int32_t k, int32_t q0, Tab4& TG)
{
#pragma unroll
	for (uint32_t p = 0; p < kMaxRollPairs; ++p) {
		if (p > 0 && p >= L.nroll) break;
		const uint32_t tw = a.roll_t[p];
		const int32_t o1 = q0 - k + (int32_t)(tw & 0xffffu), o2 = q0 - k + (int32_t)(tw >> 16);
		const uint32_t* p1 = reinterpret_cast<const uint32_t*>(L.mine + (o1 & ~3));
		const uint32_t* p2 = reinterpret_cast<const uint32_t*>(L.mine + (o2 & ~3));
		const uint32_t w1 = alignbyte(p1[1], p1[0], (uint32_t)o1 & 3u);
		const uint32_t w2 = alignbit(p2[1], p2[0], 8u * ((uint32_t)o2 & 3u) + 2u); // aligned and >> 2 in one funnel shift
		uint32_t ig = (w1 & 0xc0c0c0c0u) | (w2 & 0x3f3f3f3fu);
		asm volatile("" : "+v"(ig));
		Tab4 V;
		issue<kOne>(p == 0 ? L.tabG : L.rollT + (p - 1u) * 256u, ig, V);
#pragma unroll
		for (int b = 0; b < 4; ++b) {
			TG.t[b].x = p == 0 ? V.t[b].x : TG.t[b].x ^ V.t[b].x;
			TG.t[b].y = p == 0 ? V.t[b].y : TG.t[b].y ^ V.t[b].y;
		}
	}
}

// the 4-step groups g0 .. g1 - 1: THE per-base loop
template <class C, int wc, int kind>
__device__ __forceinline__ void walk_groups(const HfArgs& a, const Wave& W, KState& K, int32_t g0, int32_t g1)
{
	constexpr bool kGapRoll = C::spaced && wc != RAGGED; // equal lengths: the spaced value itself rolls
	for (int32_t g = g0; g < g1; ++g) {
		const int32_t q0 = g << 2;
		uint32_t ain;
		Tab4 T, TG = {};
		issue<C::one>(K.tabHb, group_idx<kind>(W.L, K, q0, ain), T);
		if constexpr (kGapRoll) toggle_terms<C::one>(a, W.L, (int32_t)K.k, q0, TG);
		auto steps = [&](auto book) { // book(b): the per-lane bookkeeping ahead of step b
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				book(b);
				roll<C::one, kGapRoll>(K, W.S, T.t[b], TG.t[b]);
				if (kind != FILL) record<C, wc>(W, K, q0 + b, kind == MAIN || q0 + b >= (int32_t)K.k - 1);
			}
		};
		uint64_t fixm = 0;
		if (wc == DIRTY) fixm = ballot((ain & 0x01010101u) != 0u);
		if (wc == RAGGED) // lanes that are shut off never trigger the extra work
			fixm = ballot((((ain & 0x01010101u) != 0u) | (K.endq < q0 + 4)) & (K.nextok != kShut));
		uint32_t fix = (uint32_t)(fixm | (fixm >> 32));
		asm volatile("" : "+s"(fix)); // opaque SGPR: the test below must stay a scalar branch
		// DIRTY: the marks only feed F1 (dirty windows are dropped by the resolve stage), so they are
		// booked in one rare divergent region ahead of the group and the steps stay on the fast path
		if (wc == DIRTY && fix) on_marks(K, q0, ain & 0x01010101u);
		// RAGGED: two copies of the group body behind ONE scalar branch: the common (no dirty byte, no read
		// end in this group) copy carries no per-lane bookkeeping at all
		if (wc == RAGGED && fix)
			steps([&](int b) {
				on_end(K, q0 + b);
				if ((ain >> (8 * b)) & 1u) on_mark(K, q0 + b);
			});
		else
			steps([](int) {});
	}
}
template <class C, int wc>
__device__ __forceinline__ void walk_single(const HfArgs& a, const Wave& W, KState& K, int32_t q) // one step outside the 4-step groups (q >= k - 1 only on the closed-form path)
{
	const unsigned char* const mine = W.L.mine;
	const int32_t k = (int32_t)K.k;
	const uint32_t ain = mine[q];
	if (wc != CLEAN) {
		if (wc == RAGGED) on_end(K, q);
		if (ain & 1u) on_mark(K, q);
	}
	const uint32_t off = (ain & 0xc0u) | (q >= k ? ((mine[q - k] >> 2) & 0x30u) : 0u);
	constexpr bool kGapRoll = C::spaced && wc != RAGGED; // only reached with q >= k (closed-form start)
	uint2 g = make_uint2(0u, 0u);
	if (kGapRoll)
		for (uint32_t p = 0; p < W.L.nroll; ++p) {
			const uint32_t tw = a.roll_t[p];
			const int32_t o1 = q - k + (int32_t)(tw & 0xffffu), o2 = q - k + (int32_t)(tw >> 16);
			const uint32_t og = (mine[o1] & 0xc0u) | ((mine[o2] >> 2) & 0x30u);
			const uint2 v = ld_h<C::one>((p == 0 ? W.L.tabG : W.L.rollT + (p - 1u) * 256u) + og);
			g.x ^= v.x, g.y ^= v.y;
		}
	roll<C::one, kGapRoll>(K, W.S, ld_h<C::one>(K.tabHb + off), g);
	record<C, wc>(W, K, q, q >= k - 1);
}

// Equal-length waves skip the k-1 window-filling steps: the H halves of window 0 come from the closed
// form over the first k bases (the resolve stage's pair table, 2 bases per lookup), which costs about
// half of rolling them in and far less for large k.  Steps k .. A-1 (A = k rounded up to a group
// boundary) run singly, the rest in 4-step groups; every step from k-1 on is recorded.
template <class C, int wc>
__device__ __forceinline__ void walk_equal(const HfArgs& a, Wave& W, KState& K)
{
	const int32_t k = (int32_t)K.k, maxq = K.maxq, full_groups = maxq >> 2;
	if (maxq < k) return;
	const auto h = closed_form<C::one, true, true>(reinterpret_cast<const uint32_t*>(W.L.mine), 0u, K.k, K.tp, [&](uint32_t i, uint32_t w) {
		if (wc == DIRTY && ballot((w & 0x01010101u) != 0u) != 0) on_marks(K, (int32_t)i, w & 0x01010101u); // marks among the first k bases only feed F1 (rare divergent region)
	});
	// high word of the 64-bit hash = (H << 1) | L[32]  ->  walk layout (H << 1) | H[30], plus the sample-bit flip
	K.fHd = ((h.fhi & ~1u) | (h.fhi >> 31)) ^ W.S.flipc;
	K.rHd = ((h.rhi & ~1u) | (h.rhi >> 31)) ^ W.S.flipc;
	record<C, wc>(W, K, k - 1, true);
	const int32_t A = (k + 3) & ~3;
	for (int32_t q = k; q < (A < maxq ? A : maxq); ++q)
		walk_single<C, wc>(a, W, K, q);
	if (A >= maxq) return compact<C>(a, W, K, maxq - 1);
	int32_t g = A >> 2, room = 7; // the first block also holds the (at most 4) steps recorded above
	for (;;) {
		const int32_t ge = g + room < full_groups ? g + room : full_groups;
		walk_groups<C, wc, MAIN>(a, W, K, g, ge);
		if (ge == full_groups) {
			if (ge - g == room && (maxq & 3) != 0) compact<C>(a, W, K, (ge << 2) - 1); // block is full: the tail gets its own
			for (int32_t q = full_groups << 2; q < maxq; ++q) // partial last group
				walk_single<C, wc>(a, W, K, q);
			compact<C>(a, W, K, maxq - 1);
			break;
		}
		compact<C>(a, W, K, (ge << 2) - 1);
		g = ge, room = 8;
	}
}
// Ragged waves roll every step from the poly-A start.  Group ranges: [0,e0) never emit and never see a real outgoing base; [e0,e1) are the (at most
// two) groups around steps k-1 and k; [e1, full_groups) are steady state
template <class C>
__device__ __forceinline__ void walk_ragged(const HfArgs& a, Wave& W, KState& K)
{
	const int32_t k = (int32_t)K.k, maxq = K.maxq, full_groups = maxq >> 2;
	const int32_t gk = (k - 1) >> 2, gm = (k + 3) >> 2; // group of step k-1; first group with q0 >= k
	const int32_t e0 = gk < full_groups ? gk : full_groups, e1 = gm < full_groups ? gm : full_groups;
	walk_groups<C, RAGGED, FILL>(a, W, K, 0, e0);
	// recorded steps start at qs = 4*e0 and are handled in blocks of 32 (8 groups): walk, then compact
	const int32_t nblk = (maxq - (e0 << 2) + 31) >> 5;
	for (int32_t blk = 0; blk < nblk; ++blk) {
		const int32_t gb = e0 + (blk << 3);
		const int32_t ge = gb + 8 < full_groups ? gb + 8 : full_groups;
		walk_groups<C, RAGGED, MIXED>(a, W, K, gb, ge < e1 ? ge : e1); // only the first block has MIXED groups
		walk_groups<C, RAGGED, MAIN>(a, W, K, gb > e1 ? gb : e1, ge);
		int32_t last = (ge << 2) - 1;
		if (blk == nblk - 1) {
			for (int32_t q = full_groups << 2; q < maxq; ++q) // partial last group
				walk_single<C, RAGGED>(a, W, K, q);
			last = maxq - 1;
		}
		compact<C>(a, W, K, last);
	}
}
// the walk of one k over the staged batch, compaction and full resolve rounds included; leaves the queue's rest and the wave's F1 in K
template <class C, int wc>
__device__ __forceinline__ void walk(const HfArgs& a, Wave& W, KState& K)
{
	if constexpr (wc == RAGGED)
		walk_ragged<C>(a, W, K);
	else
		walk_equal<C, wc>(a, W, K);
	if (wc == CLEAN) { // F1 is arithmetic there
		if (K.maxq >= (int32_t)K.k) K.f1_wave += (uint64_t)__popcll(ballot(true)) * (uint32_t)(K.maxq - (int32_t)K.k + 1);
	} else {
		if (K.nextok != kShut && K.endq > K.nextok) K.f1_lane += (uint32_t)(K.endq - K.nextok);
		uint32_t v = K.f1_lane;
		for (int o = 32; o > 0; o >>= 1)
			v += __shfl_xor(v, o);
		K.f1_wave += __builtin_amdgcn_readfirstlane(v);
	}
}

} // namespace

// kMulti = false: exactly one k (the loop over the k list folds away and every per-k value is a launch constant); the other parameters: Cfg, stage_batch
template <bool kMulti, int kMode, int kPref, bool kDump = false, bool kTiled = false, bool kOne = false, bool kSig = false>
__global__ __launch_bounds__(kPref <= 10 ? 1024 : 768) void sketch_hf_kernel(const HfArgs a)
{
#ifdef NTC_HF_CLOCKS
	const unsigned long long hc_t0 = __builtin_amdgcn_s_memrealtime();
#endif
	using C = Cfg<kMode, kDump, kOne, kSig>;
	const uint32_t n_k = kMulti ? a.n_k : 1u;
	extern __shared__ __align__(16) unsigned char smem[];
	__shared__ __align__(16) uint32_t tabH[kMaxFusedK][kMainSlots * 4];
	__shared__ __align__(16) uint32_t tabG[kMainSlots * 4];
	const uint32_t wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
	Wave W;
	// per fused plane (arrays of their own: indexed by the k loop, they must not share a struct with anything that has to stay in registers): F1, and for
	// signatures the wave's place in its current chunk of the value log, the entries left of the chunk (wave-uniform) and the values it has logged
	uint64_t f1_acc[kMaxFusedK] = {0, 0, 0, 0}, sig_at[kMaxFusedK] = {0, 0, 0, 0};
	uint32_t sig_room[kMaxFusedK] = {0, 0, 0, 0}, sig_vals[kMaxFusedK] = {0, 0, 0, 0}; // (a launch's windows per wave stay far below 2^32)
	W.lane = threadIdx.x & 63;
	W.S.init<C>(a);
	uint32_t t1_off[kMaxFusedK + 1]; // LDS offsets of the closed-form tables per fused k, [n_k] = total
	lds_setup<C>(a, n_k, smem, tabH, tabG, (int)wave, W, t1_off);
	__syncthreads();
	const uint32_t gwave = rfl(blockIdx.x * wpb + wave);
	W.log.open<C>(a, W.lane, gwave, gridDim.x * wpb);
	const int lane = W.lane;
	const uint32_t stride = a.stride, full_bytes = 64u * stride, n_pieces = stride >> 4; // bytes of a full batch; tiled: chunks per read
	W.can_prefetch = ((full_bytes + 1023u) >> 10) <= (uint32_t)kPref;
	uint4 pref[kPref];
	auto load_round = [&](uint64_t wb_, uint32_t c0) {
		if (kTiled) {
			const uint64_t r0 = wb_ * 64u;
			const unsigned char* src = a.slots + ((r0 / kTileReads) * n_pieces * kTileReads + (r0 % kTileReads) + (uint32_t)lane) * 16u;
#pragma unroll
			for (int c = 0; c < kPref; ++c)
				if (c0 + c < n_pieces) pref[c] = *reinterpret_cast<const uint4*>(src + (size_t)(c0 + c) * kTileReads * 16u);
			return;
		}
		const unsigned char* src = a.slots + wb_ * full_bytes;
#pragma unroll
		for (int c = 0; c < kPref; ++c) {
			const uint32_t off = lane * 16u + (c0 + c) * 1024u;
			if (off + 16u <= full_bytes) pref[c] = *reinterpret_cast<const uint4*>(src + off);
		}
	};
	auto store_round = [&](uint32_t c0, uint32_t& badacc) {
#pragma unroll
		for (int c = 0; c < kPref; ++c) {
			const uint32_t off = kTiled ? (uint32_t)lane * stride + (c0 + c) * 16u : lane * 16u + (c0 + c) * 1024u;
			if (kTiled ? c0 + c < n_pieces : off + 16u <= full_bytes) {
				uint4 v = pref[c];
				v.x = decode4(v.x, badacc), v.y = decode4(v.y, badacc);
				v.z = decode4(v.z, badacc), v.w = decode4(v.w, badacc);
				*reinterpret_cast<uint4*>(W.L.wdata + off) = v;
			}
		}
	};
	const uint64_t n_wb = (a.n_slots + 63) / 64;
	uint64_t wb_begin, wb_end;
	wave_share(n_wb, wpb, wave, wb_begin, wb_end);
	if (W.can_prefetch && wb_begin < wb_end && (kTiled || wb_begin * 64 + 64 <= a.n_slots)) load_round(wb_begin, 0);
	for (uint64_t wb = wb_begin; wb < wb_end; ++wb) {
		// Wave priorities follow the age of the work: staging (waits on memory anyway) 0, the walk 1, the walk after
		// its first compaction 2, compaction + resolve 3.  A batch that has been started gets finished ahead of
		// younger ones on the same SIMD instead of all four waves trading issue slots evenly: +13-15 % on genome-like
		// data (1.03 -> 0.90 ms per launch), -5 % on uniform data, which runs at the atomic-rate floor either way.
		// Slots too long for the register prefetch keep the staging at the walk's level (it would starve otherwise).
		if (W.can_prefetch) __builtin_amdgcn_s_setprio(0); // without the register prefetch the staging waits for its own loads: keep its rank
		stage_batch<kPref, kTiled>(a, W, wb, wb + 1 < wb_end ? wb + 1 : n_wb, n_wb, load_round, store_round);
		if (W.can_prefetch) __builtin_amdgcn_s_setprio(1);
		read_geometry(a, W);
		// every k of the list over the staged batch (ntRead's loop over kList, ntcard.cpp:147-158)
		for (uint32_t ki = 0; ki < n_k; ++ki) {
			KState K;
			const int wclass = k_begin<C>(a, W, ki, t1_off[ki], sig_at[ki], sig_room[ki], K);
			if (wclass == CLEAN)
				walk<C, CLEAN>(a, W, K);
			else if (wclass == DIRTY)
				walk<C, DIRTY>(a, W, K);
			else
				walk<C, RAGGED>(a, W, K);
			if (K.npend != 0) resolve_round<C>(a, W, K, K.pend, K.npend); // leftovers of the compaction queue: one last, partially filled round
			f1_acc[ki] += K.f1_wave;
			if constexpr (kSig) sig_at[ki] = K.sig_at, sig_room[ki] = K.sig_room, sig_vals[ki] += K.sig_vals;
		}
	}
	// epilogue: F1, the fill of the wave's log region, the unused rest of its last signature chunks
	for (uint32_t j = 0; j < n_k; ++j)
		if (W.lane == 0 && f1_acc[j]) atomicAdd(a.ks[j].f1, (unsigned long long)f1_acc[j]);
	W.log.close(a, W.lane);
	if constexpr (kSig)
		for (uint32_t j = 0; j < n_k; ++j) {
			for (uint32_t i = (uint32_t)W.lane; i < sig_room[j]; i += 64u)
				if (sig_at[j] + i < a.sig_cap) a.sig_log[j][sig_at[j] + i] = 0ull;
			if (W.lane == 0 && sig_vals[j] != 0u) atomicAdd(a.sig_cursor[j] + 2, (unsigned long long)sig_vals[j]);
		}
#ifdef NTC_HF_CLOCKS
	if (W.lane == 0 && gwave < 8192u) {
		g_hf_clocks[2 * gwave] = hc_t0;
		g_hf_clocks[2 * gwave + 1] = __builtin_amdgcn_s_memrealtime();
	}
#endif
}

// Every instantiation of K1, once: X(kMulti, kMode, kPref, kDump, kTiled, kOne, kSig).  Dispatch (launch_sketch_hf) and the dynamic-LDS attribute
// (set_sketch_hf_smem_limit) both read the table below.  The order of the rows is the order the kernels are emitted in.
#define HF_VARIANTS(X)                                                                                                                  \
	/* NTC_FLAG_SIGNATURE: row slots, the 10-chunk prefetch only */                                                                     \
	X(false, 1, 10, false, false, true, true) X(false, 1, 10, false, false, false, true) X(true, 0, 10, false, false, true, true)       \
	X(true, 0, 10, false, false, false, true) X(false, 0, 10, false, false, true, true) X(false, 0, 10, false, false, false, true)      \
	/* one strand: what a strand engine can reach (its tiled batches are re-laid out as row slots) */                                   \
	X(false, 3, 10, false, false, true, false) X(false, 2, 10, false, false, true, false) X(false, 1, 10, true, false, true, false)     \
	X(false, 0, 10, true, false, true, false) X(false, 1, 10, false, false, true, false) X(true, 0, 16, false, false, true, false)      \
	X(true, 0, 10, false, false, true, false) X(false, 0, 16, false, false, true, false) X(false, 0, 10, false, false, true, false)     \
	/* canonical: hash dump, nthll, spaced seed, tiled staging, row slots */                                                            \
	X(false, 1, 10, true, false, false, false) X(false, 0, 10, true, false, false, false) X(false, 3, 10, false, false, false, false)   \
	X(false, 2, 10, false, false, false, false) X(false, 1, 10, false, false, false, false) X(true, 0, 16, false, true, false, false)   \
	X(true, 0, 10, false, true, false, false) X(false, 0, 16, false, true, false, false) X(false, 0, 10, false, true, false, false)     \
	X(true, 0, 16, false, false, false, false) X(true, 0, 10, false, false, false, false) X(false, 0, 16, false, false, false, false)   \
	X(false, 0, 10, false, false, false, false)

struct HfVariant {
	bool multi;
	int mode, pref;
	bool dump, tiled, one, sig;
	void (*fn)(const HfArgs);
};
#define HF_ROW(multi, mode, pref, dump, tiled, one, sig) { multi, mode, pref, dump, tiled, one, sig, &sketch_hf_kernel<multi, mode, pref, dump, tiled, one, sig> },
static const HfVariant kHfVariants[] = { HF_VARIANTS(HF_ROW) };
#undef HF_ROW
constexpr uint32_t kHfRows = sizeof kHfVariants / sizeof kHfVariants[0];

// What launch_sketch_hf has dispatched, per row of the table (k1_variant_stats; process-wide, host only): engines launch from several threads, hence
// relaxed atomics — a reader sees every count, and the last_* words of SOME launch each
struct HfRowStats {
	std::atomic<uint64_t> launches{0}, regime[kK1Regimes]{}, last_n_slots{0};
	std::atomic<uint32_t> last_grid{0}, last_wpb{0}, last_stride{0};
};
static HfRowStats g_hf_stats[kHfRows];

// the regimes of a launch, from the same words the kernel derives them from (nchunk, can_prefetch, nvalid, wpb % 4, the wave-batch shares)
static void note_hf_launch(uint32_t row, const HfArgs& a, unsigned grid, unsigned wpb, int pref)
{
	const uint32_t nchunk = (64u * a.stride + 1023u) >> 10;
	const uint64_t n_wb = (a.n_slots + 63) / 64, waves = (uint64_t)grid * wpb;
	const bool in[kK1Regimes] = { nchunk <= (uint32_t)pref, nchunk > (uint32_t)pref, a.n_slots % 64 != 0, a.meta != nullptr,
	                              wpb % 4u != 0u,           n_wb < waves,            n_wb >= 2 * waves,    a.log_regions != 0 };
	HfRowStats& s = g_hf_stats[row];
	constexpr auto relaxed = std::memory_order_relaxed;
	s.launches.fetch_add(1, relaxed);
	for (int i = 0; i < kK1Regimes; ++i)
		if (in[i]) s.regime[i].fetch_add(1, relaxed);
	s.last_grid.store(grid, relaxed);
	s.last_wpb.store(wpb, relaxed);
	s.last_stride.store(a.stride, relaxed);
	s.last_n_slots.store(a.n_slots, relaxed);
}

bool k1_variant_stats(uint32_t row, ntc_k1_variant_info& o)
{
	if (row >= kHfRows) return false;
	const HfVariant& v = kHfVariants[row];
	const HfRowStats& s = g_hf_stats[row];
	constexpr auto relaxed = std::memory_order_relaxed;
	std::memset(&o, 0, sizeof o);
	o.multi = v.multi, o.mode = (uint8_t)v.mode, o.pref = (uint8_t)v.pref, o.dump = v.dump, o.tiled = v.tiled, o.one = v.one, o.sig = v.sig;
	o.launches = s.launches.load(relaxed);
	for (int i = 0; i < kK1Regimes; ++i)
		o.regime[i] = s.regime[i].load(relaxed);
	o.last_grid = s.last_grid.load(relaxed);
	o.last_wpb = s.last_wpb.load(relaxed);
	o.last_stride = s.last_stride.load(relaxed);
	o.last_n_slots = s.last_n_slots.load(relaxed);
	return true;
}

hipError_t launch_sketch_hf(const HfArgs& a, unsigned grid, unsigned waves_per_block, size_t smem, hipStream_t st)
{
	if (a.tiled != 0u && (a.dump != nullptr || a.gap != 0 || a.hll_bits != 0)) return hipErrorInvalidValue; // (tiled staging: plain k-mer mode only)
	if (a.ks[0].strand > 2u || (a.ks[0].strand != 0u && a.tiled != 0u)) return hipErrorInvalidValue; // (one strand: row slots)
	if (a.hll_bits != 0 && (a.n_k != 1 || a.dump != nullptr || a.hll_thr == nullptr)) return hipErrorInvalidValue; // (nthll: one plane per launch)
	// NTC_FLAG_SIGNATURE: row slots only (tiled batches are re-laid out first)
	if (a.sig_cap != 0 && (a.tiled != 0u || a.dump != nullptr || a.hll_bits != 0 || a.sig_chunk < 64u)) return hipErrorInvalidValue;
	// the wanted row.  A spaced seed or a dump takes the single-k form whatever n_k; the 16-chunk prefetch is for plain k-mer mode without signatures
	// (their slots beyond the 10-chunk prefetch stage with blocking loads)
	const bool sig = a.sig_cap != 0, one = a.ks[0].strand != 0u, dump = a.dump != nullptr, tiled = a.tiled != 0u;
	const int mode = (a.gap != 0 ? 1 : 0) | (a.hll_bits != 0 ? 2 : 0);
	const bool multi = a.n_k > 1 && mode == 0 && !dump;
	const int pref = (mode == 0 && !dump && !sig && sketch_hf_deep_prefetch(a.stride) && waves_per_block <= 12) ? 16 : 10;
	for (const HfVariant& v : kHfVariants)
		if (v.multi == multi && v.mode == mode && v.pref == pref && v.dump == dump && v.tiled == tiled && v.one == one && v.sig == sig) {
			note_hf_launch((uint32_t)(&v - kHfVariants), a, grid, waves_per_block, pref);
			hipLaunchKernelGGL(v.fn, dim3(grid), dim3(64u * waves_per_block), smem, st, a);
			return hipGetLastError();
		}
	return hipErrorInvalidValue;
}

// validation: per read, the hashes of the valid windows in window order (the layout ntc_hash_dump_device documents)
__global__ __launch_bounds__(256) void compact_dump_kernel(const uint64_t* __restrict__ full, const uint32_t* __restrict__ valid, uint64_t n_reads,
                                                           uint32_t n_win, uint32_t max_win, uint64_t* __restrict__ out, uint32_t* __restrict__ count)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const uint32_t vw = (n_win + 31u) >> 5;
	uint32_t n = 0;
	for (uint32_t w = 0; w < n_win; ++w)
		if ((valid[r * vw + (w >> 5)] >> (w & 31u)) & 1u) {
			if (n < max_win) out[r * max_win + n] = full[r * n_win + w];
			++n;
		}
	count[r] = n;
}
hipError_t launch_compact_dump(const uint64_t* full, const uint32_t* valid, uint64_t n_reads, uint32_t n_win, uint32_t max_win, uint64_t* out,
                               uint32_t* count, hipStream_t st)
{
	hipLaunchKernelGGL(compact_dump_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st, full, valid, n_reads, n_win, max_win, out, count);
	return hipGetLastError();
}

// slots of 164..256 B: a 16-chunk register prefetch covers them (the 10-chunk one would fall back to blocking loads)
bool sketch_hf_deep_prefetch(uint32_t stride) { return 64u * stride > 10u * 1024u && 64u * stride <= 16u * 1024u; }

hipError_t set_sketch_hf_smem_limit(size_t smem)
{
	for (const HfVariant& v : kHfVariants) {
		const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void*>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		if (rc != hipSuccess) return rc;
	}
	return hipSuccess;
}

} // namespace ntc

int ntc_internal_fail(int code, const char* fmt, ...); // ntc_lifecycle.hip: sets ntc_last_error()

extern "C" int ntc_k1_variant_stats(uint32_t row, ntc_k1_variant_info* out)
{
	if (!out) return ntc_internal_fail(NTC_ERR_ARG, "ntc_k1_variant_stats: null argument");
	if (!ntc::k1_variant_stats(row, *out)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_k1_variant_stats: row %u: the table has fewer rows", row);
	return 0;
}
