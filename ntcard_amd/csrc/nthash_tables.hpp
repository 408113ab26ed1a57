// nthash_tables.hpp — host-side derivation of the per-k lookup tables the HIP kernels stage in LDS.
//
// Everything is derived from the four base seeds (nthash.hpp:25-28) and the split-rotate rule
// (nthash.hpp:186-217: low 33 bits and high 31 bits rotate independently); the reference's
// msTab33r/msTab31l tables (nthash.hpp:66-183) are exactly srol^i(seed) and are NOT copied.
//
// Device representation of one strand's 64-bit hash x = L | H<<33 (L: 33 bits, H: 31 bits):
//   lo : L[0..31]
//   B  : one bit, L[32]   (forward strand keeps it in bit 31 of a scratch register, reverse in bit 0)
//   Hd : (H << 1) | H[30] (bit 0 duplicates bit 31, so both 31-bit rotates are 2 VALU ops and
//                          unsigned compares of Hd order exactly like H)
// One table entry per (in-base, out-base) pair:
//   A[slot] = { Tf.lo, Tf.Hd, Tr.lo, Tr.Hd }   (one ds_read_b128)
//   B[slot] = bit31: Tf.L[32], bit0: Tr.L[32]  (one ds_read_b32)
// with  Tf = seed(in) ^ srol^k(seed(out))            (NTF64 roll, nthash.hpp:242-248)
//       Tr = comp(out) ^ srol^k(comp(in))            (NTR64 roll, nthash.hpp:251-257, XOR-before-rotate)
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ntc {

constexpr uint64_t kSeed[4] = { 0x3c8bfbb395c60474ULL,   // A
	                            0x3193c18562a02b4cULL,   // C
	                            0x20323ed082572324ULL,   // G
	                            0x295549f54be24456ULL }; // T (and U)

// code: A=0 C=1 G=2 T=3; complement = 3 - code
inline uint64_t seed_of(unsigned code) { return kSeed[code & 3]; }
inline uint64_t comp_of(unsigned code) { return kSeed[3 - (code & 3)]; }

inline uint64_t srol(uint64_t x, unsigned n)
{
	const uint64_t M33 = (1ULL << 33) - 1, M31 = (1ULL << 31) - 1;
	uint64_t lo = x & M33, hi = x >> 33;
	unsigned a = n % 33u, b = n % 31u;
	if (a) lo = ((lo << a) | (lo >> (33u - a))) & M33;
	if (b) hi = ((hi << b) | (hi >> (31u - b))) & M31;
	return lo | (hi << 33);
}

inline uint32_t lo_of(uint64_t x) { return (uint32_t)x; }
inline uint32_t b32_of(uint64_t x) { return (uint32_t)((x >> 32) & 1u); }
inline uint32_t hd_of(uint64_t x)
{
	uint32_t h = (uint32_t)(x >> 33); // 31 bits
	return (h << 1) | (h >> 30);
}

// slots 0..15: in*4+out (steady state); slots 16..19: in with "no out base yet" (window filling)
constexpr int kMainSlots = 16;
constexpr int kSlots = 20;

struct alignas(16) HashTables {
	uint32_t A[kSlots][4]; // {Tf.lo, Tf.Hd, Tr.lo, Tr.Hd}
	uint32_t B[kSlots][4]; // [0] = bit31:Tf.L[32] | bit0:Tr.L[32]; [1..3] spare (gap tables reuse)
};

inline void build_tables(unsigned k, HashTables& t)
{
	std::memset(&t, 0, sizeof t);
	for (int slot = 0; slot < kSlots; ++slot) {
		unsigned in = slot < kMainSlots ? (unsigned)slot >> 2 : (unsigned)slot - kMainSlots;
		bool has_out = slot < kMainSlots;
		unsigned out = (unsigned)slot & 3;
		uint64_t tf = seed_of(in) ^ (has_out ? srol(seed_of(out), k) : 0);
		uint64_t tr = (has_out ? comp_of(out) : 0) ^ srol(comp_of(in), k);
		t.A[slot][0] = lo_of(tf);
		t.A[slot][1] = hd_of(tf);
		t.A[slot][2] = lo_of(tr);
		t.A[slot][3] = hd_of(tr);
		t.B[slot][0] = (b32_of(tf) << 31) | b32_of(tr);
	}
}

// Strand registers (device layout) of the hash of k consecutive 'A' bases — the state a rolling walk
// starts every read from, with 'A' as the outgoing base of its first k steps: {flo, fB, fHd, rlo, rB, rHd}.
inline void poly_a_state(unsigned k, uint32_t out[6])
{
	uint64_t fh = 0, rh = 0;
	for (unsigned i = 0; i < k; ++i) {
		fh ^= srol(seed_of(0), i);
		rh ^= srol(comp_of(0), i);
	}
	out[0] = lo_of(fh);
	out[1] = b32_of(fh) << 31;
	out[2] = hd_of(fh);
	out[3] = lo_of(rh);
	out[4] = b32_of(rh);
	out[5] = hd_of(rh);
}

// Closed-form table of the resolve stage, two bases per entry: entry (j, a, b) covers window positions 2j, 2j+1
//   fwd = srol^(k-1-2j)(seed(a)) ^ srol^(k-2-2j)(seed(b)),  rev = srol^(2j)(comp(a)) ^ srol^(2j+1)(comp(b))
// as {fwd.lo, fwd.hi, rev.lo, rev.hi} (nthash.hpp:220-239: fh = XOR_i srol^(k-1-i) seed(c_i), rh = XOR_i srol^i comp(c_i)).
// For odd k the last pair has no second base (its b term is dropped).  Entry offset: j*256 + (a*4+b)*16 bytes.
inline unsigned t2_pairs(unsigned k) { return (k + 1) / 2; }
// A spaced seed as a mask of k characters: '1' = the base at that window offset enters the hash, '0' = don't care
// (stHashIterator::parseSeed, stHashIterator.hpp:23-33).  ntcard's -g seed is 1^((k-g)/2) 0^g 1^((k-g)/2) (ntcard.cpp:407-413).
inline std::string gap_mask(unsigned k, unsigned gap)
{
	std::string m(k, '1');
	for (unsigned i = (k - gap) / 2; i < (k - gap) / 2 + gap; ++i)
		m[i] = '0';
	return m;
}
// mask == nullptr: every position is cared for
inline void build_t2(unsigned k, uint32_t* out /* t2_pairs(k)*16*4 dwords */, const char* mask)
{
	auto dc = [&](unsigned i) { return mask != nullptr && mask[i] == '0'; }; // don't-care position of a spaced seed
	for (unsigned j = 0; j < t2_pairs(k); ++j)
		for (unsigned a = 0; a < 4; ++a)
			for (unsigned b = 0; b < 4; ++b) {
				const unsigned i0 = 2 * j, i1 = 2 * j + 1;
				uint64_t f = srol(seed_of(a), k - 1 - i0), r = srol(comp_of(a), i0);
				if (dc(i0)) f = r = 0; // spaced seed: this base does not enter the hash (nthash.hpp:641-646)
				if (i1 < k && !dc(i1)) {
					f ^= srol(seed_of(b), k - 1 - i1);
					r ^= srol(comp_of(b), i1);
				}
				uint32_t* e = out + ((j * 16) + a * 4 + b) * 4;
				e[0] = (uint32_t)f;
				e[1] = (uint32_t)(f >> 32);
				e[2] = (uint32_t)r;
				e[3] = (uint32_t)(r >> 32);
			}
}
inline void build_t2(unsigned k, uint32_t* out, unsigned gap_first = 0, unsigned gap = 0)
{
	const std::string m = gap_mask(k, gap);
	(void)gap_first; // (always (k - gap) / 2)
	build_t2(k, out, gap ? m.c_str() : nullptr);
}

// Closed-form table of K1b's resolve stage, FOUR bases per entry, indexed by a packed byte of 2-bit codes in
// code2 order (code2 = (ascii >> 1) & 3: A=0 C=1 T/U=2 G=3; base t of the group in bits 2t+1:2t):
// entry (g, v) = XOR over t < 4, i = 4 g + t < k of  srol^(k-1-i)(seed(c_t))  and  srol^i(comp(c_t))   (nthash.hpp:220-239)
inline unsigned t4_groups(unsigned k) { return (k + 3) / 4; }
inline void build_t4(unsigned k, uint32_t* out /* t4_groups(k)*256*4 dwords */, const char* mask)
{
	static const unsigned code_of_code2[4] = { 0, 1, 3, 2 }; // code2 -> the A C G T numbering of seed_of()
	for (unsigned g = 0; g < t4_groups(k); ++g)
		for (unsigned v = 0; v < 256; ++v) {
			uint64_t f = 0, r = 0;
			for (unsigned t = 0; t < 4; ++t) {
				const unsigned i = 4 * g + t;
				if (i >= k) break;
				if (mask != nullptr && mask[i] == '0') continue; // spaced seed: a don't-care position (nthash.hpp:641-646)
				const unsigned c = code_of_code2[(v >> (2 * t)) & 3u];
				f ^= srol(seed_of(c), k - 1 - i);
				r ^= srol(comp_of(c), i);
			}
			uint32_t* e = out + ((size_t)g * 256 + v) * 4;
			e[0] = (uint32_t)f;
			e[1] = (uint32_t)(f >> 32);
			e[2] = (uint32_t)r;
			e[3] = (uint32_t)(r >> 32);
		}
}
inline void build_t4(unsigned k, uint32_t* out, unsigned gap_first = 0, unsigned gap = 0)
{
	const std::string m = gap_mask(k, gap);
	(void)gap_first; // (always (k - gap) / 2)
	build_t4(k, out, gap ? m.c_str() : nullptr);
}

// Spaced-seed filter table: for the p-th PAIR of don't-care positions (i, i+1), entry (a, b) holds the H halves
// (Hd layout) of  srol^(k-1-i)(seed(a)) ^ srol^(k-2-i)(seed(b))  and  srol^i(comp(a)) ^ srol^(i+1)(comp(b)),
// i.e. what NTMSM64 XORs out of fh / rh (nthash.hpp:641-646).  16-byte stride: {f.Hd, r.Hd, 0, 0}.
inline void build_gap_table(unsigned k, unsigned gap_first, unsigned gap, uint32_t* out /* ceil(gap/2)*16*4 dwords */)
{
	for (unsigned p = 0; p < (gap + 1) / 2; ++p)
		for (unsigned a = 0; a < 4; ++a)
			for (unsigned b = 0; b < 4; ++b) {
				const unsigned i0 = gap_first + 2 * p, i1 = i0 + 1;
				uint64_t f = srol(seed_of(a), k - 1 - i0), r = srol(comp_of(a), i0);
				if (i1 < gap_first + gap) {
					f ^= srol(seed_of(b), k - 1 - i1);
					r ^= srol(comp_of(b), i1);
				}
				uint32_t* e = out + ((p * 16) + a * 4 + b) * 4;
				e[0] = hd_of(f);
				e[1] = hd_of(r);
				e[2] = e[3] = 0;
			}
}

// Rolling form of the spaced seed (equal-length waves): shifting the window by one base changes four terms — the
// incoming and outgoing base (the ordinary step table) plus the base that leaves the don't-care block at its low
// end (a, window index gap_first -> gap_first-1, now cared for) and the one that enters it at its high end
// (b, index gap_first+gap -> gap_first+gap-1).  Entry (a, b): {f, r} H halves (Hd layout) of
//   f: srol^(k-gap_first)(seed(a)) ^ srol^(k-gap_first-gap)(seed(b))        (XORed in after the forward rotate)
//   r: srol^(gap_first)(comp(a))   ^ srol^(gap_first+gap)(comp(b))          (XORed in before the reverse rotate)
inline void build_gap_roll_table(unsigned k, unsigned gap_first, unsigned gap, uint32_t out[16][2])
{
	for (unsigned a = 0; a < 4; ++a)
		for (unsigned b = 0; b < 4; ++b) {
			const uint64_t f = srol(seed_of(a), k - gap_first) ^ srol(seed_of(b), k - gap_first - gap);
			const uint64_t r = srol(comp_of(a), gap_first) ^ srol(comp_of(b), gap_first + gap);
			out[a * 4 + b][0] = hd_of(f);
			out[a * 4 + b][1] = hd_of(r);
		}
}

// ---- general spaced seeds (masks): the tables of K1's spaced-seed mode ----
//
// Closed-form XOR-out (ragged and dirty-free walks of unequal length): the don't-care offsets d_0 < d_1 < ... are taken in
// PAIRS (d_2p, d_2p+1); pair p has a table like build_gap_table's, entry (a, b) = the H halves of
//   srol^(k-1-d)(seed(a)) ^ srol^(k-1-d')(seed(b))  and  srol^d(comp(a)) ^ srol^d'(comp(b))      (nthash.hpp:641-646)
// and a position word d | d' << 16 (an odd last offset pairs with itself and has no b term).
//
// Rolling form (equal-length waves): one step of the plain roll moves every base one window offset down; a base whose
// new offset j (-1 .. k-1) is cared for now but was not before, or the other way round, toggles one term:
//   j = -1     (the outgoing base)     when mask[0] == '0'   (the plain roll removed a term that was never there)
//   0 <= j < k-1                       when mask[j] != mask[j+1]
//   j = k - 1  (the incoming base)     when mask[k-1] == '0' (the plain roll added a term that must not be there)
// With t = j + 1 (the byte q - k + t of step q), the toggled term is  f: srol^(k-t)(seed(c)) (XORed after the forward rotate),
// r: srol^t(comp(c)) (XORed before the reverse rotate).  An interior run of '0's toggles twice per step (exactly the pair
// build_gap_roll_table tabulates for ntcard's -g seed), a run at either end of the window twice as well (its inner boundary
// and the end's own correction).  The toggles are looked up two at a time, one table of 16 (a, b) entries per pair.
constexpr unsigned kMaxRollPairs = 4; // a mask with more toggle pairs walks every wave with the closed-form XOR-out (mask mode)

struct SeedPlan {
	uint32_t k = 0, n_dc = 0;          // window length, don't-care positions
	uint32_t n_roll = 0;               // toggle pairs of the rolling form (1 .. kMaxRollPairs); 0: the closed-form XOR-out in every wave
	uint32_t roll_t[kMaxRollPairs] = {}; // toggle pair p: t_a | t_b << 16
	uint32_t tabg[16][2] = {};         // toggle pair 0: {f, r} H halves per (a, b); pairs 1.. are in `blob`
	// what K1 stages in LDS behind its closed-form tables: [ceil(n_dc/2)][16] x {f.Hd, r.Hd, 0, 0} XOR-out tables,
	// [n_roll - 1][16] x {f.Hd, r.Hd, 0, 0} toggle tables, [ceil(n_dc/2)] position words, zero padding to 16 B
	std::vector<uint32_t> blob;
	uint32_t extra_bytes() const { return (uint32_t)(blob.size() * 4) - (n_dc + 1) / 2 * 256u; } // the part behind the XOR-out tables
};

// mask: k characters of '0' / '1' (validated by the caller)
inline void build_seed_plan(const std::string& mask, SeedPlan& sp)
{
	const unsigned k = (unsigned)mask.size();
	sp = SeedPlan();
	sp.k = k;
	std::vector<unsigned> dc, tog;
	for (unsigned i = 0; i < k; ++i)
		if (mask[i] == '0') dc.push_back(i);
	sp.n_dc = (uint32_t)dc.size();
	if (mask[0] == '0') tog.push_back(0);
	for (unsigned j = 0; j + 1 < k; ++j)
		if (mask[j] != mask[j + 1]) tog.push_back(j + 1);
	if (mask[k - 1] == '0') tog.push_back(k);
	const unsigned npairs = ((unsigned)tog.size() + 1) / 2;
	sp.n_roll = npairs <= kMaxRollPairs ? npairs : 0;
	auto hd2 = [&](uint64_t f, uint64_t r, uint32_t* e) {
		e[0] = hd_of(f);
		e[1] = hd_of(r);
		e[2] = e[3] = 0;
	};
	const unsigned ngp = (sp.n_dc + 1) / 2, nrx = sp.n_roll > 1 ? sp.n_roll - 1 : 0;
	const size_t words = (size_t)(ngp + nrx) * 64 + ((ngp + 3) / 4) * 4;
	sp.blob.assign(words, 0u);
	for (unsigned p = 0; p < ngp; ++p) {
		const unsigned d0 = dc[2 * p], d1 = 2 * p + 1 < dc.size() ? dc[2 * p + 1] : d0;
		for (unsigned a = 0; a < 4; ++a)
			for (unsigned b = 0; b < 4; ++b) {
				uint64_t f = srol(seed_of(a), k - 1 - d0), r = srol(comp_of(a), d0);
				if (d1 != d0) {
					f ^= srol(seed_of(b), k - 1 - d1);
					r ^= srol(comp_of(b), d1);
				}
				hd2(f, r, sp.blob.data() + ((size_t)p * 16 + a * 4 + b) * 4);
			}
		sp.blob[(size_t)(ngp + nrx) * 64 + p] = d0 | (d1 << 16);
	}
	for (unsigned p = 0; p < sp.n_roll; ++p) {
		const unsigned ta = tog[2 * p], tb = 2 * p + 1 < tog.size() ? tog[2 * p + 1] : ta;
		sp.roll_t[p] = ta | (tb << 16);
		for (unsigned a = 0; a < 4; ++a)
			for (unsigned b = 0; b < 4; ++b) {
				uint64_t f = srol(seed_of(a), k - ta), r = srol(comp_of(a), ta);
				if (tb != ta) {
					f ^= srol(seed_of(b), k - tb);
					r ^= srol(comp_of(b), tb);
				}
				if (p == 0) {
					sp.tabg[a * 4 + b][0] = hd_of(f);
					sp.tabg[a * 4 + b][1] = hd_of(r);
				} else {
					hd2(f, r, sp.blob.data() + ((size_t)(ngp + p - 1) * 16 + a * 4 + b) * 4);
				}
			}
	}
}

// ---- one strand (NTC_FLAG_STRAND_FORWARD / _REVERSE): the tables of K1's one-strand instantiations ----
//
// The one-strand kernel reads the FIRST half of every table entry and nothing else, so forward against reverse is
// decided here: the wanted strand's words are moved to the front of each entry (strand: 0 canonical = leave the
// tables alone, 1 forward, 2 reverse).  It rolls one form for both strands, x' = rot(x) ^ T, rot = rotl31 forward and
// rotr31 reverse.  NTR64 (nthash.hpp:251-257) XORs before it rotates, rh' = rotr(rh ^ Tr) = rotr(rh) ^ rotr(Tr): the
// reverse strand's STEP terms (HfK::tabh, the toggle tables of a spaced seed) are therefore handed over rotated
// right by one; the closed-form terms (build_t2, the XOR-out tables) apply to the value as it stands and are not.
inline uint32_t hd_rotr(uint32_t hd)
{
	uint32_t h = hd >> 1; // 31 bits
	h = (h >> 1) | ((h & 1u) << 30);
	return (h << 1) | (h >> 30);
}
inline void strand_t2(unsigned k, uint32_t* t2 /* build_t2's output */, unsigned strand)
{
	if (strand != 2) return; // (forward: already in front)
	for (size_t e = 0; e < (size_t)t2_pairs(k) * 16; ++e) {
		t2[e * 4 + 0] = t2[e * 4 + 2];
		t2[e * 4 + 1] = t2[e * 4 + 3];
	}
}
inline void strand_seed_plan(SeedPlan& sp, unsigned strand)
{
	if (strand != 2 || sp.k == 0) return;
	const unsigned ngp = (sp.n_dc + 1) / 2, nrx = sp.n_roll > 1 ? sp.n_roll - 1 : 0;
	for (size_t e = 0; e < (size_t)ngp * 16; ++e) // XOR-out tables: as they are
		sp.blob[e * 4] = sp.blob[e * 4 + 1];
	for (size_t e = (size_t)ngp * 16; e < (size_t)(ngp + nrx) * 16; ++e) // toggle tables of pairs 1 ..: rotated
		sp.blob[e * 4] = hd_rotr(sp.blob[e * 4 + 1]);
	for (unsigned e = 0; e < 16; ++e)
		sp.tabg[e][0] = hd_rotr(sp.tabg[e][1]);
}

} // namespace ntc
