// ntc_bloom_walk.hpp — what the plain Bloom filters (ntc_bloom.hip), the counting filters (ntc_cbloom.hip) and the blocked filters (ntc_bbloom.hip)
// share: the remainder by the filter's size, the multi-hash, the argument checks, THE WALK over every window of a device-resident input (DESIGN.md §4
// "Bloom filters") and the layer between the walk and a KIND of filter.  A kind is a VIEW: a small struct passed by value — the filter's pointer and its
// hashes — with the per-value operations the kind has (BitsView here, BlockedView in ntc_bbloom.hpp, CountersView in ntc_cbloom.hip):
//   void     View::insert(uint64_t h0) const         every kind
//   bool     View::test(uint64_t h0) const           the bit kinds: whether all bits of h0 are set
//   uint32_t View::count(uint64_t h0, floor) const   the counting kind
//   unsigned char View::answer(uint64_t h0) const    what a query over given h_0 values writes per value: test as 0 / 1, or the count
// InsertAct<View>, TestAct<View> and the two kernels over given h_0 values are templates over the view; the kinds differ by that type and nowhere else.
// What is done with a window's value is a template parameter of the walk kernel, an action `Act`:
//   Act::kMode                         kWalkTotal    r = act(h0) is added to one total per call (an insert: 1 per window; the solid insert: 1 per window
//                                                    that passed)
//                                      kWalkPerSeq   per sequence: its windows, and the sum of r = act(h0) over them (a query: r = hit)
//                                      kWalkProfile  r = act(h0) is the byte of the window's START position; every position of [0, n) gets a byte
//   uint32_t Act::operator()(uint64_t h0) const      the action on the value of one window
//
// The walk: the bytes [offsets[0], offsets[n_seqs]) are positions p = 0 .. n - 1; block b = the window STARTS [b B, (b + 1) B), B = NTC_BLOOM_BLOCK.  A
// workgroup of 256 lanes
//   stage   loads the B + k - 1 bytes its windows cover with 16-byte loads from the 16-byte grid of the source (lead = the source address mod 16, the
//           same for every block since 16 | B) and writes them to LDS as CODES: 0 .. 3 = A C G T/U, 4 = no base (N, IUPAC, anything else, and every
//           position outside [0, n))
//   mark    ORs 8 into the code of every position behind the block's first where a sequence starts: the sequences come from a device copy of the offsets,
//           found by one binary search per workgroup
//   walk    a lane takes 16 consecutive window starts: it rolls over their 16 + k - 1 codes, `run` = the bases seen since the last start or non-base.
//           While run < k the step has no outgoing base (the window fills), from then on it is the roll of nthash.hpp:242-257; a window is emitted when
//           run >= k and its start is one of the lane's.  A start or a non-base sets run, fh and rh to zero.
// kWalkPerSeq keeps (windows, sum) of the lane's current sequence in registers, adds them to a table in LDS indexed by the sequence's number behind the
// block's first (global atomics behind the table's end) and the workgroup adds every used entry to the output once.
// kWalkProfile: a lane knows a window only at its END, so it holds the 16 bytes of its starts in registers and stores them once, 16 bytes wide where the
// output address allows, never outside [0, n); a lane none of whose windows lies inside the input still owns — and writes — the zeros of its positions.
#pragma once
#include <algorithm>

#include "ntc_engine.hpp"

namespace ntc_bloom {

using ntc_eng::fail;
using ntc_eng::kMaxK;

constexpr uint32_t kBlock = NTC_BLOOM_BLOCK; // window starts per workgroup
constexpr uint32_t kRun = kBlock / 256u;     // consecutive windows per lane
constexpr uint32_t kStageBytes = 16u * ((15u + kBlock + kMaxK - 1u + 15u) / 16u);
constexpr uint32_t kSeqSlots = 1024u;        // kWalkPerSeq: sequences per block summed in LDS
constexpr uint64_t kMultiSeed = 0x90b45d39fb6da1faULL; // nthash.hpp:381-390
static_assert(kBlock % 256u == 0 && kBlock % 16u == 0 && kRun == 16u, "the block is 256 runs of 16 on the 16-byte grid");

enum { kWalkTotal = 0, kWalkPerSeq = 1, kWalkProfile = 2 };

// h % m without a division: a mask when m is a power of two, else floor(h / m) by one multiply-high with a 65-bit constant 2^64 + magic (the round-up
// method of Granlund & Montgomery as libdivide's branch-free u64 path states it), exact for every 64-bit h; the constants are computed once on the host
struct BloomMod {
	uint64_t m, magic;
	uint32_t shift, pow2;
};
inline BloomMod bloom_mod(uint64_t m)
{
	BloomMod d{m, 0, 0, (m & (m - 1)) == 0 ? 1u : 0u};
	if (d.pow2) return d;
	uint32_t L = 0;
	while ((m >> (L + 1)) != 0) ++L;
	uint64_t rem = 1ull << L, q = 0; // floor(2^(64 + L) / m) by long division: 2^L < m < 2^40, so neither rem nor q overflows
	for (int i = 0; i < 64; ++i) {
		rem <<= 1, q <<= 1;
		if (rem >= m) rem -= m, q |= 1;
	}
	q += q;
	if (rem + rem >= m) q += 1;
	d.magic = q + 1;
	d.shift = L;
	return d;
}
__device__ __forceinline__ uint64_t bloom_loc(const BloomMod& d, uint64_t h)
{
	if (d.pow2) return h & (d.m - 1);
	const uint64_t q = __umul64hi(d.magic, h);
	const uint64_t t = (((h - q) >> 1) + q) >> d.shift;
	return h - t * d.m;
}
// the dword of a plain filter and the bit in it (little-endian dwords over the reference's bytes: bit 7 - loc % 8 of byte loc / 8)
__host__ __device__ __forceinline__ uint32_t bloom_bit(uint64_t loc) { return 1u << (uint32_t)((loc & 24u) + 7u - (loc & 7u)); }
inline uint64_t filter_words(uint64_t m_bits) { return ((m_bits + 7u) / 8u + 3u) / 4u; }
__device__ __forceinline__ uint64_t bloom_multi(uint64_t h0, uint32_t i, uint64_t kmul)
{
	const uint64_t t = h0 * ((uint64_t)i ^ kmul);
	return t ^ (t >> 27);
}
// the n_hash positions of one value: what every action is built on
struct BloomHashes {
	BloomMod mod;
	uint32_t n_hash;
	uint64_t kmul; // k * multiSeed
	__device__ __forceinline__ uint64_t loc(uint64_t h0, uint32_t i) const { return bloom_loc(mod, i ? bloom_multi(h0, i, kmul) : h0); }
};
inline BloomHashes bloom_hashes(uint64_t m, uint32_t n_hash, uint32_t k) { return BloomHashes{bloom_mod(m), n_hash, (uint64_t)k * kMultiSeed}; }

__device__ __forceinline__ void bloom_set(uint32_t* filter, const BloomHashes& hs, uint64_t h0)
{
	for (uint32_t i = 0; i < hs.n_hash; ++i) {
		const uint64_t loc = hs.loc(h0, i);
		const uint32_t bit = bloom_bit(loc);
		uint32_t* w = filter + (loc >> 5);
		// A PLAIN load decides whether the atomic is needed.  No ordering is required: bits only go 0 -> 1 during a build, so a stale value can only
		// show a bit clear that is already set — a redundant atomic, never a lost one.
		if ((*w & bit) == 0) (void)__hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}
__device__ __forceinline__ bool bloom_test(const uint32_t* filter, const BloomHashes& hs, uint64_t h0)
{
	for (uint32_t i = 0; i < hs.n_hash; ++i) {
		const uint64_t loc = hs.loc(h0, i);
		if ((filter[loc >> 5] & bloom_bit(loc)) == 0) return false; // leave at the first clear bit
	}
	return true;
}
// The view of a plain filter.  A view has internal linkage, and with it every kernel instantiated over it: the kernel is its translation unit's own, and
// LDS that an instantiation only writes (block_total of a kWalkPerSeq walk) can be dropped from it.
namespace {
struct BitsView {
	uint32_t* filter;
	BloomHashes hs;
	__device__ __forceinline__ void insert(uint64_t h0) const { bloom_set(filter, hs, h0); }
	__device__ __forceinline__ bool test(uint64_t h0) const { return bloom_test(filter, hs, h0); }
	__device__ __forceinline__ unsigned char answer(uint64_t h0) const { return test(h0) ? 1 : 0; }
};
} // namespace
inline BitsView bits_view(const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k)
{
	return BitsView{static_cast<uint32_t*>(const_cast<void*>(d_filter)), bloom_hashes(m_bits, n_hash, k)};
}

// split rotate by one to the left / right (nthash.hpp:186-217): bits [0, 33) and [33, 64) rotate on their own
__device__ __forceinline__ uint64_t srol1(uint64_t x)
{
	return ((x << 1) & ~((1ull << 33) | 1ull)) | ((x >> 63) << 33) | ((x >> 32) & 1ull);
}
__device__ __forceinline__ uint64_t sror1(uint64_t x)
{
	return ((x >> 1) & ~(1ull << 32)) | ((x & 1ull) << 32) | (((x >> 33) & 1ull) << 63);
}

__device__ __forceinline__ uint32_t bloom_code(uint32_t b)
{
	const uint32_t x = b | 0x20u; // (b | 0x20 == 'a' only for 'A' and 'a', and so on)
	return x == 'a' ? 0u : x == 'c' ? 1u : x == 'g' ? 2u : (x == 't' || x == 'u') ? 3u : 4u;
}

struct BloomWalk {
	const uint4* src16;  // the 16-byte grid of the source: position p is byte lead + p behind it
	uint32_t lead;       // 0 .. 15
	uint32_t k, strand;
	uint64_t n;          // positions
	const uint64_t* off; // device copy of the offsets, n_seqs + 1
	uint64_t n_seqs;
	uint64_t in[5][2];   // per code of the incoming base: {seed, srol^k(comp)}; [4]: zeros
	uint64_t out[5][2];  // per code of the outgoing base: {srol^k(seed), comp}; [4] = no outgoing base: zeros
	unsigned long long* total; // kWalkTotal
	uint32_t* windows;   // kWalkPerSeq: per sequence
	uint32_t* hits;
	unsigned char* profile; // kWalkProfile: n bytes
};

// the first index in [lo, hi) whose offset is > v, or hi
__device__ __forceinline__ uint64_t bloom_upper(const uint64_t* off, uint64_t lo, uint64_t hi, uint64_t v)
{
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (off[mid] > v)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

// kWalkProfile: the lane's 16 bytes `r` (byte i: position j0 + i) to out[j0 .. min(j0 + 16, n))
__device__ __forceinline__ void bloom_store_run(unsigned char* out, uint64_t j0, uint64_t n, const uint32_t r[4])
{
	if (j0 >= n) return;
	unsigned char* p = out + j0;
	const uint32_t left = n - j0 < 16u ? (uint32_t)(n - j0) : 16u;
	const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
	if (left == 16u && (addr & 15u) == 0) {
		*reinterpret_cast<uint4*>(p) = make_uint4(r[0], r[1], r[2], r[3]);
		return;
	}
#pragma unroll
	for (uint32_t d = 0; d < 4; ++d) {
		if ((addr & 3u) == 0 && 4u * d + 4u <= left) {
			reinterpret_cast<uint32_t*>(p)[d] = r[d];
		} else {
#pragma unroll
			for (uint32_t t = 0; t < 4; ++t)
				if (4u * d + t < left) p[4u * d + t] = (unsigned char)(r[d] >> (8u * t));
		}
	}
}

template <class Act> __global__ __launch_bounds__(256) void bloom_walk_kernel(const BloomWalk a, const Act act)
{
	constexpr bool kPerSeq = Act::kMode == kWalkPerSeq, kProfile = Act::kMode == kWalkProfile;
	__shared__ uint4 stage16[kStageBytes / 16u];
	__shared__ uint64_t tab_in[5][2], tab_out[5][2];
	__shared__ uint32_t seq_w[kPerSeq ? kSeqSlots : 1u], seq_h[kPerSeq ? kSeqSlots : 1u];
	__shared__ uint32_t block_total;
	unsigned char* stage = reinterpret_cast<unsigned char*>(stage16);
	uint32_t* stage32 = reinterpret_cast<uint32_t*>(stage16);
	const uint32_t tid = threadIdx.x;
	const uint64_t jb = (uint64_t)blockIdx.x * kBlock; // the block's first window start
	const uint32_t span = kBlock + a.k - 1u;           // positions jb .. jb + span - 1 are staged: LDS bytes lead .. lead + span - 1

	if (tid == 0) { // (constant indices: the arguments stay in scalar registers)
#pragma unroll
		for (uint32_t c = 0; c < 5; ++c) {
			tab_in[c][0] = a.in[c][0], tab_in[c][1] = a.in[c][1];
			tab_out[c][0] = a.out[c][0], tab_out[c][1] = a.out[c][1];
		}
		block_total = 0;
	}
	if (kPerSeq)
		for (uint32_t s = tid; s < kSeqSlots; s += 256u)
			seq_w[s] = 0, seq_h[s] = 0;
	// stage: 16-byte piece c holds the positions jb + 16 c - lead .. + 15.  A piece is loaded iff it holds a position of [0, n): an aligned 16-byte piece
	// never crosses a page, so the bytes around the source's first and last in it are mapped; they are staged as "no base" and never read as anything else
	const uint32_t n_pieces = (a.lead + span + 15u) / 16u; // <= kStageBytes / 16
	for (uint32_t c = tid; c < n_pieces; c += 256u) {
		const int64_t p0 = (int64_t)(jb + 16u * c) - (int64_t)a.lead; // position of the piece's first byte
		const int64_t lo = p0 < 0 ? -p0 : 0, hi = (int64_t)a.n - p0;   // the piece's bytes [lo, hi) are positions of [0, n)
		uint4 v = make_uint4(0, 0, 0, 0);
		const bool any = lo < 16 && hi > 0;
		if (any) v = a.src16[(jb >> 4) + c];
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
		uint32_t o[4];
#pragma unroll
		for (uint32_t d = 0; d < 4; ++d) {
			uint32_t codes = 0;
#pragma unroll
			for (uint32_t t = 0; t < 4; ++t) {
				const int64_t i = 4 * d + t;
				const uint32_t cd = (any && i >= lo && i < hi) ? bloom_code((w[d] >> (8u * t)) & 0xffu) : 4u;
				codes |= cd << (8u * t);
			}
			o[d] = codes;
		}
		stage16[c] = make_uint4(o[0], o[1], o[2], o[3]);
	}
	// the sequences that start behind jb and inside the staged span (every lane runs the same search: the loads are broadcasts)
	const uint64_t off0 = a.off[0];
	const uint64_t s_lo = bloom_upper(a.off, 0, a.n_seqs + 1u, off0 + jb); // >= 1; sequence s_lo - 1 holds position jb
	const uint64_t last = jb + span < a.n ? jb + span : a.n;                 // positions < last are staged and inside the input
	__syncthreads();
	for (uint64_t i = s_lo + tid; i <= a.n_seqs; i += 256u) {
		const uint64_t p = a.off[i] - off0;
		if (p >= last) break;
		const uint32_t q = a.lead + (uint32_t)(p - jb);
		atomicOr(&stage32[q >> 2], 8u << (8u * (q & 3u)));
	}
	__syncthreads();

	// walk
	const uint64_t j0 = jb + (uint64_t)tid * kRun;
	uint32_t my_windows = 0, my_hits = 0;
	uint32_t prof[4] = {0, 0, 0, 0}; // kWalkProfile: byte i of the 16 = the window that starts at j0 + i
	uint64_t seq = 0, s_hi = 0;
	if (j0 + a.k <= a.n) { // (else no window of this lane lies inside the input)
		if (kPerSeq) {
			s_hi = bloom_upper(a.off, s_lo, a.n_seqs + 1u, off0 + last - 1u); // every search of this block ends in [s_lo, s_hi]
			seq = bloom_upper(a.off, s_lo, s_hi, off0 + j0) - 1u;
		}
		auto flush = [&]() {
			if (!kPerSeq || my_windows == 0) return;
			const uint64_t slot = seq - (s_lo - 1u);
			if (slot < kSeqSlots) {
				atomicAdd(&seq_w[slot], my_windows);
				if (my_hits) atomicAdd(&seq_h[slot], my_hits);
			} else {
				atomicAdd(&a.windows[seq], my_windows);
				if (my_hits) atomicAdd(&a.hits[seq], my_hits);
			}
			my_windows = my_hits = 0;
		};
		const uint32_t q0 = a.lead + tid * kRun;
		const uint32_t steps = kRun + a.k - 1u;
		uint32_t run = 0;
		uint64_t fh = 0, rh = 0;
		for (uint32_t s = 0; s < steps; ++s) {
			const uint32_t c = stage[q0 + s];
			if ((c & 8u) && s != 0) { // a sequence starts here (at s == 0 the lane starts fresh anyway)
				run = 0, fh = 0, rh = 0;
				if (kPerSeq) {
					flush();
					seq = bloom_upper(a.off, s_lo, s_hi, off0 + j0 + s) - 1u;
				}
			}
			const uint32_t in = c & 7u;
			if (in == 4u) {
				run = 0, fh = 0, rh = 0;
				continue;
			}
			const uint32_t out = run >= a.k ? stage[q0 + s - a.k] & 3u : 4u;
			fh = srol1(fh) ^ tab_in[in][0] ^ tab_out[out][0];
			rh = sror1(rh ^ tab_in[in][1] ^ tab_out[out][1]);
			++run;
			if (run >= a.k && s + 1u >= a.k) { // the window that ends here starts at j0 + s + 1 - k >= j0
				const uint64_t h0 = a.strand == 1u ? fh : a.strand == 2u ? rh : (rh < fh ? rh : fh);
				const uint32_t r = act(h0);
				if (kProfile) {
					const uint32_t i = s + 1u - a.k, sh = 8u * (i & 3u); // 0 .. 15
					prof[0] |= (i >> 2) == 0u ? r << sh : 0u;
					prof[1] |= (i >> 2) == 1u ? r << sh : 0u;
					prof[2] |= (i >> 2) == 2u ? r << sh : 0u;
					prof[3] |= (i >> 2) == 3u ? r << sh : 0u;
				} else if (kPerSeq) {
					++my_windows;
					my_hits += r;
				} else {
					my_windows += r;
				}
			}
		}
		flush();
	}
	if (kProfile) {
		bloom_store_run(a.profile, j0, a.n, prof);
	} else if (kPerSeq) {
		__syncthreads();
		for (uint32_t s = tid; s < kSeqSlots; s += 256u) {
			const uint32_t w = seq_w[s], h = seq_h[s];
			if (w) atomicAdd(&a.windows[s_lo - 1u + s], w); // (w != 0 only for a sequence that exists)
			if (h) atomicAdd(&a.hits[s_lo - 1u + s], h);
		}
	} else {
		if (my_windows) atomicAdd(&block_total, my_windows);
		__syncthreads();
		if (tid == 0 && block_total) atomicAdd(a.total, (unsigned long long)block_total);
	}
}

// the walk's actions of every kind: insert a window's value (1 per window), test it (1 per hit)
template <class View> struct InsertAct {
	static constexpr int kMode = kWalkTotal;
	View v;
	__device__ __forceinline__ uint32_t operator()(uint64_t h0) const
	{
		v.insert(h0);
		return 1u;
	}
};
template <class View> struct TestAct {
	static constexpr int kMode = kWalkPerSeq;
	View v;
	__device__ __forceinline__ uint32_t operator()(uint64_t h0) const { return v.test(h0) ? 1u : 0u; }
};

// the same over n given values h_0, without a walk
template <class View> __global__ __launch_bounds__(256) void insert_hashes_kernel(View v, const uint64_t* __restrict__ h0, uint64_t n)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		v.insert(h0[i]);
}
template <class View> __global__ __launch_bounds__(256) void query_hashes_kernel(View v, const uint64_t* __restrict__ h0, uint64_t n, unsigned char* __restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		out[i] = v.answer(h0[i]);
}

inline unsigned stride_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255u) / 256u, 256u * 16u); }

// one launch of a grid-stride kernel over n items on the caller's stream, waited for: what every entry point without a walk and without scratch is
template <class... Params, class... Args> int launch_strided(int32_t device, void* stream, void (*kernel)(Params...), uint64_t n, Args... args)
{
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	hipLaunchKernelGGL(kernel, dim3(stride_grid(n)), dim3(256), 0, st, args...);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

// The checks every filter call shares; `who` names the call, `what` the unit of m ("m_bits" of a plain filter, "m" counters of a counting one).  A kind
// whose m is a multiple of a block (ntc_bbloom.hpp) passes the block's bits as `block`: the rule for m and its wording follow from it.
inline int check_filter(const char* who, const void* d_filter, uint64_t m, uint32_t n_hash, uint32_t k, const char* what = "m_bits", const char* array = "filter",
                        uint32_t block = 0)
{
	if (!d_filter) return fail(NTC_ERR_ARG, "%s: null %s", who, array);
	if ((uintptr_t)d_filter & 3u) return fail(NTC_ERR_ARG, "%s: the %s is not 4-byte aligned", who, array);
	if (block && (m < block || m >= (1ull << 40) || m % block != 0))
		return fail(NTC_ERR_ARG, "%s: %s=%llu is no multiple of %u in %u..2^40-%u", who, what, (unsigned long long)m, block, block, block);
	if (m < 1 || m >= (1ull << 40)) return fail(NTC_ERR_ARG, "%s: %s=%llu outside 1..2^40-1", who, what, (unsigned long long)m);
	if (n_hash < 1 || n_hash > 32) return fail(NTC_ERR_ARG, "%s: n_hash=%u outside 1..32", who, n_hash);
	if (k < 1 || k > kMaxK) return fail(NTC_ERR_ARG, "%s: k=%u outside 1..%u", who, k, kMaxK);
	return 0;
}

// n given values h_0 and, for a query, the array their answers go to (`out_ok`: it is there; `what` names the pair in the message)
inline int check_hashes(const char* who, const void* d_h0_u64, uint64_t n, const char* what = "hashes", bool out_ok = true)
{
	if (n && (!d_h0_u64 || !out_ok)) return fail(NTC_ERR_ARG, "%s: null %s", who, what);
	if ((uintptr_t)d_h0_u64 & 7u) return fail(NTC_ERR_ARG, "%s: the hashes are not 8-byte aligned", who);
	return 0;
}

inline int check_input(const char* who, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs)
{
	if (strand > 2) return fail(NTC_ERR_ARG, "%s: strand %u is none of 0 (canonical), 1 (forward), 2 (reverse)", who, strand);
	if (!offsets) return fail(NTC_ERR_ARG, "%s: null offsets", who);
	for (uint64_t i = 0; i < n_seqs; ++i)
		if (offsets[i + 1] < offsets[i]) return fail(NTC_ERR_ARG, "%s: offsets not monotone at sequence %llu", who, (unsigned long long)i);
	const uint64_t n = offsets[n_seqs] - offsets[0];
	if (n && !d_bases) return fail(NTC_ERR_ARG, "%s: null bases", who);
	if (n > (1ull << 43)) return fail(NTC_ERR_ARG, "%s: %llu bytes in one call (at most 2^43)", who, (unsigned long long)n);
	return 0;
}

// What the three shapes below share: the offsets go up into `d_off`, the walk's arguments are filled in beside the outputs the caller has set in `a`
// (all else zero), one launch over `blocks` blocks of window starts, checked.
template <class Act>
int walk_launch(hipStream_t st, BloomWalk a, const Act& act, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t* d_off,
                uint64_t blocks)
{
	HIP_TRY(hipMemcpyAsync(d_off, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
	const uintptr_t first = reinterpret_cast<uintptr_t>(d_bases) + offsets[0];
	a.src16 = reinterpret_cast<const uint4*>(first & ~(uintptr_t)15);
	a.lead = (uint32_t)(first & 15u);
	a.k = k, a.strand = strand;
	a.n = offsets[n_seqs] - offsets[0];
	a.off = d_off;
	a.n_seqs = n_seqs;
	for (unsigned c = 0; c < 4; ++c) {
		a.in[c][0] = ntc::seed_of(c);
		a.in[c][1] = ntc::srol(ntc::comp_of(c), k);
		a.out[c][0] = ntc::srol(ntc::seed_of(c), k);
		a.out[c][1] = ntc::comp_of(c);
	}
	hipLaunchKernelGGL(bloom_walk_kernel<Act>, dim3((unsigned)blocks), dim3(256), 0, st, a, act); // (n <= 2^43: blocks is below 2^31)
	HIP_TRY(hipGetLastError());
	return 0;
}

// The three shapes a walking entry point has.  walk_total: one launch over the blocks of window starts, *total comes back (the call is synchronous).
// walk_per_seq: the two per-sequence arrays are zeroed and filled.  walk_profile: one byte per position.  `who` names the call in messages.
template <class Act>
int walk_total(const char* who, int32_t device, void* stream, const Act& act, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs,
               uint64_t* total_out)
{
	static_assert(Act::kMode == kWalkTotal, "an action that sums into one total");
	const uint64_t n = offsets[n_seqs] - offsets[0];
	if (n < k) { // no window: no device
		if (total_out) *total_out = 0;
		return 0;
	}
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	ntc_eng::DevBuf<uint64_t> d_off; // (scratch of this call: freed on every way out)
	ntc_eng::DevBuf<unsigned long long> d_total;
	if (!d_off.reserve((n_seqs + 1) * 8) || !d_total.reserve(8))
		return fail(NTC_ERR_MEMORY, "%s: cannot allocate %llu B of scratch on device", who, (unsigned long long)((n_seqs + 1) * 8 + 8));
	HIP_TRY(hipMemsetAsync(d_total, 0, 8, st));
	BloomWalk a{};
	a.total = d_total;
	if (int rc = walk_launch(st, a, act, k, strand, d_bases, offsets, n_seqs, d_off, (n - k + 1 + kBlock - 1) / kBlock)) return rc;
	unsigned long long total = 0;
	HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (total_out) *total_out = total;
	return 0;
}

template <class Act>
int walk_per_seq(const char* who, int32_t device, void* stream, const Act& act, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs,
                 void* d_windows_u32, void* d_hits_u32)
{
	static_assert(Act::kMode == kWalkPerSeq, "an action that sums per sequence");
	if (n_seqs && (!d_windows_u32 || !d_hits_u32)) return fail(NTC_ERR_ARG, "%s: null output", who);
	if (n_seqs == 0) return 0;
	const uint64_t n = offsets[n_seqs] - offsets[0];
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	ntc_eng::DevBuf<uint64_t> d_off; // (scratch of this call: freed on every way out)
	if (n >= k && !d_off.reserve((n_seqs + 1) * 8)) return fail(NTC_ERR_MEMORY, "%s: cannot allocate %llu B of scratch on device", who, (unsigned long long)((n_seqs + 1) * 8));
	HIP_TRY(hipMemsetAsync(d_windows_u32, 0, n_seqs * 4, st));
	HIP_TRY(hipMemsetAsync(d_hits_u32, 0, n_seqs * 4, st));
	if (n >= k) {
		BloomWalk a{};
		a.windows = static_cast<uint32_t*>(d_windows_u32);
		a.hits = static_cast<uint32_t*>(d_hits_u32);
		if (int rc = walk_launch(st, a, act, k, strand, d_bases, offsets, n_seqs, d_off, (n - k + 1 + kBlock - 1) / kBlock)) return rc;
	}
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

template <class Act>
int walk_profile(const char* who, int32_t device, void* stream, const Act& act, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs,
                 void* d_profile_u8)
{
	static_assert(Act::kMode == kWalkProfile, "an action that gives the byte of a window's start");
	const uint64_t n = offsets[n_seqs] - offsets[0];
	if (n && !d_profile_u8) return fail(NTC_ERR_ARG, "%s: null output", who);
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	ntc_eng::DevBuf<uint64_t> d_off; // (scratch of this call: freed on every way out)
	if (!d_off.reserve((n_seqs + 1) * 8)) return fail(NTC_ERR_MEMORY, "%s: cannot allocate %llu B of scratch on device", who, (unsigned long long)((n_seqs + 1) * 8));
	BloomWalk a{};
	a.profile = static_cast<unsigned char*>(d_profile_u8);
	// every POSITION has a lane, not only every window start: the last k - 1 positions, and all of an input shorter than k, get their zeros from the kernel
	if (int rc = walk_launch(st, a, act, k, strand, d_bases, offsets, n_seqs, d_off, (n + kBlock - 1) / kBlock)) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

} // namespace ntc_bloom
