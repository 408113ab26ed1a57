// ntc_sig_algebra.hip — set algebra and the abundance spectrum of signatures, on the device: union (counts added), select (intersect, subtract, abundance
// filter) and hist (include/ntcard_hip.h: ntc_signature_union_device, ntc_signature_select_device, ntc_signature_hist_device; DESIGN.md §4 "Signatures",
// "Set algebra and spectrum").  All of them are linear passes over lists that are sorted and on the device already.
//
//   compaction  the primitive under union and select: a byte of flag per entry says whether the entry stays; the kept entries go to the output in their order.
//            count    a workgroup per TILE of 2048 entries (at most kCompactBlocks of them, the rest in a grid-stride loop): the set flags of the tile
//            scan     ONE workgroup walks the tile counts 256 tiles per turn: every tile's first output position, and the total
//            scatter  a workgroup per tile again; wave w takes the entries [512 w, 512 w + 512) of the tile in 8 rounds of 64, so the order of the entries is
//                     (tile, wave, round, lane) and a kept entry's rank = the tile's base + the kept entries of the waves below + those of the wave's earlier
//                     rounds + lanes_below(ballot)
//            The host waits once in front of the scatter — the total and the lists' bad entries come home in one copy — and once at the end.
//   union    gather   every list into one pair buffer, list after list (blockIdx.y = the list; a list without counts gives 1 each)
//            sort     sig_sort() (ntc_sig_sort.hip; it waits once for its digit histograms above 4096 pairs)
//            heads    flag[i] = the pair's key differs from the one before it
//            compaction, whose scatter lets every run head add up its run: at most n_lists pairs, because every list ascends strictly
//   select   flags    a lane per entry of A: the count test, then list_lower_bound in reference after reference until one decides
//            compaction
//   hist     one launch: LDS bins for the counts below kHistLdsBins, global atomics for the rest and for the flush; the lanes of a wave that hold the first
//            lane's count send one add (hist_add)
// No kernel waits on another workgroup; a launch reads what an earlier launch of the stream wrote.  Vector stores and plain C++ only.
#include "ntc_sig_device.hpp"

namespace ntc {

namespace {

constexpr uint32_t kCompactTile = 2048;                         // entries per workgroup and turn
constexpr uint32_t kCompactRounds = kCompactTile / 256u;        // 8 of them per lane
constexpr uint32_t kCompactWaveItems = 64u * kCompactRounds;    // 512 per wave
constexpr uint32_t kCompactBlocks = 512;     // grid cap of compact_count_kernel and compact_scatter_kernel (tiles per turn)
constexpr uint32_t kCompactScanTiles = 256;  // tiles per turn of compact_scan_kernel
constexpr uint32_t kUnionGatherBlocks = 1024; // grid cap of union_gather_kernel (per list)
constexpr uint32_t kUnionHeadBlocks = 1024;  // ... of union_head_kernel
constexpr uint32_t kSelectBlocks = 3072;     // ... of select_flag_kernel (its lanes wait on dependent loads: more workgroups than the streaming kernels get)
constexpr uint32_t kHistBlocks = 1024;       // ... of sig_hist_kernel
constexpr uint32_t kHistLdsBins = 1024;      // the counts 0 .. 1023 are binned in LDS (the default spectrum, -c 1000, is LDS-resident)
constexpr uint32_t kAlgebraMaxLists = 1024;
static_assert(kCompactTile == 256u * kCompactRounds && kCompactRounds <= 32u, "a lane and round = one entry, a bit of `keep` each");

__global__ __launch_bounds__(256) void compact_count_kernel(const unsigned char* __restrict__ flags, uint64_t n, uint32_t* __restrict__ tile_count, uint64_t tiles)
{
	__shared__ uint32_t wsum[4];
	for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const uint64_t base = t * kCompactTile + threadIdx.x;
		uint32_t c = 0;
#pragma unroll
		for (uint32_t r = 0; r < kCompactRounds; ++r) {
			const uint64_t i = base + r * 256u;
			c += i < n ? flags[i] : 0u;
		}
		c = (uint32_t)wave_sum(c);
		if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = c;
		__syncthreads();
		if (threadIdx.x == 0u) tile_count[t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
		__syncthreads();
	}
}

// one workgroup: the tile counts become their exclusive prefix sums (fewer than 2^32 entries in all: 32-bit positions), *total = the sum
__global__ __launch_bounds__(256) void compact_scan_kernel(uint32_t* __restrict__ tile_count, uint64_t tiles, unsigned long long* __restrict__ total)
{
	__shared__ uint32_t wsum[4];
	uint32_t carry = 0, sum = 0;
	for (uint64_t t0 = 0; t0 < tiles; t0 += kCompactScanTiles) {
		const uint64_t t = t0 + threadIdx.x;
		const uint32_t v = t < tiles ? tile_count[t] : 0u;
		const uint32_t ex = block_scan(v, wsum, sum);
		if (t < tiles) tile_count[t] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0u) *total = carry;
}
static_assert(kCompactScanTiles == 256u, "a thread per tile of a turn");

// the flagged entries of (keys, vals) go to (out_keys, out_vals) in their order; tile_base: what compact_scan_kernel left; room: the entries the output holds
// (>= the total the scan found, so no rank reaches it: the flags are this call's own scratch).  vals == nullptr: 1 each; out_vals == nullptr: keys only.
// kRuns (union): a flagged entry is the head of a run of equal keys and takes the run's values, added up and saturating at 2^32 - 1
template <bool kRuns>
__global__ __launch_bounds__(256) void compact_scatter_kernel(const unsigned char* __restrict__ flags, uint64_t n, const uint32_t* __restrict__ tile_base, uint64_t tiles,
                                                              const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                              unsigned long long* __restrict__ out_keys, uint32_t* __restrict__ out_vals, uint64_t room)
{
	__shared__ uint32_t wcount[4];
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const uint64_t first = t * kCompactTile + (uint64_t)wave * kCompactWaveItems + lane;
		uint32_t keep = 0; // bit r: the lane's entry of round r stays
#pragma unroll
		for (uint32_t r = 0; r < kCompactRounds; ++r) {
			const uint64_t i = first + r * 64u;
			if (i < n && flags[i]) keep |= 1u << r;
		}
		const uint32_t c = (uint32_t)wave_sum((unsigned long long)__popc(keep));
		if (lane == 0u) wcount[wave] = c;
		__syncthreads();
		uint64_t at = tile_base[t];
#pragma unroll
		for (uint32_t w = 0; w < 4u; ++w)
			at += w < wave ? wcount[w] : 0u;
#pragma unroll
		for (uint32_t r = 0; r < kCompactRounds; ++r) {
			const bool mine = ((keep >> r) & 1u) != 0u;
			const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
			const uint64_t rank = at + lanes_below(m);
			if (mine && rank < room) {
				const uint64_t i = first + r * 64u;
				const unsigned long long k = keys[i];
				out_keys[rank] = k;
				if (out_vals) {
					unsigned long long sum = vals ? vals[i] : 1u;
					if (kRuns)
						for (uint64_t j = i + 1; j < n && keys[j] == k; ++j)
							sum += vals[j];
					out_vals[rank] = sum < 0xffffffffull ? (uint32_t)sum : 0xffffffffu;
				}
			}
			at += (uint64_t)__popcll(m);
		}
		__syncthreads(); // (wcount is the next turn's)
	}
}

// blockIdx.y = the list: its entries go to keys_out[base[list] ..], their counts (counts[list] == 0: 1 each) to vals_out (nullptr: none).  counts[] holds
// device addresses as words
__global__ __launch_bounds__(256) void union_gather_kernel(const unsigned long long* const* __restrict__ lists, const uint64_t* __restrict__ ns,
                                                           const unsigned long long* __restrict__ counts, const unsigned long long* __restrict__ base,
                                                           unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ vals_out)
{
	const uint32_t li = blockIdx.y;
	const unsigned long long* a = lists[li];
	const uint32_t* c = (const uint32_t*)(uintptr_t)counts[li];
	const uint64_t n = ns[li], o = base[li];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		keys_out[o + i] = a[i];
		if (vals_out) vals_out[o + i] = c ? c[i] : 1u;
	}
}

// flags[i] = keys[i] starts a run of equal keys
__global__ __launch_bounds__(256) void union_head_kernel(const unsigned long long* __restrict__ keys, uint64_t n, unsigned char* __restrict__ flags)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		flags[i] = (i == 0 || keys[i - 1] != keys[i]) ? 1 : 0;
}

// lists[n_refs] is A.  flags[i] = A's entry i passes the count test (ca == nullptr: its count is 1) and the membership rule of `mode` over the references; a
// lane leaves the references at the first one that decides: one that lacks the entry under IN_ALL, one that holds it under IN_NONE and IN_ANY.  A search stays
// inside its list whatever the list holds, so a list that fails the ascent check costs a wrong flag at most, and the host throws the flags away
__global__ __launch_bounds__(256) void select_flag_kernel(const unsigned long long* const* __restrict__ lists, const uint64_t* __restrict__ ns, uint32_t n_refs,
                                                          const uint32_t* __restrict__ ca, uint32_t mode, uint32_t min_count, uint32_t max_count,
                                                          unsigned char* __restrict__ flags)
{
	const unsigned long long* a = lists[n_refs];
	const uint64_t na = ns[n_refs];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < na; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t c = ca ? ca[i] : 1u;
		bool keep = c >= min_count && (max_count == 0u || c <= max_count);
		if (keep) {
			const unsigned long long x = a[i];
			bool decided = false;
			for (uint32_t r = 0; r < n_refs && !decided; ++r) {
				const unsigned long long* l = lists[r];
				const uint64_t nl = ns[r];
				const uint64_t at = list_lower_bound(l, nl, x);
				const bool found = at < nl && l[at] == x;
				decided = mode == NTC_SIG_IN_ALL ? !found : found;
			}
			keep = mode == NTC_SIG_IN_ANY ? decided : !decided;
		}
		flags[i] = keep ? 1 : 0;
	}
}

// hist[min(v, cov_max + 1)] += 1 for every count v, hist[cov_max + 2] += the counts.  A workgroup's LDS bins are 32-bit: it sees n / gridDim.x entries, fewer
// than 2^32 for every n a device can hold
__global__ __launch_bounds__(256) void sig_hist_kernel(const uint32_t* __restrict__ counts, uint64_t n, uint32_t cov_max, unsigned long long* __restrict__ hist)
{
	__shared__ uint32_t h[kHistLdsBins];
	for (uint32_t b = threadIdx.x; b < kHistLdsBins; b += 256u)
		h[b] = 0u;
	__syncthreads();
	const uint64_t step = (uint64_t)gridDim.x * 256u;
	const uint64_t rounds = (n + step - 1) / step; // every wave runs the same number of rounds: hist_add sees whole waves
	unsigned long long weight = 0;
	for (uint64_t r = 0, i = (uint64_t)blockIdx.x * 256u + threadIdx.x; r < rounds; ++r, i += step) {
		const bool valid = i < n;
		const uint32_t v = valid ? counts[i] : 0u;
		const bool low = v < kHistLdsBins;
		weight += v;
		hist_add(h, low ? v : 0u, valid && low);
		if (valid && !low) atomicAdd(hist + (v <= cov_max ? v : cov_max + 1u), 1ull);
	}
	__syncthreads();
	for (uint32_t b = threadIdx.x; b < kHistLdsBins; b += 256u)
		if (h[b]) atomicAdd(hist + (b <= cov_max ? b : cov_max + 1u), (unsigned long long)h[b]);
	weight = wave_sum(weight);
	if ((threadIdx.x & 63u) == 0u && weight) atomicAdd(hist + cov_max + 2u, weight);
}

// The flags of n entries and the tile counts under them: the scratch of one compaction, 1 B per entry and 4 B per tile
struct Compaction {
	ntc_eng::DevBuf<unsigned char> flags;
	ntc_eng::DevBuf<uint32_t> tile_count;
	uint64_t n = 0, tiles = 0;
	static size_t bytes(uint64_t n) { return (size_t)std::max<uint64_t>(n, 1) + (size_t)std::max<uint64_t>((n + kCompactTile - 1) / kCompactTile, 1) * 4; }
	bool reserve(uint64_t entries)
	{
		n = entries, tiles = (n + kCompactTile - 1) / kCompactTile;
		return flags.reserve((size_t)std::max<uint64_t>(n, 1)) && tile_count.reserve((size_t)std::max<uint64_t>(tiles, 1) * 4);
	}
	unsigned grid() const { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, kCompactBlocks)); }
	// count and scan: *d_total = the flagged entries
	hipError_t rank(unsigned long long* d_total, hipStream_t st)
	{
		hipLaunchKernelGGL(compact_count_kernel, dim3(grid()), dim3(256), 0, st, (const unsigned char*)flags.get(), n, tile_count.get(), tiles);
		hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(256), 0, st, tile_count.get(), tiles, d_total);
		return hipGetLastError();
	}
	template <bool kRuns>
	hipError_t scatter(const unsigned long long* keys, const uint32_t* vals, void* out_keys, void* out_vals, uint64_t room, hipStream_t st)
	{
		if (tiles == 0) return hipSuccess;
		hipLaunchKernelGGL(compact_scatter_kernel<kRuns>, dim3(grid()), dim3(256), 0, st, (const unsigned char*)flags.get(), n, (const uint32_t*)tile_count.get(), tiles, keys,
		                   vals, (unsigned long long*)out_keys, (uint32_t*)out_vals, room);
		return hipGetLastError();
	}
};

// do the `an` values of `a_bytes` bytes at a and the `bn` values of `b_bytes` bytes at b share a byte?
bool overlap(const void* a, uint64_t an, uint64_t a_bytes, const void* b, uint64_t bn, uint64_t b_bytes)
{
	if (!a || !b || !an || !bn) return false;
	const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
	return ua < ub + bn * b_bytes && ub < ua + an * a_bytes;
}

// the part of the output protocol both calls decide before the device is touched (nullptr: the arguments are fine)
const char* bad_output(const void* d_out, const void* d_out_counts, uint64_t cap, const uint64_t* n_out)
{
	if (!n_out) return "n_out is null";
	if (!d_out && (cap || d_out_counts)) return "a null hash output asks for the size alone: cap must be 0 and the count output null";
	return nullptr;
}

} // namespace

} // namespace ntc

using namespace ntc_eng;

extern "C" {

int ntc_signature_union_device(int32_t device, void* stream, uint32_t n_lists, const void* const* d_hashes_u64, const void* const* d_counts_u32, const uint64_t* n,
                               void* d_out_u64, void* d_out_counts_u32, uint64_t cap, uint64_t* n_out)
{
	using namespace ntc;
	if (const char* why = bad_output(d_out_u64, d_out_counts_u32, cap, n_out)) return fail(NTC_ERR_ARG, "ntc_signature_union_device: %s", why);
	if (n_lists < 1 || n_lists > kAlgebraMaxLists) return fail(NTC_ERR_ARG, "ntc_signature_union_device: %u lists (1 .. 1024 are taken)", n_lists);
	if (!d_hashes_u64 || !n) return fail(NTC_ERR_ARG, "ntc_signature_union_device: null argument");
	uint64_t total = 0;
	for (uint32_t i = 0; i < n_lists; ++i) {
		if (n[i] >> 32) return fail(NTC_ERR_ARG, "ntc_signature_union_device: list %u has %llu entries (fewer than 2^32 are taken)", i, (unsigned long long)n[i]);
		if (!d_hashes_u64[i] && n[i]) return fail(NTC_ERR_ARG, "ntc_signature_union_device: list %u is null and has %llu entries", i, (unsigned long long)n[i]);
		total += n[i];
	}
	if (total >> 32) return fail(NTC_ERR_ARG, "ntc_signature_union_device: the lists have %llu entries in all (fewer than 2^32 are taken)", (unsigned long long)total);
	for (uint32_t i = 0; i < n_lists; ++i) {
		const void* c = d_counts_u32 ? d_counts_u32[i] : nullptr;
		if (overlap(d_out_u64, cap, 8, d_hashes_u64[i], n[i], 8) || overlap(d_out_u64, cap, 8, c, n[i], 4) || overlap(d_out_counts_u32, cap, 4, d_hashes_u64[i], n[i], 8) ||
		    overlap(d_out_counts_u32, cap, 4, c, n[i], 4))
			return fail(NTC_ERR_ARG, "ntc_signature_union_device: an output array overlaps list %u", i);
	}
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const size_t nl = n_lists;
	const bool one = n_lists == 1; // a checked copy: nothing to sort, no run longer than one pair
	// the lists' extra words (8 B each): [kept 1][count arrays nl][base nl]
	const size_t x_total = 0, x_counts = 1, x_base = x_counts + nl, n_extra = x_base + nl;
	SigLists lists;
	Compaction comp;
	DevBuf<unsigned long long> d_keys, d_alt_k;
	DevBuf<uint32_t> d_vals, d_alt_v;
	DevBuf<unsigned char> d_aux;
	const bool two = total > sig_sort_one_launch();
	const size_t pair_bytes = one ? 0 : (size_t)std::max<uint64_t>(total, 1) * 12 * (two ? 2 : 1) + sig_sort_aux_bytes(total);
	if (!lists.reserve(nl, n_extra, n_extra) ||
	    (!one && (!comp.reserve(total) || !d_keys.reserve((size_t)std::max<uint64_t>(total, 1) * 8) || !d_vals.reserve((size_t)std::max<uint64_t>(total, 1) * 4) ||
	              (two && (!d_alt_k.reserve(total * 8) || !d_alt_v.reserve(total * 4) || !d_aux.reserve(sig_sort_aux_bytes(total))))))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_union_device: cannot allocate %zu B of scratch on device; nothing was written",
		            lists.bytes() + pair_bytes + (one ? 0 : Compaction::bytes(total)));
	}
	unsigned long long* const x = lists.extra();
	uint64_t longest = 0, at = 0;
	for (size_t i = 0; i < nl; ++i) {
		lists.set(i, d_hashes_u64[i], n[i]);
		x[x_counts + i] = (unsigned long long)(uintptr_t)(d_counts_u32 ? d_counts_u32[i] : nullptr);
		x[x_base + i] = at;
		at += n[i];
		longest = std::max(longest, n[i]);
	}
	HIP_TRY(lists.start(st));
	const dim3 gather_grid(capped_grid(longest, kUnionGatherBlocks), n_lists);
	if (one) {
		HIP_TRY(lists.read_back(st));
		HIP_TRY(hipStreamSynchronize(st));
		if (lists.bad(0) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_union_device: list 0 is not strictly ascending at entry %llu", lists.bad(0));
		if (d_out_u64 && cap < total)
			return fail(NTC_ERR_ARG, "ntc_signature_union_device: the union has %llu entries and the output room for %llu", (unsigned long long)total, (unsigned long long)cap);
		if (d_out_u64 && total) {
			hipLaunchKernelGGL(union_gather_kernel, gather_grid, dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), lists.d_extra() + x_counts, lists.d_extra() + x_base,
			                   (unsigned long long*)d_out_u64, (uint32_t*)d_out_counts_u32);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(st));
		}
		*n_out = total;
		return 0;
	}
	if (total)
		hipLaunchKernelGGL(union_gather_kernel, gather_grid, dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), lists.d_extra() + x_counts, lists.d_extra() + x_base, d_keys.get(),
		                   d_vals.get());
	HIP_TRY(hipGetLastError());
	bool in_alt = false;
	HIP_TRY(sig_sort(d_keys, d_vals, d_alt_k, d_alt_v, total, d_aux.get(), st, &in_alt)); // (an unsorted list is sorted like any other; its result is thrown away below)
	const unsigned long long* keys = in_alt ? d_alt_k.get() : d_keys.get();
	const uint32_t* vals = in_alt ? d_alt_v.get() : d_vals.get();
	if (total) hipLaunchKernelGGL(union_head_kernel, dim3(capped_grid(total, kUnionHeadBlocks)), dim3(256), 0, st, keys, total, comp.flags.get());
	HIP_TRY(comp.rank(lists.d_extra() + x_total, st));
	HIP_TRY(lists.read_back(st, 1));
	HIP_TRY(hipStreamSynchronize(st)); // the wait in front of the scatter: every list is checked, the size of the union is known
	for (size_t i = 0; i < nl; ++i)
		if (lists.bad(i) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_union_device: list %zu is not strictly ascending at entry %llu", i, lists.bad(i));
	const uint64_t kept = x[x_total];
	if (d_out_u64 && cap < kept)
		return fail(NTC_ERR_ARG, "ntc_signature_union_device: the union has %llu entries and the output room for %llu", (unsigned long long)kept, (unsigned long long)cap);
	if (d_out_u64 && kept) {
		HIP_TRY(comp.scatter<true>(keys, vals, d_out_u64, d_out_counts_u32, cap, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	*n_out = kept;
	return 0;
}

int ntc_signature_select_device(int32_t device, void* stream, const void* d_a_u64, const void* d_ca_u32, uint64_t na, uint32_t n_refs, const void* const* d_refs_u64,
                                const uint64_t* n, uint32_t mode, uint32_t min_count, uint32_t max_count, void* d_out_u64, void* d_out_counts_u32, uint64_t cap,
                                uint64_t* n_out)
{
	using namespace ntc;
	if (const char* why = bad_output(d_out_u64, d_out_counts_u32, cap, n_out)) return fail(NTC_ERR_ARG, "ntc_signature_select_device: %s", why);
	if (n_refs > kAlgebraMaxLists) return fail(NTC_ERR_ARG, "ntc_signature_select_device: %u references (0 .. 1024 are taken)", n_refs);
	if (n_refs && (!d_refs_u64 || !n)) return fail(NTC_ERR_ARG, "ntc_signature_select_device: null argument");
	if (mode > NTC_SIG_IN_ANY) return fail(NTC_ERR_ARG, "ntc_signature_select_device: mode %u (NTC_SIG_IN_ALL, _NONE and _ANY are taken)", mode);
	if (max_count != 0 && min_count > max_count) return fail(NTC_ERR_ARG, "ntc_signature_select_device: min_count %u is above max_count %u", min_count, max_count);
	if (na >> 32) return fail(NTC_ERR_ARG, "ntc_signature_select_device: A has %llu entries (fewer than 2^32 are taken)", (unsigned long long)na);
	if (!d_a_u64 && na) return fail(NTC_ERR_ARG, "ntc_signature_select_device: A is null and has %llu entries", (unsigned long long)na);
	for (uint32_t i = 0; i < n_refs; ++i) {
		if (n[i] >> 32) return fail(NTC_ERR_ARG, "ntc_signature_select_device: reference %u has %llu entries (fewer than 2^32 are taken)", i, (unsigned long long)n[i]);
		if (!d_refs_u64[i] && n[i]) return fail(NTC_ERR_ARG, "ntc_signature_select_device: reference %u is null and has %llu entries", i, (unsigned long long)n[i]);
	}
	if (overlap(d_out_u64, cap, 8, d_a_u64, na, 8) || overlap(d_out_u64, cap, 8, d_ca_u32, na, 4) || overlap(d_out_counts_u32, cap, 4, d_a_u64, na, 8) ||
	    overlap(d_out_counts_u32, cap, 4, d_ca_u32, na, 4))
		return fail(NTC_ERR_ARG, "ntc_signature_select_device: an output array overlaps A");
	for (uint32_t i = 0; i < n_refs; ++i)
		if (overlap(d_out_u64, cap, 8, d_refs_u64[i], n[i], 8) || overlap(d_out_counts_u32, cap, 4, d_refs_u64[i], n[i], 8))
			return fail(NTC_ERR_ARG, "ntc_signature_select_device: an output array overlaps reference %u", i);
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const size_t nr = n_refs, nl = nr + 1; // the lists: the references, then A
	SigLists lists;                        // one extra word: the kept entries
	Compaction comp;
	if (!lists.reserve(nl, 1, 1) || !comp.reserve(na)) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_select_device: cannot allocate %zu B of scratch on device; nothing was written", lists.bytes() + Compaction::bytes(na));
	}
	for (size_t i = 0; i < nr; ++i)
		lists.set(i, d_refs_u64[i], n[i]);
	lists.set(nr, d_a_u64, na);
	HIP_TRY(lists.start(st));
	if (na)
		hipLaunchKernelGGL(select_flag_kernel, dim3(capped_grid(na, kSelectBlocks)), dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), n_refs, (const uint32_t*)d_ca_u32, mode,
		                   min_count, max_count, comp.flags.get());
	HIP_TRY(comp.rank(lists.d_extra(), st));
	HIP_TRY(lists.read_back(st, 1));
	HIP_TRY(hipStreamSynchronize(st)); // the wait in front of the scatter: every list is checked, the size of the result is known
	if (lists.bad(nr) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_select_device: A is not strictly ascending at entry %llu", lists.bad(nr));
	for (size_t i = 0; i < nr; ++i)
		if (lists.bad(i) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_select_device: reference %zu is not strictly ascending at entry %llu", i, lists.bad(i));
	const uint64_t kept = lists.extra()[0];
	if (d_out_u64 && cap < kept)
		return fail(NTC_ERR_ARG, "ntc_signature_select_device: the result has %llu entries and the output room for %llu", (unsigned long long)kept, (unsigned long long)cap);
	if (d_out_u64 && kept) {
		HIP_TRY(comp.scatter<false>((const unsigned long long*)d_a_u64, (const uint32_t*)d_ca_u32, d_out_u64, d_out_counts_u32, cap, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	*n_out = kept;
	return 0;
}

int ntc_signature_hist_device(int32_t device, void* stream, const void* d_counts_u32, uint64_t n, uint32_t cov_max, uint64_t* hist_out, uint64_t* weight_out)
{
	using namespace ntc;
	if (!hist_out) return fail(NTC_ERR_ARG, "ntc_signature_hist_device: hist_out is null");
	if (cov_max < 1 || cov_max > 65535) return fail(NTC_ERR_ARG, "ntc_signature_hist_device: cov_max %u (1 .. 65535 are taken)", cov_max);
	if (!d_counts_u32 && n) return fail(NTC_ERR_ARG, "ntc_signature_hist_device: the count array is null and has %llu entries", (unsigned long long)n);
	const size_t words = (size_t)cov_max + 3; // the bins, the overflow bin, the weight
	std::vector<unsigned long long> h(words, 0ull);
	if (n) {
		HIP_TRY(hipSetDevice(device));
		hipStream_t st = (hipStream_t)stream;
		DevBuf<unsigned long long> d_h;
		if (!d_h.reserve(words * 8)) {
			(void)hipGetLastError();
			return fail(NTC_ERR_MEMORY, "ntc_signature_hist_device: cannot allocate %zu B of scratch on device; nothing was written", words * 8);
		}
		HIP_TRY(hipMemsetAsync(d_h, 0, words * 8, st));
		hipLaunchKernelGGL(sig_hist_kernel, dim3(capped_grid(n, kHistBlocks)), dim3(256), 0, st, (const uint32_t*)d_counts_u32, n, cov_max, d_h.get());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(h.data(), d_h, words * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	std::copy(h.begin(), h.begin() + cov_max + 2, hist_out);
	if (weight_out) *weight_out = h[cov_max + 2];
	return 0;
}

} // extern "C"
