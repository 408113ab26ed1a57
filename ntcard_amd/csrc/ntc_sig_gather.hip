// ntc_sig_gather.hip — gather: the greedy decomposition of a query signature over up to 1024 reference signatures, on the device
// (include/ntcard_hip.h: ntc_signature_gather_device; DESIGN.md §4 "Signatures", "Gather").
//
// Every round picks the reference that holds the most query entries no earlier pick has taken (the lowest index among equals), reports it and takes its
// entries out.  All results are integer sums, so no order of the work changes them.
//   search   ONCE per call: for every reference the query positions it hits.  A work item (a workgroup) is a reference and 4096 entries of the SHORTER of
//            (reference, query); a lane takes an entry and runs lower_bound in the longer list — reference entries in the query (the hit is where the search
//            ends), or, where the query is the shorter, query entries in the reference (the hit is the lane's own index).  Pass 1 counts the hits of every
//            reference (= common); the host reads the counts, allocates exactly 4 B per hit and gives every reference its range; pass 2 runs the same
//            search and writes the positions: a wave books its item's hits with one atomic on the reference's cursor, a lane's place among them comes
//            from ballots.  The order inside a hit list is whatever the atomics make it.
//   rounds   one byte per query entry says whether it is still live.  Per round, three launches in stream order:
//            count   items of (reference, 4096 of its hits): unique[ref] += live[pos], weight[ref] += live[pos] x count[pos], one atomic pair per wave
//            pick    one workgroup: the largest unique (lowest index among equals); it stops the run (threshold, row limit) by setting `done`, or writes
//                    the row and the winner; either way it zeroes unique[] and weight[] for the next round
//            clear   live[pos] = 0 over the winner's hits (distinct positions: plain stores)
//            Each of them reads `done` first and leaves when it is set, so the host enqueues kGatherBatch rounds at a time and waits once per batch.
//   rest     what is still live after the last reported row, and the sum of its counts.
// No kernel waits on another workgroup; a launch reads what an earlier launch of the stream wrote.  Vector stores and plain C++ only.
#include "ntc_sig_device.hpp"

namespace ntc {

namespace {

constexpr uint32_t kGatherChunk = 4096;            // entries (search) or hits (count) per work item
constexpr uint32_t kGatherLaneItems = kGatherChunk / 256u; // of them per lane
constexpr uint32_t kGatherSearchItems = 1u << 18;  // search work items per launch
constexpr uint32_t kGatherCountBlocks = 1024;      // grid cap of gather_count_kernel (it walks the rest of the items in a grid-stride loop)
constexpr uint32_t kGatherClearBlocks = 1024;      // ... of gather_clear_kernel and gather_rest_kernel
constexpr uint32_t kGatherBatch = 32;              // rounds enqueued between two waits of the host
constexpr uint32_t kGatherMaxRefs = 1024;

// the words the round kernels share
struct GatherState {
	uint32_t done;   // set by the pick that stops the run: every later round kernel leaves at once
	uint32_t winner; // the reference of the round's row
	uint32_t n_rows; // rows written (= rounds that did not stop)
	uint32_t pad;
};

// the list whose range of work items holds `item`: base[0 .. n_lists] ascending, base[0] = 0, item < base[n_lists] (lists without items are stepped over)
__device__ __forceinline__ uint32_t gather_list_of(const unsigned long long* __restrict__ base, uint32_t n_lists, unsigned long long item)
{
	uint32_t lo = 0, hi = n_lists; // the last list with base[list] <= item
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) / 2u;
		if (base[mid] <= item)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// a workgroup per work item first_item + blockIdx.x: kGatherChunk entries of the shorter of (reference, query) searched in the longer.  lists[n_refs] is the
// query.  kWrite == false: common[ref] += hits.  kWrite == true: the positions go to hits[start[ref] + ...], booked on cursor[ref] — common[ref] of them in
// all, as pass 1 counted, so the writes stay inside the reference's range
template <bool kWrite>
__global__ __launch_bounds__(256) void gather_search_kernel(const unsigned long long* const* __restrict__ lists, const uint64_t* __restrict__ ns, uint32_t n_refs,
                                                            const unsigned long long* __restrict__ item_base, unsigned long long first_item,
                                                            unsigned long long* __restrict__ common, const unsigned long long* __restrict__ start,
                                                            uint32_t* __restrict__ cursor, uint32_t* __restrict__ hits)
{
	const unsigned long long item = first_item + blockIdx.x;
	const uint32_t ref = gather_list_of(item_base, n_refs, item);
	const unsigned long long* q = lists[n_refs];
	const unsigned long long* r = lists[ref];
	const uint64_t nq = ns[n_refs], nr = ns[ref];
	const bool by_query = nq < nr; // the query is the shorter: its entries look themselves up in the reference
	const unsigned long long* s = by_query ? q : r;
	const unsigned long long* l = by_query ? r : q;
	const uint64_t n_s = by_query ? nq : nr, n_l = by_query ? nr : nq;
	const uint64_t first = (item - item_base[ref]) * kGatherChunk;
	uint32_t pos[kGatherLaneItems];
	uint32_t hit = 0; // bit t: the lane's entry of turn t is in both lists
#pragma unroll
	for (uint32_t t = 0; t < kGatherLaneItems; ++t) {
		const uint64_t i = first + t * 256u + threadIdx.x;
		pos[t] = 0;
		if (i < n_s) {
			const unsigned long long x = s[i];
			const uint64_t at = list_lower_bound(l, n_l, x);
			if (at < n_l && l[at] == x) {
				hit |= 1u << t;
				pos[t] = (uint32_t)(by_query ? i : at); // (< nq < 2^32)
			}
		}
	}
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave_hits = (uint32_t)wave_sum((unsigned long long)__popc(hit));
	if (!kWrite) {
		if (lane == 0u && wave_hits) atomicAdd(common + ref, (unsigned long long)wave_hits);
		return;
	}
	if (wave_hits == 0u) return; // (the same for the whole wave)
	uint32_t at = 0;
	if (lane == 0u) at = atomicAdd(cursor + ref, wave_hits);
	at = __builtin_amdgcn_readfirstlane(at);
	uint32_t* out = hits + start[ref];
	const unsigned long long room = common[ref]; // (lists that change between the passes must not carry a write out of the range)
#pragma unroll
	for (uint32_t t = 0; t < kGatherLaneItems; ++t) {
		const bool mine = ((hit >> t) & 1u) != 0u;
		const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
		if (mine && at + lanes_below(m) < room) out[at + lanes_below(m)] = pos[t];
		at += (uint32_t)__popcll(m);
	}
}

// work items of (reference, kGatherChunk of its hits), n_items in all, walked gridDim.x at a time: unique[ref] += the live ones among them, weight[ref] += their
// counts (counts == nullptr: 1 each)
__global__ __launch_bounds__(256) void gather_count_kernel(const GatherState* __restrict__ state, const unsigned long long* __restrict__ item_base, uint32_t n_refs,
                                                           unsigned long long n_items, const unsigned long long* __restrict__ common,
                                                           const unsigned long long* __restrict__ start, const uint32_t* __restrict__ hits,
                                                           const unsigned char* __restrict__ live, const uint32_t* __restrict__ counts, uint32_t* __restrict__ unique,
                                                           unsigned long long* __restrict__ weight)
{
	if (state->done) return;
	for (unsigned long long item = blockIdx.x; item < n_items; item += gridDim.x) {
		const uint32_t ref = gather_list_of(item_base, n_refs, item);
		const uint64_t n = common[ref], first = (item - item_base[ref]) * kGatherChunk;
		const uint64_t end = first + kGatherChunk < n ? first + kGatherChunk : n;
		const uint32_t* h = hits + start[ref];
		uint32_t u = 0;
		unsigned long long w = 0;
		for (uint64_t i = first + threadIdx.x; i < end; i += 256u) {
			const uint32_t p = h[i];
			const uint32_t alive = live[p];
			u += alive;
			w += counts ? (unsigned long long)alive * counts[p] : (unsigned long long)alive;
		}
		u = (uint32_t)wave_sum(u);
		w = wave_sum(w);
		if ((threadIdx.x & 63u) == 0u && u) {
			atomicAdd(unique + ref, u);
			atomicAdd(weight + ref, w);
		}
	}
}

// one workgroup.  The reference with the largest unique[], the lowest index among equals.  The run stops — `done`, nothing else is written — when that count
// is below the threshold or row_limit (= min(rows_cap, n_refs)) rows are written; else the round's row and its winner.  unique[] and weight[] are zero again
// when it ends
__global__ __launch_bounds__(256) void gather_pick_kernel(GatherState* __restrict__ state, uint32_t n_refs, unsigned long long threshold, uint32_t row_limit,
                                                          const unsigned long long* __restrict__ common, uint32_t* __restrict__ unique,
                                                          unsigned long long* __restrict__ weight, ntc_gather_row* __restrict__ rows)
{
	__shared__ uint32_t best_u[4], best_i[4];
	if (state->done) return;
	uint32_t bu = 0, bi = ~0u;
	for (uint32_t i = threadIdx.x; i < n_refs; i += 256u) { // (a thread's indices ascend: `>` keeps the lowest of equals)
		const uint32_t u = unique[i];
		if (bi == ~0u || u > bu) bu = u, bi = i;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const uint32_t ou = (uint32_t)__shfl_xor((int)bu, o), oi = (uint32_t)__shfl_xor((int)bi, o);
		if (ou > bu || (ou == bu && oi < bi)) bu = ou, bi = oi;
	}
	if ((threadIdx.x & 63u) == 0u) best_u[threadIdx.x >> 6] = bu, best_i[threadIdx.x >> 6] = bi;
	__syncthreads();
	if (threadIdx.x == 0u) {
#pragma unroll
		for (uint32_t w = 1; w < 4u; ++w)
			if (best_u[w] > bu || (best_u[w] == bu && best_i[w] < bi)) bu = best_u[w], bi = best_i[w];
		const uint32_t n_rows = state->n_rows;
		if ((unsigned long long)bu < threshold || n_rows >= row_limit) { // (bi is a reference: n_refs >= 1 and thread 0 saw index 0)
			state->done = 1u;
		} else {
			ntc_gather_row row;
			row.ref = bi, row.reserved = 0u;
			row.common = common[bi], row.unique = bu, row.unique_weight = weight[bi];
			rows[n_rows] = row;
			state->winner = bi;
			state->n_rows = n_rows + 1u;
		}
	}
	__syncthreads(); // the winner's weight is read
	for (uint32_t i = threadIdx.x; i < n_refs; i += 256u) {
		unique[i] = 0u;
		weight[i] = 0ull;
	}
}

__global__ __launch_bounds__(256) void gather_clear_kernel(const GatherState* __restrict__ state, const unsigned long long* __restrict__ common,
                                                           const unsigned long long* __restrict__ start, const uint32_t* __restrict__ hits, unsigned char* __restrict__ live)
{
	if (state->done) return;
	const uint32_t ref = state->winner;
	const uint64_t n = common[ref];
	const uint32_t* h = hits + start[ref];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		live[h[i]] = 0;
}

// out[0] += the live entries, out[1] += their counts (counts == nullptr: 1 each)
__global__ __launch_bounds__(256) void gather_rest_kernel(const unsigned char* __restrict__ live, const uint32_t* __restrict__ counts, uint64_t nq,
                                                          unsigned long long* __restrict__ out)
{
	unsigned long long u = 0, w = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nq; i += (uint64_t)gridDim.x * 256u) {
		const unsigned long long alive = live[i];
		u += alive;
		w += counts ? alive * counts[i] : alive;
	}
	u = wave_sum(u);
	w = wave_sum(w);
	if ((threadIdx.x & 63u) == 0u && u) {
		atomicAdd(out, u);
		atomicAdd(out + 1, w);
	}
}

} // namespace

} // namespace ntc

using namespace ntc_eng;

extern "C" {

int ntc_signature_gather_device(int32_t device, void* stream, const void* d_query_u64, const void* d_query_counts_u32, uint64_t nq, uint32_t n_refs,
                                const void* const* d_refs_u64, const uint64_t* n, uint64_t threshold, ntc_gather_row* rows, uint32_t rows_cap, uint32_t* n_rows,
                                uint64_t* unassigned, uint64_t* unassigned_weight)
{
	using namespace ntc;
	if (n_refs < 1 || n_refs > kGatherMaxRefs) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: %u references (1 .. 1024 are taken)", n_refs);
	if (!d_refs_u64 || !n || !n_rows || (!rows && rows_cap)) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: null argument");
	if (nq >> 32) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: the query has %llu entries (fewer than 2^32 are taken)", (unsigned long long)nq);
	if (!d_query_u64 && nq) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: the query is null and has %llu entries", (unsigned long long)nq);
	for (uint32_t i = 0; i < n_refs; ++i) {
		if (n[i] >> 32) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: reference %u has %llu entries (fewer than 2^32 are taken)", i, (unsigned long long)n[i]);
		if (!d_refs_u64[i] && n[i]) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: reference %u is null and has %llu entries", i, (unsigned long long)n[i]);
	}
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const size_t nr = n_refs, nl = nr + 1; // the lists: the references, then the query
	const uint32_t row_limit = std::min(rows_cap, n_refs);
	if (threshold == 0) threshold = 1;
	// the lists' extra words (8 B each): [common nr][search item base nl][count item base nl][start nr][weight nr][rest 2]
	const size_t x_common = 0, x_sbase = nr, x_cbase = x_sbase + nl, x_start = x_cbase + nl, x_weight = x_start + nr, x_rest = x_weight + nr, n_extra = x_rest + 2;
	SigLists lists;
	DevBuf<uint32_t> d_u; // device words (4 B each): [cursor nr][unique nr]
	DevBuf<GatherState> d_state;
	DevBuf<ntc_gather_row> d_rows;
	DevBuf<unsigned char> d_live;
	DevBuf<uint32_t> d_hits;
	if (!lists.reserve(nl, n_extra, n_extra) || !d_u.reserve(2 * nr * 4) || !d_state.reserve(sizeof(GatherState)) ||
	    !d_rows.reserve((size_t)std::max(row_limit, 1u) * sizeof(ntc_gather_row)) || !d_live.reserve((size_t)std::max<uint64_t>(nq, 1))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_gather_device: cannot allocate %zu B of scratch on device; nothing was written",
		            lists.bytes() + 2 * nr * 4 + sizeof(GatherState) + (size_t)std::max(row_limit, 1u) * sizeof(ntc_gather_row) + (size_t)std::max<uint64_t>(nq, 1));
	}
	unsigned long long* const x = lists.extra();
	unsigned long long search_items = 0;
	for (size_t i = 0; i < nl; ++i) {
		const uint64_t len = i < nr ? n[i] : nq;
		lists.set(i, i < nr ? d_refs_u64[i] : d_query_u64, len);
		x[x_sbase + i] = search_items;
		if (i < nr) search_items += (std::min(len, nq) + kGatherChunk - 1) / kGatherChunk;
	}
	HIP_TRY(lists.start(st));
	HIP_TRY(hipMemsetAsync(d_u, 0, 2 * nr * 4, st));
	HIP_TRY(hipMemsetAsync(d_state, 0, sizeof(GatherState), st));
	if (nq) HIP_TRY(hipMemsetAsync(d_live, 1, nq, st));
	unsigned long long* const d_common = lists.d_extra() + x_common;
	unsigned long long* const d_start = lists.d_extra() + x_start;
	unsigned long long* const d_weight = lists.d_extra() + x_weight;
	uint32_t* d_cursor = d_u.get();
	uint32_t* d_unique = d_u.get() + nr;
	const uint32_t* d_counts = (const uint32_t*)d_query_counts_u32;
	// pass 1 of the search.  An unsorted list makes its searches miss or hit at random but keeps them inside the list, and its result is thrown away below
	auto search = [&](bool write) {
		for (unsigned long long first = 0; first < search_items; first += kGatherSearchItems) {
			const unsigned grid = (unsigned)std::min<unsigned long long>(kGatherSearchItems, search_items - first);
			if (write)
				hipLaunchKernelGGL(gather_search_kernel<true>, dim3(grid), dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), n_refs, lists.d_extra() + x_sbase, first, d_common, d_start,
				                   d_cursor, d_hits.get());
			else
				hipLaunchKernelGGL(gather_search_kernel<false>, dim3(grid), dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), n_refs, lists.d_extra() + x_sbase, first, d_common, d_start,
				                   d_cursor, (uint32_t*)nullptr);
		}
	};
	search(false);
	HIP_TRY(hipGetLastError());
	HIP_TRY(lists.read_back(st, nr)); // the bad entries and common[]
	HIP_TRY(hipStreamSynchronize(st)); // the one wait of the search: every list is checked and every reference's hits are counted
	if (lists.bad(nr) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: the query is not strictly ascending at entry %llu", lists.bad(nr));
	for (size_t i = 0; i < nr; ++i)
		if (lists.bad(i) != kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_gather_device: reference %zu is not strictly ascending at entry %llu", i, lists.bad(i));
	unsigned long long total_hits = 0, count_items = 0, most_hits = 0;
	for (size_t i = 0; i < nr; ++i) {
		const unsigned long long c = x[x_common + i];
		x[x_start + i] = total_hits;
		x[x_cbase + i] = count_items;
		total_hits += c;
		count_items += (c + kGatherChunk - 1) / kGatherChunk;
		most_hits = std::max(most_hits, c);
	}
	x[x_cbase + nr] = count_items;
	if (!d_hits.reserve((size_t)std::max<unsigned long long>(total_hits, 1) * 4)) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_gather_device: cannot allocate %llu B for the hit lists on device; nothing was written", total_hits * 4);
	}
	HIP_TRY(hipMemcpyAsync(lists.d_extra() + x_cbase, x + x_cbase, (nl + nr) * 8, hipMemcpyHostToDevice, st)); // the count items' base and the starts
	if (total_hits) HIP_TRY(hipMemsetAsync(d_hits, 0, (size_t)total_hits * 4, st)); // (pass 2 writes every entry; a list changed under the call leaves valid positions)
	search(true);
	HIP_TRY(hipGetLastError());
	// the rounds: at most row_limit of them write a row and one more stops the run
	GatherState state{};
	const unsigned count_grid = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(count_items, kGatherCountBlocks));
	const unsigned clear_grid = capped_grid(most_hits, kGatherClearBlocks);
	for (uint64_t enqueued = 0; !state.done;) {
		const uint64_t batch = std::min<uint64_t>(kGatherBatch, (uint64_t)row_limit + 1 - enqueued);
		if (batch == 0) return fail(NTC_ERR_DEVICE, "ntc_signature_gather_device: the rounds did not stop after %llu of them", (unsigned long long)enqueued);
		for (uint64_t r = 0; r < batch; ++r) {
			if (count_items)
				hipLaunchKernelGGL(gather_count_kernel, dim3(count_grid), dim3(256), 0, st, (const GatherState*)d_state.get(), lists.d_extra() + x_cbase, n_refs, count_items,
				                   d_common, d_start, (const uint32_t*)d_hits.get(), (const unsigned char*)d_live.get(), d_counts, d_unique,
				                   d_weight);
			hipLaunchKernelGGL(gather_pick_kernel, dim3(1), dim3(256), 0, st, d_state.get(), n_refs, (unsigned long long)threshold, row_limit, d_common, d_unique,
			                   d_weight, d_rows.get());
			if (most_hits)
				hipLaunchKernelGGL(gather_clear_kernel, dim3(clear_grid), dim3(256), 0, st, (const GatherState*)d_state.get(), d_common, d_start,
				                   (const uint32_t*)d_hits.get(), d_live.get());
		}
		HIP_TRY(hipGetLastError());
		enqueued += batch;
		HIP_TRY(hipMemcpyAsync(&state, d_state, sizeof state, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	if (nq) hipLaunchKernelGGL(gather_rest_kernel, dim3(capped_grid(nq, kGatherClearBlocks)), dim3(256), 0, st, (const unsigned char*)d_live.get(), d_counts, nq, lists.d_extra() + x_rest);
	HIP_TRY(hipGetLastError());
	std::vector<ntc_gather_row> got(state.n_rows);
	unsigned long long rest[2] = {0, 0};
	if (state.n_rows) HIP_TRY(hipMemcpyAsync(got.data(), d_rows, got.size() * sizeof(ntc_gather_row), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(rest, lists.d_extra() + x_rest, sizeof rest, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	std::copy(got.begin(), got.end(), rows);
	*n_rows = state.n_rows;
	if (unassigned) *unassigned = rest[0];
	if (unassigned_weight) *unassigned_weight = rest[1];
	return 0;
}

} // extern "C"
