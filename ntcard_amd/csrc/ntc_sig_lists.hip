// ntc_sig_lists.hip — sorted hash lists on the device: SigLists (ntc_sig_device.hpp) with the one ascent check every consumer of such lists runs, and the
// intersections of two lists and of all pairs of many (include/ntcard_hip.h: ntc_signature_compare_device, ntc_signature_matrix_device; DESIGN.md §4
// "Signatures", "Sort and compare").  Gather (ntc_sig_gather.hip) is the third consumer.
// No kernel waits on another workgroup; a launch reads what an earlier launch wrote.  Vector stores and plain C++ only.
#include "ntc_sig_device.hpp"

namespace ntc {

namespace {

constexpr uint32_t kAscentBlocks = 1024; // grid cap of sig_ascent_kernel (per list)
constexpr uint32_t kCompareBlocks = 8192; // ... of sig_compare_kernel
constexpr uint32_t kMatChunk = 4096;     // entries of a pair's shorter list per work item (a workgroup)
constexpr uint32_t kMatItems = 1u << 18; // work items per launch: the scratch that holds them is 4 MiB whatever the number of pairs

struct MatItem {
	uint32_t i, j;  // the pair, i < j
	uint64_t start; // first entry of the shorter list
};

// bad[list] = the smallest i >= 1 with a[i - 1] >= a[i] (kNoBad: strictly ascending); blockIdx.y = the list
__global__ __launch_bounds__(256) void sig_ascent_kernel(const unsigned long long* const* __restrict__ lists, const uint64_t* __restrict__ ns, unsigned long long* __restrict__ bad)
{
	const uint32_t li = blockIdx.y;
	const unsigned long long* a = lists[li];
	const uint64_t n = ns[li];
	for (uint64_t i = 1 + (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
		if (a[i - 1] >= a[i]) atomicMin(bad + li, (unsigned long long)i);
}

// every lane an entry of the shorter list, searched in the longer one; out[0] += hits, out[1] += min(count, count) of the hits (cs != nullptr): one atomic
// each per wave
__global__ __launch_bounds__(256) void sig_compare_kernel(const unsigned long long* __restrict__ s, const uint32_t* __restrict__ cs, uint64_t ns,
                                                          const unsigned long long* __restrict__ l, const uint32_t* __restrict__ cl, uint64_t nl,
                                                          unsigned long long* __restrict__ out)
{
	unsigned long long hits = 0, sum = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < ns; i += (uint64_t)gridDim.x * 256u) {
		const unsigned long long x = s[i];
		const uint64_t at = list_lower_bound(l, nl, x);
		if (at < nl && l[at] == x) {
			++hits;
			if (cs) sum += (unsigned long long)(cs[i] < cl[at] ? cs[i] : cl[at]);
		}
	}
	hits = wave_sum(hits);
	sum = wave_sum(sum);
	if ((threadIdx.x & 63u) == 0u) {
		if (hits) atomicAdd(out, hits);
		if (sum) atomicAdd(out + 1, sum);
	}
}

// a workgroup per work item: kMatChunk entries of the pair's shorter list against the longer one; counts[i * n_sigs + j] += hits, one atomic per wave
__global__ __launch_bounds__(256) void sig_matrix_kernel(const unsigned long long* const* __restrict__ lists, const uint64_t* __restrict__ ns, const MatItem* __restrict__ items,
                                                         uint32_t n_sigs, unsigned long long* __restrict__ counts)
{
	const MatItem it = items[blockIdx.x];
	const uint64_t ni = ns[it.i], nj = ns[it.j];
	const bool i_short = ni <= nj;
	const unsigned long long* s = i_short ? lists[it.i] : lists[it.j];
	const unsigned long long* l = i_short ? lists[it.j] : lists[it.i];
	const uint64_t n_s = i_short ? ni : nj, n_l = i_short ? nj : ni;
	const uint64_t end = it.start + kMatChunk < n_s ? it.start + kMatChunk : n_s;
	unsigned long long hits = 0;
	for (uint64_t q = it.start + threadIdx.x; q < end; q += 256u) {
		const unsigned long long x = s[q];
		const uint64_t at = list_lower_bound(l, n_l, x);
		hits += (at < n_l && l[at] == x) ? 1u : 0u;
	}
	hits = wave_sum(hits);
	if ((threadIdx.x & 63u) == 0u && hits) atomicAdd(counts + (uint64_t)it.i * n_sigs + it.j, hits);
}

} // namespace

bool SigLists::reserve(size_t n_lists, size_t extra, size_t mirrored)
{
	nl_ = n_lists, extra_ = extra, longest_ = 0;
	w_.assign(3 * nl_ + mirrored, 0ull);
	std::fill(w_.begin() + 2 * nl_, w_.begin() + 3 * nl_, kNoBad);
	return d_.reserve(bytes());
}

void SigLists::set(size_t i, const void* d_list, uint64_t n)
{
	w_[i] = (unsigned long long)(uintptr_t)d_list;
	w_[nl_ + i] = n;
	longest_ = std::max(longest_, n);
}

hipError_t SigLists::start(hipStream_t st)
{
	const hipError_t rc = hipMemcpyAsync(d_, w_.data(), w_.size() * 8, hipMemcpyHostToDevice, st);
	if (rc != hipSuccess || longest_ < 2) return rc;
	hipLaunchKernelGGL(sig_ascent_kernel, dim3(capped_grid(longest_, kAscentBlocks), (unsigned)nl_), dim3(256), 0, st, d_ptrs(), d_lens(), d_.get() + 2 * nl_);
	return hipGetLastError();
}

hipError_t SigLists::read_back(hipStream_t st, size_t extra_words)
{
	return hipMemcpyAsync(w_.data() + 2 * nl_, d_.get() + 2 * nl_, (nl_ + extra_words) * 8, hipMemcpyDeviceToHost, st);
}

} // namespace ntc

using namespace ntc_eng;

extern "C" {

int ntc_signature_compare_device(int32_t device, void* stream, const void* d_a_u64, const void* d_ca_u32, uint64_t na, const void* d_b_u64, const void* d_cb_u32,
                                 uint64_t nb, uint64_t* n_common, uint64_t* min_sum)
{
	if (!n_common || (!d_a_u64 && na) || (!d_b_u64 && nb)) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: null argument");
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const bool weigh = d_ca_u32 && d_cb_u32 && min_sum;
	ntc::SigLists lists; // extra words: the hits, the sum
	if (!lists.reserve(2, 2, 2)) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_compare_device: cannot allocate %zu B on device", lists.bytes());
	}
	lists.set(0, d_a_u64, na);
	lists.set(1, d_b_u64, nb);
	HIP_TRY(lists.start(st));
	if (na && nb) {
		const bool a_short = na <= nb;
		const uint64_t n_s = a_short ? na : nb;
		hipLaunchKernelGGL(ntc::sig_compare_kernel, dim3(ntc::capped_grid(n_s, ntc::kCompareBlocks)), dim3(256), 0, st, (const unsigned long long*)(a_short ? d_a_u64 : d_b_u64),
		                   weigh ? (const uint32_t*)(a_short ? d_ca_u32 : d_cb_u32) : nullptr, n_s, (const unsigned long long*)(a_short ? d_b_u64 : d_a_u64),
		                   weigh ? (const uint32_t*)(a_short ? d_cb_u32 : d_ca_u32) : nullptr, a_short ? nb : na, lists.d_extra());
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(lists.read_back(st, 2));
	HIP_TRY(hipStreamSynchronize(st));
	if (lists.bad(0) != ntc::kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: the first list is not strictly ascending at entry %llu", lists.bad(0));
	if (lists.bad(1) != ntc::kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: the second list is not strictly ascending at entry %llu", lists.bad(1));
	*n_common = lists.extra()[0];
	if (weigh) *min_sum = lists.extra()[1];
	return 0;
}

int ntc_signature_matrix_device(int32_t device, void* stream, uint32_t n_sigs, const void* const* d_hashes_u64, const uint64_t* n, uint64_t* common_out)
{
	if (n_sigs < 1 || n_sigs > 1024) return fail(NTC_ERR_ARG, "ntc_signature_matrix_device: %u lists (1 .. 1024 are taken)", n_sigs);
	if (!d_hashes_u64 || !n || !common_out) return fail(NTC_ERR_ARG, "ntc_signature_matrix_device: null argument");
	for (uint32_t i = 0; i < n_sigs; ++i)
		if (!d_hashes_u64[i] && n[i]) return fail(NTC_ERR_ARG, "ntc_signature_matrix_device: list %u is null and has %llu entries", i, (unsigned long long)n[i]);
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const size_t ns = n_sigs, cells = ns * ns;
	ntc::SigLists lists; // extra words: the counts of the pairs, n_sigs x n_sigs (zeroed on the device, read once at the end)
	DevBuf<ntc::MatItem> d_items; // the work items of a round
	if (!lists.reserve(ns, cells, 0) || !d_items.reserve((size_t)ntc::kMatItems * sizeof(ntc::MatItem))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_matrix_device: cannot allocate %zu B of scratch on device", lists.bytes() + (size_t)ntc::kMatItems * sizeof(ntc::MatItem));
	}
	for (size_t i = 0; i < ns; ++i)
		lists.set(i, d_hashes_u64[i], n[i]);
	HIP_TRY(lists.start(st));
	HIP_TRY(hipMemsetAsync(lists.d_extra(), 0, cells * 8, st));
	HIP_TRY(lists.read_back(st));
	HIP_TRY(hipStreamSynchronize(st)); // every list is checked once, before any pair is looked at
	for (size_t i = 0; i < ns; ++i)
		if (lists.bad(i) != ntc::kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_matrix_device: list %zu is not strictly ascending at entry %llu", i, lists.bad(i));
	// rounds of at most kMatItems work items: the launches grow with the entries to search, not with the pairs
	std::vector<ntc::MatItem> items;
	items.reserve(ntc::kMatItems);
	auto run_round = [&]() -> int {
		if (items.empty()) return 0;
		HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ntc::MatItem), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(ntc::sig_matrix_kernel, dim3((unsigned)items.size()), dim3(256), 0, st, lists.d_ptrs(), lists.d_lens(), (const ntc::MatItem*)d_items.get(), n_sigs,
		                   lists.d_extra());
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(st)); // (the host items and d_items are reused by the next round)
		items.clear();
		return 0;
	};
	for (uint32_t i = 0; i < n_sigs; ++i)
		for (uint32_t j = i + 1; j < n_sigs; ++j) {
			const uint64_t n_s = std::min(n[i], n[j]);
			for (uint64_t start = 0; start < n_s; start += ntc::kMatChunk) {
				items.push_back(ntc::MatItem{i, j, start});
				if (items.size() == ntc::kMatItems)
					if (int rc = run_round()) return rc;
			}
		}
	if (int rc = run_round()) return rc;
	std::vector<unsigned long long> counts(cells);
	HIP_TRY(hipMemcpyAsync(counts.data(), lists.d_extra(), cells * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (size_t i = 0; i < ns; ++i) {
		common_out[i * ns + i] = n[i];
		for (size_t j = i + 1; j < ns; ++j)
			common_out[i * ns + j] = common_out[j * ns + i] = counts[i * ns + j];
	}
	return 0;
}

} // extern "C"
