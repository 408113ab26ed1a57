// ntc_sig_device.hpp — what the signature translation units share (ntc_signature.hip, ntc_sig_sort.hip, ntc_sig_lists.hip, ntc_sig_gather.hip, ntc_sig_algebra.hip; DESIGN.md §4
// "Signatures"): the wave helpers of their kernels, the clamp of their grids, and SigLists, the owner of "lists on the device" under compare, matrix,
// gather and the set algebra.  Vector stores and plain C++ only.
#pragma once
#include "ntc_engine.hpp"

namespace ntc {

// of the lanes whose bit is set in m, those below the calling lane
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// the sum of x over the wave, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
	uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned long long y = ((unsigned long long)(uint32_t)__shfl_xor((int)hi, o) << 32) | (uint32_t)__shfl_xor((int)lo, o);
		x += y;
		lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
	}
	return x;
}

// the first active lane's x, in every lane
__device__ __forceinline__ unsigned long long wave_first(unsigned long long x)
{
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
	return ((unsigned long long)hi << 32) | lo;
}

// the first index >= x of the ascending list l[0 .. n) (any list: the search stays inside [0, n])
__device__ __forceinline__ uint64_t list_lower_bound(const unsigned long long* __restrict__ l, uint64_t n, unsigned long long x)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (l[mid] < x)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// h[d] += 1 for every valid lane (whole waves call this).  The lanes that hold the first lane's d send one add: a value most lanes agree in — a signature's top
// bits, a nearly full bin, the count 1 of a spectrum — is not 64 adds to one LDS address
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t d, bool valid)
{
	const uint32_t first = __builtin_amdgcn_readfirstlane(d);
	const uint64_t same = __builtin_amdgcn_ballot_w64(valid && d == first);
	if (!valid) return;
	if (d != first)
		atomicAdd(h + d, 1u);
	else if (lanes_below(same) == 0u)
		atomicAdd(h + d, (uint32_t)__popcll(same));
}

// exclusive prefix sum of v over a workgroup of 256 threads; total = the sum.  wsum: 4 words of LDS, free again on return
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t& total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t inc = v;
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
		if (lane >= o) inc += t;
	}
	if (lane == 63u) wsum[wave] = inc;
	__syncthreads();
	uint32_t pre = 0;
	total = 0;
#pragma unroll
	for (uint32_t w = 0; w < 4u; ++w) {
		const uint32_t s = wsum[w];
		pre += w < wave ? s : 0u;
		total += s;
	}
	__syncthreads();
	return pre + inc - v;
}

// workgroups of 256 threads for n entries, one at least and `cap` at most (the kernel walks the rest in a grid-stride loop)
inline unsigned capped_grid(uint64_t n, uint32_t cap) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, cap)); }

constexpr unsigned long long kNoBad = ~0ull; // SigLists::bad() of a list that ascends

// Lists of u64 on the device, handed to kernels as one table of device words
//     [pointers n_lists][lengths n_lists][first bad entry n_lists][extra words of the caller]
// with a host mirror of the table and of the first `mirrored` extra words.  start() uploads the mirror and launches the ascent check of every list
// (ntc_sig_lists.hip: sig_ascent_kernel); read_back() brings the bad entries home.  Both are asynchronous: the caller owns the wait, and bad() holds after it.
// The extra words ride in the same allocation, upload and read-back, so a caller's own words (compare's {hits, sum}, the matrix' cells, gather's
// sections) cost no second one.
class SigLists {
public:
	bool reserve(size_t n_lists, size_t extra, size_t mirrored); // false: no device memory for bytes() (the mirror: bad = kNoBad, extra words = 0)
	void set(size_t i, const void* d_list, uint64_t n);
	hipError_t start(hipStream_t st);                             // the upload, then one ascent launch (none where no list has two entries)
	hipError_t read_back(hipStream_t st, size_t extra_words = 0); // the bad entries and the first extra_words (<= mirrored) extra words, one copy
	size_t bytes() const { return (3 * nl_ + extra_) * 8; }
	const unsigned long long* const* d_ptrs() const { return (const unsigned long long* const*)d_.get(); }
	const uint64_t* d_lens() const { return (const uint64_t*)(d_.get() + nl_); }
	unsigned long long* d_extra() const { return d_.get() + 3 * nl_; }
	unsigned long long* extra() { return w_.data() + 3 * nl_; } // the mirror of the first `mirrored` extra words
	unsigned long long bad(size_t i) const { return w_[2 * nl_ + i]; } // the smallest i >= 1 with l[i - 1] >= l[i]; kNoBad: strictly ascending

private:
	size_t nl_ = 0, extra_ = 0;
	uint64_t longest_ = 0;
	ntc_eng::DevBuf<unsigned long long> d_;
	std::vector<unsigned long long> w_;
};

} // namespace ntc
