// ntc_sig_device.hpp — what the signature translation units share (ntc_signature.hip, ntc_sig_sort.hip, ntc_sig_lists.hip, ntc_sig_gather.hip; DESIGN.md §4
// "Signatures"): the wave helpers of their kernels, the clamp of their grids, and SigLists, the owner of "lists on the device" under compare, matrix and
// gather.  Vector stores and plain C++ only.
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
