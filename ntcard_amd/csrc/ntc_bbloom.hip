// ntc_bbloom.hip — BLOCKED Bloom filters on the device (include/ntcard_hip.h: ntc_bbloom_*_device; DESIGN.md §4 "Blocked filters"): every bit of a k-mer
// in one aligned 512-bit block, one random cache line per k-mer where the plain filter (ntc_bloom.hip) fetches n_hash.  The block arithmetic is
// ntc_bbloom.hpp's, and so is the blocked filter's view (BlockedView); the walk over the input, the remainder, the checks, the insert and test actions
// and the kernels over given h_0 values are ntc_bloom_walk.hpp's templates over a view: here are the entry points and the histogram of the blocks' set bits.  The image is an ordinary bit image in the plain filter's bit rule:
// ntc_bloom_popcount_device and ntc_bloom_or_device serve it as they are.  (The solid insert with a blocked destination is in ntc_cbloom.hip, beside the
// counters it reads.)
#include "ntc_bbloom.hpp"

using namespace ntc_eng;
using namespace ntc_bloom;

namespace {

// out[v] += the blocks that hold v set bits, v = 0 .. 512.  A lane takes a block: its 16 dwords as four 16-byte loads where the filter is 16-byte aligned
// (`wide`), else dword by dword.  One histogram per workgroup in LDS (a workgroup sees fewer than 2^31 blocks), one global add per used bin; the empty
// blocks — most of a filter at the start of a build — are counted in registers.
__global__ __launch_bounds__(256) void bbloom_hist_kernel(const uint32_t* __restrict__ filter, uint64_t n_blocks, uint32_t wide, unsigned long long* out)
{
	__shared__ uint32_t h[kBlockBits + 1u];
	for (uint32_t s = threadIdx.x; s <= kBlockBits; s += 256u)
		h[s] = 0;
	__syncthreads();
	uint32_t n0 = 0;
	for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < n_blocks; b += (uint64_t)gridDim.x * 256u) {
		uint32_t v = 0;
		if (wide) {
			const uint4* q = reinterpret_cast<const uint4*>(filter) + 4u * b;
#pragma unroll
			for (uint32_t d = 0; d < 4; ++d) {
				const uint4 x = q[d];
				v += (uint32_t)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w));
			}
		} else {
#pragma unroll
			for (uint32_t d = 0; d < 16; ++d)
				v += (uint32_t)__popc(filter[16u * b + d]);
		}
		if (v == 0)
			++n0;
		else
			atomicAdd(&h[v], 1u);
	}
	if (n0) atomicAdd(&h[0], n0);
	__syncthreads();
	for (uint32_t s = threadIdx.x; s <= kBlockBits; s += 256u)
		if (h[s]) atomicAdd(&out[s], (unsigned long long)h[s]);
}

} // namespace

extern "C" {

int ntc_bbloom_insert_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                             const uint64_t* offsets, uint64_t n_seqs, uint64_t* n_windows)
{
	if (int rc = check_blocked("ntc_bbloom_insert_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_input("ntc_bbloom_insert_device", strand, d_bases, offsets, n_seqs)) return rc;
	const InsertAct<BlockedView> act{blocked_view(d_filter, m_bits, n_hash, k)};
	return walk_total("ntc_bbloom_insert_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, n_windows);
}

int ntc_bbloom_query_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                            const uint64_t* offsets, uint64_t n_seqs, void* d_windows_u32, void* d_hits_u32)
{
	if (int rc = check_blocked("ntc_bbloom_query_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_input("ntc_bbloom_query_device", strand, d_bases, offsets, n_seqs)) return rc;
	const TestAct<BlockedView> act{blocked_view(d_filter, m_bits, n_hash, k)};
	return walk_per_seq("ntc_bbloom_query_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, d_windows_u32, d_hits_u32);
}

int ntc_bbloom_insert_hashes_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n)
{
	if (int rc = check_blocked("ntc_bbloom_insert_hashes_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_bbloom_insert_hashes_device", d_h0_u64, n)) return rc;
	if (n == 0) return 0;
	return launch_strided(device, stream, insert_hashes_kernel<BlockedView>, n, blocked_view(d_filter, m_bits, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n);
}

int ntc_bbloom_query_hashes_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n,
                                   void* d_flags_u8)
{
	if (int rc = check_blocked("ntc_bbloom_query_hashes_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_bbloom_query_hashes_device", d_h0_u64, n)) return rc;
	if (n && !d_flags_u8) return fail(NTC_ERR_ARG, "ntc_bbloom_query_hashes_device: null flags");
	if (n == 0) return 0;
	return launch_strided(device, stream, query_hashes_kernel<BlockedView>, n, blocked_view(d_filter, m_bits, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n,
	                      static_cast<unsigned char*>(d_flags_u8));
}

int ntc_bbloom_hist_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint64_t* hist_u64)
{
	if (int rc = check_blocked("ntc_bbloom_hist_device", d_filter, m_bits, 1, 1)) return rc;
	if (!hist_u64) return fail(NTC_ERR_ARG, "ntc_bbloom_hist_device: null hist");
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	constexpr size_t kBytes = (kBlockBits + 1u) * 8u;
	DevBuf<unsigned long long> d_out; // (scratch of this call: freed on every way out)
	if (!d_out.reserve(kBytes)) return fail(NTC_ERR_MEMORY, "ntc_bbloom_hist_device: cannot allocate %zu B of scratch on device", kBytes);
	HIP_TRY(hipMemsetAsync(d_out, 0, kBytes, st));
	const uint64_t n_blocks = m_bits / kBlockBits;
	hipLaunchKernelGGL(bbloom_hist_kernel, dim3(stride_grid(n_blocks)), dim3(256), 0, st, static_cast<const uint32_t*>(d_filter), n_blocks,
	                   ((uintptr_t)d_filter & 15u) == 0 ? 1u : 0u, d_out.get());
	HIP_TRY(hipGetLastError());
	unsigned long long out[kBlockBits + 1u];
	HIP_TRY(hipMemcpyAsync(out, d_out, kBytes, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (uint32_t v = 0; v <= kBlockBits; ++v)
		hist_u64[v] = out[v];
	return 0;
}

} // extern "C"
