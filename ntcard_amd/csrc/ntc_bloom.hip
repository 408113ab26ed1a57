// ntc_bloom.hip — Bloom filters of EVERY k-mer on the device (include/ntcard_hip.h: ntc_bloom_*_device; DESIGN.md §4 "Bloom filters").  The layout is the
// reference's vendor/ntHash/lib/BloomFilter.hpp:56-66: position loc = h_i % m_bits, bit 7 - loc % 8 of byte loc / 8; h_0 the window's value, h_i the
// multi-hash of nthash.hpp:381-390.  Engine-less tools: kernels and their entry points in one file.
//
// The walk over the input (stage as codes, mark sequence starts, 16 window starts per lane, roll), the remainder by m_bits, the argument checks and the
// plain filter's view (BitsView: set the n_hash bits of a value, test them) are ntc_bloom_walk.hpp's, shared with the counting and the blocked filters
// (ntc_cbloom.hip, ntc_bbloom.hip): here are the entry points — the shared actions and kernels over that view — and the streaming kernels of a bit image.
#include "ntc_bloom_walk.hpp"

using namespace ntc_eng;
using namespace ntc_bloom;

namespace {

// out[0] += the set bits of the filter's first m_bits; out[1] += the set bits behind them (last_mask: the bits of the LAST dword that are below m_bits)
__global__ __launch_bounds__(256) void bloom_popcount_kernel(const uint32_t* __restrict__ filter, uint64_t n_words, uint32_t last_mask, unsigned long long* out)
{
	__shared__ unsigned long long part[4];
	unsigned long long sum = 0;
	uint32_t pad = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t w = filter[i];
		if (i + 1u == n_words) {
			sum += (uint32_t)__popc(w & last_mask);
			pad = (uint32_t)__popc(w & ~last_mask);
		} else {
			sum += (uint32_t)__popc(w);
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		sum += (unsigned long long)__shfl_xor((long long)sum, o);
	if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = sum;
	__syncthreads();
	if (threadIdx.x == 0) atomicAdd(&out[0], part[0] + part[1] + part[2] + part[3]);
	if (pad) atomicAdd(&out[1], (unsigned long long)pad);
}

__global__ __launch_bounds__(256) void bloom_or_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint64_t n_words)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t s = src[i];
		if (s) dst[i] |= s;
	}
}

} // namespace

extern "C" {

int ntc_bloom_insert_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                            const uint64_t* offsets, uint64_t n_seqs, uint64_t* n_windows)
{
	if (int rc = check_filter("ntc_bloom_insert_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_input("ntc_bloom_insert_device", strand, d_bases, offsets, n_seqs)) return rc;
	const InsertAct<BitsView> act{bits_view(d_filter, m_bits, n_hash, k)};
	return walk_total("ntc_bloom_insert_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, n_windows);
}

int ntc_bloom_query_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                           const uint64_t* offsets, uint64_t n_seqs, void* d_windows_u32, void* d_hits_u32)
{
	if (int rc = check_filter("ntc_bloom_query_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_input("ntc_bloom_query_device", strand, d_bases, offsets, n_seqs)) return rc;
	const TestAct<BitsView> act{bits_view(d_filter, m_bits, n_hash, k)};
	return walk_per_seq("ntc_bloom_query_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, d_windows_u32, d_hits_u32);
}

int ntc_bloom_insert_hashes_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n)
{
	if (int rc = check_filter("ntc_bloom_insert_hashes_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_bloom_insert_hashes_device", d_h0_u64, n)) return rc;
	if (n == 0) return 0;
	return launch_strided(device, stream, insert_hashes_kernel<BitsView>, n, bits_view(d_filter, m_bits, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n);
}

int ntc_bloom_query_hashes_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n,
                                  void* d_flags_u8)
{
	if (int rc = check_filter("ntc_bloom_query_hashes_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_bloom_query_hashes_device", d_h0_u64, n, "hashes or flags", d_flags_u8 != nullptr)) return rc;
	if (n == 0) return 0;
	return launch_strided(device, stream, query_hashes_kernel<BitsView>, n, bits_view(d_filter, m_bits, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n,
	                      static_cast<unsigned char*>(d_flags_u8));
}

int ntc_bloom_popcount_device(int32_t device, void* stream, const void* d_filter, uint64_t m_bits, uint64_t* pop)
{
	if (int rc = check_filter("ntc_bloom_popcount_device", d_filter, m_bits, 1, 1)) return rc;
	if (!pop) return fail(NTC_ERR_ARG, "ntc_bloom_popcount_device: null pop");
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf<unsigned long long> d_out; // (scratch of this call: freed on every way out)
	if (!d_out.reserve(16)) return fail(NTC_ERR_MEMORY, "ntc_bloom_popcount_device: cannot allocate 16 B of scratch on device");
	HIP_TRY(hipMemsetAsync(d_out, 0, 16, st));
	const uint64_t n_words = filter_words(m_bits);
	uint32_t last_mask = 0; // the positions of the last dword that are below m_bits, by the bit rule
	for (uint64_t loc = (n_words - 1) * 32; loc < m_bits; ++loc)
		last_mask |= bloom_bit(loc);
	hipLaunchKernelGGL(bloom_popcount_kernel, dim3(stride_grid(n_words)), dim3(256), 0, st, static_cast<const uint32_t*>(d_filter), n_words, last_mask, d_out.get());
	HIP_TRY(hipGetLastError());
	unsigned long long out[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(out, d_out, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (out[1] != 0) return fail(NTC_ERR_STATE, "ntc_bloom_popcount_device: %llu bits are set behind the filter's m_bits=%llu", out[1], (unsigned long long)m_bits);
	*pop = out[0];
	return 0;
}

int ntc_bloom_or_device(int32_t device, void* stream, void* d_dst, const void* d_src, uint64_t m_bits)
{
	if (int rc = check_filter("ntc_bloom_or_device", d_dst, m_bits, 1, 1)) return rc;
	if (int rc = check_filter("ntc_bloom_or_device", d_src, m_bits, 1, 1)) return rc;
	if (d_dst == d_src) return 0;
	const uint64_t n_words = filter_words(m_bits);
	return launch_strided(device, stream, bloom_or_kernel, n_words, static_cast<uint32_t*>(d_dst), static_cast<const uint32_t*>(d_src), n_words);
}

} // extern "C"
