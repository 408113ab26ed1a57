// ntc_cbloom.hip — COUNTING Bloom filters on the device (include/ntcard_hip.h: ntc_cbloom_*_device, ntc_bloom_insert_solid_device; DESIGN.md §4 "Counting
// filters and solid k-mers").  m unsigned 8-bit counters, counter loc = byte loc, the array padded to a multiple of 4 bytes whose padding stays 0.  A
// k-mer's n_hash positions are the plain filter's (ntc_bloom_walk.hpp: h_i % m); an insert adds one to each, saturating at 255, so that after any inserts
// in any order counter[loc] = min(255, increments aimed at loc) — no conservative update, whose result would depend on the order of concurrent inserts.
// The count of a k-mer is the minimum of its counters.  The walk over the input, the insert action and the kernels over given h_0 values are
// ntc_bloom_walk.hpp's templates over a filter's view: here are the counting filter's view (CountersView), the counting kind's own actions (count >= c,
// count, "count >= c -> insert into a plain or a blocked filter") and the streaming kernels over the counters (threshold, add, hist).
#include "ntc_bbloom.hpp"

using namespace ntc_eng;
using namespace ntc_bloom;

namespace {

// counter loc += 1, saturating.  A PLAIN load of the dword first: a byte that reads 255 needs nothing.  Counters only rise, so a stale value can only read
// LOWER than the truth — then the compare-and-swap, which fails on a stale dword and returns the fresh one, decides.  The loop re-reads the byte, leaves at
// 255 and adds 1 << 8 (loc & 3): never a carry into the neighbour, which an unconditional add on the dword would produce at 255.
__device__ __forceinline__ void cbloom_inc(uint32_t* counters, uint64_t loc)
{
	uint32_t* w = counters + (loc >> 2);
	const uint32_t sh = 8u * (uint32_t)(loc & 3u);
	uint32_t old = *w;
	while (((old >> sh) & 0xffu) != 0xffu) {
		if (__hip_atomic_compare_exchange_strong(w, &old, old + (1u << sh), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
	}
}
__device__ __forceinline__ void cbloom_insert(uint32_t* counters, const BloomHashes& hs, uint64_t h0)
{
	for (uint32_t i = 0; i < hs.n_hash; ++i)
		cbloom_inc(counters, hs.loc(h0, i)); // (two equal positions of one k-mer: two increments)
}
// min(the k-mer's counters), left as soon as one is below `floor` (the value returned is then some counter below floor, not the minimum)
__device__ __forceinline__ uint32_t cbloom_count(const unsigned char* counters, const BloomHashes& hs, uint64_t h0, uint32_t floor)
{
	uint32_t c = 255u;
	for (uint32_t i = 0; i < hs.n_hash; ++i) {
		const uint32_t v = counters[hs.loc(h0, i)];
		c = v < c ? v : c;
		if (c < floor) break;
	}
	return c;
}

// the view of a counting filter
struct CountersView {
	uint32_t* counters;
	BloomHashes hs;
	__device__ __forceinline__ void insert(uint64_t h0) const { cbloom_insert(counters, hs, h0); }
	__device__ __forceinline__ uint32_t count(uint64_t h0, uint32_t floor) const { return cbloom_count(reinterpret_cast<const unsigned char*>(counters), hs, h0, floor); }
	__device__ __forceinline__ unsigned char answer(uint64_t h0) const { return (unsigned char)count(h0, 0u); }
};
CountersView counters_view(const void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k)
{
	return CountersView{static_cast<uint32_t*>(const_cast<void*>(d_counters)), bloom_hashes(m, n_hash, k)};
}

// the counting kind's own actions
struct AtLeastAct {
	static constexpr int kMode = kWalkPerSeq;
	const unsigned char* counters;
	BloomHashes hs;
	uint32_t min_count;
	__device__ __forceinline__ uint32_t operator()(uint64_t h0) const { return cbloom_count(counters, hs, h0, min_count) >= min_count ? 1u : 0u; }
};
struct CountAct {
	static constexpr int kMode = kWalkProfile;
	const unsigned char* counters;
	BloomHashes hs;
	__device__ __forceinline__ uint32_t operator()(uint64_t h0) const { return cbloom_count(counters, hs, h0, 0u); }
};
// the second stage: a window whose count in a FINISHED counting filter is >= min_count is inserted into a filter of its own kind, size and hash count —
// `Dst` is that filter's view: plain (BitsView) or blocked (BlockedView: one line of the destination per window that passed)
template <class Dst> struct SolidAct {
	static constexpr int kMode = kWalkTotal;
	const unsigned char* counters;
	BloomHashes chs;
	uint32_t min_count;
	Dst dst;
	__device__ __forceinline__ uint32_t operator()(uint64_t h0) const
	{
		if (cbloom_count(counters, chs, h0, min_count) < min_count) return 0u;
		dst.insert(h0);
		return 1u;
	}
};

// dword i of the plain filter = the positions 32 i .. 32 i + 31: a lane reads their 32 counters — two 16-byte loads where the array is 16-byte aligned
// and holds all 32, else the dwords that exist (n_dwords = the padded array's) — and writes the dword.  The padding counters are 0 and min_count >= 1: no
// bit from m on is set.
__global__ __launch_bounds__(256) void cbloom_threshold_kernel(const uint32_t* __restrict__ counters, uint64_t n_dwords, uint32_t wide, uint32_t min_count,
                                                               uint32_t* __restrict__ filter, uint64_t n_words)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256u) {
		uint32_t c[8];
		if (wide && 8u * i + 8u <= n_dwords) {
			const uint4 lo = reinterpret_cast<const uint4*>(counters)[2u * i], hi = reinterpret_cast<const uint4*>(counters)[2u * i + 1u];
			c[0] = lo.x, c[1] = lo.y, c[2] = lo.z, c[3] = lo.w, c[4] = hi.x, c[5] = hi.y, c[6] = hi.z, c[7] = hi.w;
		} else {
#pragma unroll
			for (uint32_t d = 0; d < 8; ++d)
				c[d] = 8u * i + d < n_dwords ? counters[8u * i + d] : 0u;
		}
		uint32_t word = 0;
#pragma unroll
		for (uint32_t j = 0; j < 32; ++j) // position 32 i + j: bit 7 - j % 8 of byte j / 8 of the dword
			word |= ((c[j >> 2] >> (8u * (j & 3u))) & 0xffu) >= min_count ? bloom_bit(j) : 0u;
		filter[i] = word;
	}
}

__device__ __forceinline__ uint32_t sat_add4(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
#pragma unroll
	for (uint32_t t = 0; t < 4; ++t) {
		const uint32_t s = ((a >> (8u * t)) & 0xffu) + ((b >> (8u * t)) & 0xffu);
		r |= (s > 255u ? 255u : s) << (8u * t);
	}
	return r;
}
__global__ __launch_bounds__(256) void cbloom_add_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint64_t n_dwords)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_dwords; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t s = src[i];
		if (s) dst[i] = sat_add4(dst[i], s);
	}
}

// out[v] += the counters of value v among the first m, out[256] += the non-zero bytes behind them.  One histogram per wave in LDS (a workgroup sees fewer
// than 2^32 counters: m < 2^40 over up to 4096 workgroups), one global add per used bin and workgroup.  The values 0 and 1 — most of a filter that is
// sized for its input — are counted in registers: 64 lanes adding to one LDS word are served one after the other.
__global__ __launch_bounds__(256) void cbloom_hist_kernel(const uint32_t* __restrict__ counters, uint64_t n_dwords, uint64_t m, unsigned long long* out)
{
	__shared__ uint32_t h[4][256];
	for (uint32_t s = threadIdx.x; s < 1024u; s += 256u)
		(&h[0][0])[s] = 0;
	__syncthreads();
	uint32_t* mine = h[threadIdx.x >> 6];
	uint32_t pad = 0, n0 = 0, n1 = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_dwords; i += (uint64_t)gridDim.x * 256u) {
		const uint32_t w = counters[i];
		const uint32_t inside = 4u * i + 4u <= m ? 4u : (uint32_t)(m - 4u * i); // (the last dword: bytes from m on are padding)
		if (w == 0) {
			n0 += inside;
			continue;
		}
#pragma unroll
		for (uint32_t t = 0; t < 4; ++t) {
			const uint32_t v = (w >> (8u * t)) & 0xffu;
			if (t >= inside)
				pad += v ? 1u : 0u;
			else if (v == 0)
				++n0;
			else if (v == 1u)
				++n1;
			else
				atomicAdd(&mine[v], 1u);
		}
	}
	if (n0) atomicAdd(&mine[0], n0);
	if (n1) atomicAdd(&mine[1], n1);
	__syncthreads();
	const uint32_t sum = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
	if (sum) atomicAdd(&out[threadIdx.x], (unsigned long long)sum);
	if (pad) atomicAdd(&out[256], (unsigned long long)pad);
}

uint64_t counter_dwords(uint64_t m) { return (m + 3u) / 4u; }

int check_counters(const char* who, const void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k) { return check_filter(who, d_counters, m, n_hash, k, "m", "counter array"); }
int check_min_count(const char* who, uint32_t min_count)
{
	if (min_count < 1 || min_count > 255) return fail(NTC_ERR_ARG, "%s: min_count=%u outside 1..255", who, min_count);
	return 0;
}

} // namespace

extern "C" {

int ntc_cbloom_insert_device(int32_t device, void* stream, void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                             const uint64_t* offsets, uint64_t n_seqs, uint64_t* n_windows)
{
	if (int rc = check_counters("ntc_cbloom_insert_device", d_counters, m, n_hash, k)) return rc;
	if (int rc = check_input("ntc_cbloom_insert_device", strand, d_bases, offsets, n_seqs)) return rc;
	const InsertAct<CountersView> act{counters_view(d_counters, m, n_hash, k)};
	return walk_total("ntc_cbloom_insert_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, n_windows);
}

int ntc_cbloom_query_device(int32_t device, void* stream, const void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                            const uint64_t* offsets, uint64_t n_seqs, uint32_t min_count, void* d_windows_u32, void* d_hits_u32)
{
	if (int rc = check_counters("ntc_cbloom_query_device", d_counters, m, n_hash, k)) return rc;
	if (int rc = check_min_count("ntc_cbloom_query_device", min_count)) return rc;
	if (int rc = check_input("ntc_cbloom_query_device", strand, d_bases, offsets, n_seqs)) return rc;
	const AtLeastAct act{static_cast<const unsigned char*>(d_counters), bloom_hashes(m, n_hash, k), min_count};
	return walk_per_seq("ntc_cbloom_query_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, d_windows_u32, d_hits_u32);
}

int ntc_cbloom_profile_device(int32_t device, void* stream, const void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand, const void* d_bases,
                              const uint64_t* offsets, uint64_t n_seqs, void* d_counts_u8)
{
	if (int rc = check_counters("ntc_cbloom_profile_device", d_counters, m, n_hash, k)) return rc;
	if (int rc = check_input("ntc_cbloom_profile_device", strand, d_bases, offsets, n_seqs)) return rc;
	const CountAct act{static_cast<const unsigned char*>(d_counters), bloom_hashes(m, n_hash, k)};
	return walk_profile("ntc_cbloom_profile_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, d_counts_u8);
}

int ntc_cbloom_insert_hashes_device(int32_t device, void* stream, void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n)
{
	if (int rc = check_counters("ntc_cbloom_insert_hashes_device", d_counters, m, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_cbloom_insert_hashes_device", d_h0_u64, n)) return rc;
	if (n == 0) return 0;
	return launch_strided(device, stream, insert_hashes_kernel<CountersView>, n, counters_view(d_counters, m, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n);
}

int ntc_cbloom_query_hashes_device(int32_t device, void* stream, const void* d_counters, uint64_t m, uint32_t n_hash, uint32_t k, const void* d_h0_u64, uint64_t n,
                                   void* d_counts_u8)
{
	if (int rc = check_counters("ntc_cbloom_query_hashes_device", d_counters, m, n_hash, k)) return rc;
	if (int rc = check_hashes("ntc_cbloom_query_hashes_device", d_h0_u64, n, "hashes or counts", d_counts_u8 != nullptr)) return rc;
	if (n == 0) return 0;
	return launch_strided(device, stream, query_hashes_kernel<CountersView>, n, counters_view(d_counters, m, n_hash, k), static_cast<const uint64_t*>(d_h0_u64), n,
	                      static_cast<unsigned char*>(d_counts_u8));
}

int ntc_cbloom_threshold_device(int32_t device, void* stream, const void* d_counters, uint64_t m, uint32_t min_count, void* d_filter)
{
	if (int rc = check_counters("ntc_cbloom_threshold_device", d_counters, m, 1, 1)) return rc;
	if (int rc = check_min_count("ntc_cbloom_threshold_device", min_count)) return rc;
	if (int rc = check_filter("ntc_cbloom_threshold_device", d_filter, m, 1, 1)) return rc;
	const uint64_t n_words = filter_words(m);
	return launch_strided(device, stream, cbloom_threshold_kernel, n_words, static_cast<const uint32_t*>(d_counters), counter_dwords(m),
	                      ((uintptr_t)d_counters & 15u) == 0 ? 1u : 0u, min_count, static_cast<uint32_t*>(d_filter), n_words);
}

int ntc_bloom_insert_solid_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, const void* d_counters, uint64_t m, uint32_t c_n_hash,
                                  uint32_t min_count, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t* n_windows)
{
	if (int rc = check_filter("ntc_bloom_insert_solid_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_counters("ntc_bloom_insert_solid_device", d_counters, m, c_n_hash, k)) return rc;
	if (int rc = check_min_count("ntc_bloom_insert_solid_device", min_count)) return rc;
	if (int rc = check_input("ntc_bloom_insert_solid_device", strand, d_bases, offsets, n_seqs)) return rc;
	const SolidAct<BitsView> act{static_cast<const unsigned char*>(d_counters), bloom_hashes(m, c_n_hash, k), min_count, bits_view(d_filter, m_bits, n_hash, k)};
	return walk_total("ntc_bloom_insert_solid_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, n_windows);
}

int ntc_bbloom_insert_solid_device(int32_t device, void* stream, void* d_filter, uint64_t m_bits, uint32_t n_hash, const void* d_counters, uint64_t m, uint32_t c_n_hash,
                                   uint32_t min_count, uint32_t k, uint32_t strand, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint64_t* n_windows)
{
	if (int rc = check_blocked("ntc_bbloom_insert_solid_device", d_filter, m_bits, n_hash, k)) return rc;
	if (int rc = check_counters("ntc_bbloom_insert_solid_device", d_counters, m, c_n_hash, k)) return rc;
	if (int rc = check_min_count("ntc_bbloom_insert_solid_device", min_count)) return rc;
	if (int rc = check_input("ntc_bbloom_insert_solid_device", strand, d_bases, offsets, n_seqs)) return rc;
	const SolidAct<BlockedView> act{static_cast<const unsigned char*>(d_counters), bloom_hashes(m, c_n_hash, k), min_count, blocked_view(d_filter, m_bits, n_hash, k)};
	return walk_total("ntc_bbloom_insert_solid_device", device, stream, act, k, strand, d_bases, offsets, n_seqs, n_windows);
}

int ntc_cbloom_add_device(int32_t device, void* stream, void* d_dst, const void* d_src, uint64_t m)
{
	if (int rc = check_counters("ntc_cbloom_add_device", d_dst, m, 1, 1)) return rc;
	if (int rc = check_counters("ntc_cbloom_add_device", d_src, m, 1, 1)) return rc;
	if (d_dst == d_src) return fail(NTC_ERR_ARG, "ntc_cbloom_add_device: dst and src are the same array");
	const uint64_t n_dwords = counter_dwords(m);
	return launch_strided(device, stream, cbloom_add_kernel, n_dwords, static_cast<uint32_t*>(d_dst), static_cast<const uint32_t*>(d_src), n_dwords);
}

int ntc_cbloom_hist_device(int32_t device, void* stream, const void* d_counters, uint64_t m, uint64_t* hist_u64)
{
	if (int rc = check_counters("ntc_cbloom_hist_device", d_counters, m, 1, 1)) return rc;
	if (!hist_u64) return fail(NTC_ERR_ARG, "ntc_cbloom_hist_device: null hist");
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf<unsigned long long> d_out; // (scratch of this call: freed on every way out)
	if (!d_out.reserve(257 * 8)) return fail(NTC_ERR_MEMORY, "ntc_cbloom_hist_device: cannot allocate %d B of scratch on device", 257 * 8);
	HIP_TRY(hipMemsetAsync(d_out, 0, 257 * 8, st));
	const uint64_t n_dwords = counter_dwords(m);
	hipLaunchKernelGGL(cbloom_hist_kernel, dim3(stride_grid(n_dwords)), dim3(256), 0, st, static_cast<const uint32_t*>(d_counters), n_dwords, m, d_out.get());
	HIP_TRY(hipGetLastError());
	unsigned long long out[257];
	HIP_TRY(hipMemcpyAsync(out, d_out, 257 * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (out[256] != 0) return fail(NTC_ERR_STATE, "ntc_cbloom_hist_device: %llu bytes behind the filter's m=%llu counters are not 0", out[256], (unsigned long long)m);
	for (int v = 0; v < 256; ++v)
		hist_u64[v] = out[v];
	return 0;
}

} // extern "C"
