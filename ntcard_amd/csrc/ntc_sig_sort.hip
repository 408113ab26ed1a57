// ntc_sig_sort.hip — signatures on the device behind the container: a stable radix sort of (u64 key, u32 value) pairs (include/ntcard_hip.h:
// ntc_signature_sort_device; DESIGN.md §4 "Signatures", "Sort and compare").  ntc_signature / ntc_signature_device sort their compaction with sig_sort()
// below; the intersections of sorted lists are in ntc_sig_lists.hip.
//
// The sort is LSD, 8 bits per digit, eight digits.  A workgroup of four waves takes a TILE of 4096 pairs, wave w the 1024 pairs [1024 w, 1024 w + 1024) of it in
// 16 rounds of 64 (a lane and round = one pair, a wave's load = 512 contiguous bytes), so the order of the pairs is (tile, wave, round, lane).
//   hist     one launch: the histograms of ALL eight digits (LDS counters per workgroup, added to 8 x 256 global ones).  The host reads them: a digit in which
//            one bin holds every key moves nothing and is skipped — all of them for equal keys, most for keys that differ in a few bytes; a signature's
//            top digit keeps two or three live bins (the two patterns of ntComp) and is not skipped.
//   per digit that is left, three launches:
//   count    a workgroup per tile: how many of its keys fall into each bin, to table[bin][tile]
//   scan     a workgroup per bin: the exclusive prefix sums of its row, from the bin's base (the bins below it, out of the global histogram) — the table then
//            holds the position of the first key of every (bin, tile)
//   scatter  a workgroup per tile: per-wave bin counts in LDS, turned into the first position of every (wave, bin); then, round by round, a key's position =
//            its wave's counter of its bin + the lanes below it that hold the same digit (eight ballots), and the lowest such lane moves the counter on.
//            Equal digits keep their order at every step, so the sort is stable.
// n <= 4096: ONE launch of one workgroup — the pairs stay in registers, the same ranking runs digit by digit (a digit all keys agree in is skipped there as
// well), and LDS holds the counters and one copy of the pairs to permute them through.
// No kernel waits on another workgroup; a launch reads what an earlier launch wrote.  Vector stores and plain C++ only.
#include "ntc_sig_device.hpp"

namespace ntc {

namespace {

constexpr uint32_t kSortBits = 8, kSortBins = 1u << kSortBits, kSortDigits = 64u / kSortBits;
constexpr uint32_t kSortWaves = 4, kSortThreads = 64u * kSortWaves, kSortRounds = 16;
constexpr uint32_t kSortWaveItems = 64u * kSortRounds;          // 1024 pairs per wave
constexpr uint32_t kSortTile = kSortWaves * kSortWaveItems;     // 4096 pairs per workgroup
constexpr uint32_t kSortSmall = kSortTile;                      // up to here: one launch
static_assert(kSortThreads == kSortBins, "a thread per bin");

__device__ __forceinline__ uint32_t digit_of(unsigned long long k, uint32_t shift) { return (uint32_t)(k >> shift) & (kSortBins - 1u); }

// (hist_add — one add for the lanes that hold the first lane's digit — and block_scan are in ntc_sig_device.hpp: the set algebra uses them too)

// a key's position: the counter of its digit in its wave's row + the valid lanes below it with the same digit; the lowest of them moves the counter past all
// of them.  Whole waves call this; the row is the calling wave's alone (its lanes read it in one instruction and one lane per digit writes it in a later one)
__device__ __forceinline__ uint32_t wave_rank(volatile uint32_t* row, uint32_t d, bool valid)
{
	uint64_t m = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
	for (uint32_t b = 0; b < kSortBits; ++b) {
		const bool bit = ((d >> b) & 1u) != 0u;
		const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
		m &= bit ? bal : ~bal;
	}
	const uint32_t below = lanes_below(m);
	const uint32_t old = valid ? row[d] : 0u;
	__builtin_amdgcn_wave_barrier();
	if (valid && below == 0u) row[d] = old + (uint32_t)__popcll(m);
	__builtin_amdgcn_wave_barrier();
	return old + below;
}

static_assert(kSortWaves == 4 && kSortThreads == 256, "block_scan (ntc_sig_device.hpp) scans a workgroup of four waves");

__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const unsigned long long* __restrict__ keys, uint64_t n, uint32_t* __restrict__ ghist)
{
	__shared__ uint32_t h[kSortDigits * kSortBins];
	for (uint32_t i = threadIdx.x; i < kSortDigits * kSortBins; i += kSortThreads)
		h[i] = 0u;
	__syncthreads();
	const uint64_t step = (uint64_t)gridDim.x * kSortThreads;
	const uint64_t rounds = (n + step - 1) / step; // every wave runs the same number of rounds: hist_add sees whole waves
	for (uint64_t r = 0, i = (uint64_t)blockIdx.x * kSortThreads + threadIdx.x; r < rounds; ++r, i += step) {
		const bool valid = i < n;
		const unsigned long long k = valid ? keys[i] : 0ull;
#pragma unroll
		for (uint32_t p = 0; p < kSortDigits; ++p)
			hist_add(h + p * kSortBins, digit_of(k, p * kSortBits), valid);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kSortDigits * kSortBins; i += kSortThreads)
		if (h[i]) atomicAdd(ghist + i, h[i]);
}

__global__ __launch_bounds__(kSortThreads) void sort_count_kernel(const unsigned long long* __restrict__ keys, uint64_t n, uint32_t shift, uint32_t* __restrict__ table,
                                                                  uint64_t tiles)
{
	__shared__ uint32_t h[kSortBins];
	h[threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t base = (uint64_t)blockIdx.x * kSortTile + threadIdx.x;
#pragma unroll 4
	for (uint32_t r = 0; r < kSortTile / kSortThreads; ++r) {
		const uint64_t i = base + (uint64_t)r * kSortThreads;
		const bool valid = i < n;
		hist_add(h, digit_of(valid ? keys[i] : 0ull, shift), valid);
	}
	__syncthreads();
	table[(uint64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// workgroup d: row d of the table becomes its exclusive prefix sums, from the keys of the bins below d (fewer than 2^32 keys in all: 32-bit positions)
__global__ __launch_bounds__(kSortThreads) void sort_scan_kernel(const uint32_t* __restrict__ ghist, uint32_t* __restrict__ table, uint64_t tiles)
{
	__shared__ uint32_t wsum[kSortWaves];
	const uint32_t d = blockIdx.x;
	uint32_t carry = 0, total = 0;
	(void)block_scan(threadIdx.x < d ? ghist[threadIdx.x] : 0u, wsum, carry);
	uint32_t* row = table + (uint64_t)d * tiles;
	for (uint64_t t0 = 0; t0 < tiles; t0 += kSortThreads) {
		const uint64_t t = t0 + threadIdx.x;
		const uint32_t v = t < tiles ? row[t] : 0u;
		const uint32_t ex = block_scan(v, wsum, total);
		if (t < tiles) row[t] = carry + ex;
		carry += total;
	}
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const unsigned long long* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                                    unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ vals_out, uint64_t n, uint32_t shift,
                                                                    const uint32_t* __restrict__ table, uint64_t tiles)
{
	__shared__ uint32_t cnt[kSortWaves][kSortBins];
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
	for (uint32_t w = 0; w < kSortWaves; ++w)
		cnt[w][threadIdx.x] = 0u;
	const uint64_t base = (uint64_t)blockIdx.x * kSortTile + (uint64_t)wave * kSortWaveItems + lane;
	unsigned long long k[kSortRounds];
	uint32_t v[kSortRounds];
#pragma unroll
	for (uint32_t r = 0; r < kSortRounds; ++r) {
		const uint64_t i = base + r * 64u;
		k[r] = i < n ? keys_in[i] : 0ull;
		v[r] = (vals_in && i < n) ? vals_in[i] : 0u;
	}
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < kSortRounds; ++r)
		hist_add(cnt[wave], digit_of(k[r], shift), base + r * 64u < n);
	__syncthreads();
	{ // thread d: the counts of bin d, wave by wave, become the position of each wave's first key of the bin
		uint32_t run = table[(uint64_t)threadIdx.x * tiles + blockIdx.x];
#pragma unroll
		for (uint32_t w = 0; w < kSortWaves; ++w) {
			const uint32_t c = cnt[w][threadIdx.x];
			cnt[w][threadIdx.x] = run;
			run += c;
		}
	}
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < kSortRounds; ++r) {
		const bool valid = base + r * 64u < n;
		const uint32_t at = wave_rank(cnt[wave], digit_of(k[r], shift), valid); // (< n: the table counted these very keys)
		if (valid) {
			keys_out[at] = k[r];
			if (vals_in) vals_out[at] = v[r];
		}
	}
}

// n <= kSortSmall pairs, one workgroup, in place.  Wave w holds the pairs [w C, w C + C), C = 64 x rounds, rounds = ceil(n / 256), in registers
__global__ __launch_bounds__(kSortThreads) void sort_small_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t n)
{
	__shared__ unsigned long long kbuf[kSortSmall];
	__shared__ uint32_t vbuf[kSortSmall];
	__shared__ uint32_t cnt[kSortWaves][kSortBins];
	__shared__ uint32_t wsum[kSortWaves];
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t rounds = (n + kSortThreads - 1u) / kSortThreads; // <= kSortRounds
	const uint32_t base = wave * rounds * 64u + lane;
	unsigned long long k[kSortRounds];
	uint32_t v[kSortRounds];
#pragma unroll
	for (uint32_t r = 0; r < kSortRounds; ++r) {
		const uint32_t i = base + r * 64u;
		const bool valid = r < rounds && i < n;
		k[r] = valid ? keys[i] : 0ull;
		v[r] = (vals && valid) ? vals[i] : 0u;
	}
	for (uint32_t shift = 0; shift < 64u; shift += kSortBits) {
#pragma unroll
		for (uint32_t w = 0; w < kSortWaves; ++w)
			cnt[w][threadIdx.x] = 0u;
		__syncthreads();
#pragma unroll
		for (uint32_t r = 0; r < kSortRounds; ++r)
			if (r < rounds) hist_add(cnt[wave], digit_of(k[r], shift), base + r * 64u < n);
		__syncthreads();
		uint32_t c[kSortWaves], tot = 0;
#pragma unroll
		for (uint32_t w = 0; w < kSortWaves; ++w) {
			c[w] = cnt[w][threadIdx.x];
			tot += c[w];
		}
		if (__syncthreads_or(tot == n)) continue; // every key in one bin: this digit moves nothing
		uint32_t total = 0;
		uint32_t run = block_scan(tot, wsum, total);
#pragma unroll
		for (uint32_t w = 0; w < kSortWaves; ++w) {
			cnt[w][threadIdx.x] = run;
			run += c[w];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t r = 0; r < kSortRounds; ++r) {
			if (r < rounds) {
				const bool valid = base + r * 64u < n;
				const uint32_t at = wave_rank(cnt[wave], digit_of(k[r], shift), valid); // (< n <= kSortSmall)
				if (valid) {
					kbuf[at] = k[r];
					vbuf[at] = v[r];
				}
			}
		}
		__syncthreads();
#pragma unroll
		for (uint32_t r = 0; r < kSortRounds; ++r) {
			const uint32_t i = base + r * 64u;
			if (r < rounds && i < n) {
				k[r] = kbuf[i];
				v[r] = vbuf[i];
			}
		}
		__syncthreads();
	}
#pragma unroll
	for (uint32_t r = 0; r < kSortRounds; ++r) {
		const uint32_t i = base + r * 64u;
		if (r < rounds && i < n) {
			keys[i] = k[r];
			if (vals) vals[i] = v[r];
		}
	}
}

} // namespace

uint64_t sig_sort_one_launch() { return kSortSmall; }

// [8 x 256 digit histograms][256 x tiles table]
size_t sig_sort_aux_bytes(uint64_t n)
{
	if (n <= kSortSmall) return 0;
	const uint64_t tiles = (n + kSortTile - 1) / kSortTile;
	return (size_t)(kSortDigits * kSortBins + kSortBins * tiles) * 4u;
}

hipError_t sig_sort(unsigned long long* keys, uint32_t* vals, unsigned long long* alt_keys, uint32_t* alt_vals, uint64_t n, void* aux, hipStream_t st, bool* in_alt)
{
	*in_alt = false;
	if (n < 2) return hipSuccess;
	if (n >> 32) return hipErrorInvalidValue;
	if (n <= kSortSmall) {
		hipLaunchKernelGGL(sort_small_kernel, dim3(1), dim3(kSortThreads), 0, st, keys, vals, (uint32_t)n);
		return hipGetLastError();
	}
	const uint64_t tiles = (n + kSortTile - 1) / kSortTile; // < 2^20
	uint32_t* ghist = static_cast<uint32_t*>(aux);
	uint32_t* table = ghist + kSortDigits * kSortBins;
	hipError_t rc = hipMemsetAsync(ghist, 0, kSortDigits * kSortBins * 4u, st);
	if (rc != hipSuccess) return rc;
	hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)std::min<uint64_t>(tiles, 2048)), dim3(kSortThreads), 0, st, keys, n, ghist);
	if ((rc = hipGetLastError()) != hipSuccess) return rc;
	std::vector<uint32_t> h(kSortDigits * kSortBins);
	if ((rc = hipMemcpyAsync(h.data(), ghist, h.size() * 4u, hipMemcpyDeviceToHost, st)) != hipSuccess) return rc;
	if ((rc = hipStreamSynchronize(st)) != hipSuccess) return rc;
	unsigned long long* ks[2] = {keys, alt_keys};
	uint32_t* vs[2] = {vals, vals ? alt_vals : nullptr};
	uint32_t cur = 0;
	for (uint32_t p = 0; p < kSortDigits; ++p) {
		const uint32_t* hp = h.data() + p * kSortBins;
		if (std::find(hp, hp + kSortBins, (uint32_t)n) != hp + kSortBins) continue; // one bin holds every key
		const uint32_t shift = p * kSortBits;
		hipLaunchKernelGGL(sort_count_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, st, ks[cur], n, shift, table, tiles);
		hipLaunchKernelGGL(sort_scan_kernel, dim3(kSortBins), dim3(kSortThreads), 0, st, ghist + p * kSortBins, table, tiles);
		hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, st, ks[cur], vs[cur], ks[cur ^ 1u], vs[cur ^ 1u], n, shift, table, tiles);
		if ((rc = hipGetLastError()) != hipSuccess) return rc;
		cur ^= 1u;
	}
	*in_alt = cur != 0;
	return hipSuccess;
}

} // namespace ntc

using namespace ntc_eng;

extern "C" {

int ntc_signature_sort_device(int32_t device, void* stream, void* d_keys_u64, void* d_vals_u32, uint64_t n)
{
	if (!d_keys_u64 && n) return fail(NTC_ERR_ARG, "ntc_signature_sort_device: null key array");
	if (n >> 32) return fail(NTC_ERR_ARG, "ntc_signature_sort_device: %llu pairs (fewer than 2^32 are sorted)", (unsigned long long)n);
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	unsigned long long* keys = (unsigned long long*)d_keys_u64;
	uint32_t* vals = (uint32_t*)d_vals_u32;
	DevBuf<unsigned long long> alt_k; // (scratch of this call: freed on every way out)
	DevBuf<uint32_t> alt_v;
	DevBuf<unsigned char> aux;
	if (n > ntc::sig_sort_one_launch() && (!alt_k.reserve(n * 8) || (vals && !alt_v.reserve(n * 4)) || !aux.reserve(ntc::sig_sort_aux_bytes(n)))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_sort_device: cannot allocate %llu B of scratch on device; nothing was changed",
		            (unsigned long long)(n * (vals ? 12 : 8) + ntc::sig_sort_aux_bytes(n)));
	}
	bool in_alt = false;
	HIP_TRY(ntc::sig_sort(keys, vals, alt_k, alt_v, n, aux.get(), st, &in_alt));
	if (in_alt) {
		HIP_TRY(hipMemcpyAsync(keys, alt_k, n * 8, hipMemcpyDeviceToDevice, st));
		if (vals) HIP_TRY(hipMemcpyAsync(vals, alt_v, n * 4, hipMemcpyDeviceToDevice, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

} // extern "C"
