// ntc_sig_sort.hip — signatures on the device behind the container: a stable radix sort of (u64 key, u32 value) pairs, the intersection of two sorted lists
// and of all pairs of many (include/ntcard_hip.h: ntc_signature_sort_device, ntc_signature_compare_device, ntc_signature_matrix_device; DESIGN.md §4
// "Signatures", "Sort and compare").  ntc_signature / ntc_signature_device sort their compaction with sig_sort() below.
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
#include "ntc_engine.hpp"

namespace ntc {

namespace {

constexpr uint32_t kSortBits = 8, kSortBins = 1u << kSortBits, kSortDigits = 64u / kSortBits;
constexpr uint32_t kSortWaves = 4, kSortThreads = 64u * kSortWaves, kSortRounds = 16;
constexpr uint32_t kSortWaveItems = 64u * kSortRounds;          // 1024 pairs per wave
constexpr uint32_t kSortTile = kSortWaves * kSortWaveItems;     // 4096 pairs per workgroup
constexpr uint32_t kSortSmall = kSortTile;                      // up to here: one launch
static_assert(kSortThreads == kSortBins, "a thread per bin");

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

__device__ __forceinline__ uint32_t digit_of(unsigned long long k, uint32_t shift) { return (uint32_t)(k >> shift) & (kSortBins - 1u); }

// h[d] += 1 for every valid lane (whole waves call this).  The lanes that hold the first lane's digit send one add: a digit most keys agree in — a signature's top
// bits, a nearly full bin — is not 64 adds to one LDS address
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

// exclusive prefix sum of v over the workgroup's 256 threads; total = the sum.  wsum: kSortWaves words of LDS, free again on return
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
	for (uint32_t w = 0; w < kSortWaves; ++w) {
		const uint32_t s = wsum[w];
		pre += w < wave ? s : 0u;
		total += s;
	}
	__syncthreads();
	return pre + inc - v;
}

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

// ---- intersections ----
constexpr uint32_t kMatChunk = 4096;     // entries of a pair's shorter list per work item (a workgroup)
constexpr uint32_t kMatItems = 1u << 18; // work items per launch: the scratch that holds them is 4 MiB whatever the number of pairs
constexpr unsigned long long kNoBad = ~0ull;

struct MatItem {
	uint32_t i, j;  // the pair, i < j
	uint64_t start; // first entry of the shorter list
};

// the first index >= x of the ascending list l[0 .. n) (any list: the search stays inside [0, n])
__device__ __forceinline__ uint64_t lower_bound(const unsigned long long* __restrict__ l, uint64_t n, unsigned long long x)
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
		const uint64_t at = lower_bound(l, nl, x);
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
		const uint64_t at = lower_bound(l, n_l, x);
		hits += (at < n_l && l[at] == x) ? 1u : 0u;
	}
	hits = wave_sum(hits);
	if ((threadIdx.x & 63u) == 0u && hits) atomicAdd(counts + (uint64_t)it.i * n_sigs + it.j, hits);
}

unsigned ascent_blocks(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 1024)); }

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

int ntc_signature_compare_device(int32_t device, void* stream, const void* d_a_u64, const void* d_ca_u32, uint64_t na, const void* d_b_u64, const void* d_cb_u32,
                                 uint64_t nb, uint64_t* n_common, uint64_t* min_sum)
{
	if (!n_common || (!d_a_u64 && na) || (!d_b_u64 && nb)) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: null argument");
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	const bool weigh = d_ca_u32 && d_cb_u32 && min_sum;
	// device words: the two lists, their lengths, the first bad entry of each, the hits, the sum
	unsigned long long w[8] = {(unsigned long long)(uintptr_t)d_a_u64, (unsigned long long)(uintptr_t)d_b_u64, na, nb, ntc::kNoBad, ntc::kNoBad, 0ull, 0ull};
	DevBuf<unsigned long long> d_w;
	if (!d_w.reserve(sizeof w)) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_compare_device: cannot allocate %zu B on device", sizeof w);
	}
	HIP_TRY(hipMemcpyAsync(d_w, w, sizeof w, hipMemcpyHostToDevice, st));
	if (na > 1 || nb > 1)
		hipLaunchKernelGGL(ntc::sig_ascent_kernel, dim3(ntc::ascent_blocks(std::max(na, nb)), 2), dim3(256), 0, st, (const unsigned long long* const*)d_w.get(),
		                   (const uint64_t*)(d_w.get() + 2), d_w.get() + 4);
	if (na && nb) {
		const bool a_short = na <= nb;
		const uint64_t n_s = a_short ? na : nb;
		const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_s + 255) / 256, 8192));
		hipLaunchKernelGGL(ntc::sig_compare_kernel, dim3(grid), dim3(256), 0, st, (const unsigned long long*)(a_short ? d_a_u64 : d_b_u64),
		                   weigh ? (const uint32_t*)(a_short ? d_ca_u32 : d_cb_u32) : nullptr, n_s, (const unsigned long long*)(a_short ? d_b_u64 : d_a_u64),
		                   weigh ? (const uint32_t*)(a_short ? d_cb_u32 : d_ca_u32) : nullptr, a_short ? nb : na, d_w.get() + 6);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(w, d_w, sizeof w, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (w[4] != ntc::kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: the first list is not strictly ascending at entry %llu", w[4]);
	if (w[5] != ntc::kNoBad) return fail(NTC_ERR_ARG, "ntc_signature_compare_device: the second list is not strictly ascending at entry %llu", w[5]);
	*n_common = w[6];
	if (weigh) *min_sum = w[7];
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
	// device words: [lists][lengths][first bad entry of each list][counts of the pairs, n_sigs x n_sigs], then the work items of a round
	DevBuf<unsigned long long> d_w;
	DevBuf<ntc::MatItem> d_items;
	if (!d_w.reserve((3 * ns + cells) * 8) || !d_items.reserve((size_t)ntc::kMatItems * sizeof(ntc::MatItem))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "ntc_signature_matrix_device: cannot allocate %zu B of scratch on device", (3 * ns + cells) * 8 + (size_t)ntc::kMatItems * sizeof(ntc::MatItem));
	}
	std::vector<unsigned long long> w(3 * ns, ntc::kNoBad);
	uint64_t longest = 0;
	for (size_t i = 0; i < ns; ++i) {
		w[i] = (unsigned long long)(uintptr_t)d_hashes_u64[i];
		w[ns + i] = n[i];
		longest = std::max<uint64_t>(longest, n[i]);
	}
	HIP_TRY(hipMemcpyAsync(d_w, w.data(), w.size() * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_w.get() + 3 * ns, 0, cells * 8, st));
	const unsigned long long* const* d_lists = (const unsigned long long* const*)d_w.get();
	const uint64_t* d_ns = (const uint64_t*)(d_w.get() + ns);
	if (longest > 1) {
		hipLaunchKernelGGL(ntc::sig_ascent_kernel, dim3(ntc::ascent_blocks(longest), n_sigs), dim3(256), 0, st, d_lists, d_ns, d_w.get() + 2 * ns);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(w.data() + 2 * ns, d_w.get() + 2 * ns, ns * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st)); // every list is checked once, before any pair is looked at
	for (size_t i = 0; i < ns; ++i)
		if (w[2 * ns + i] != ntc::kNoBad)
			return fail(NTC_ERR_ARG, "ntc_signature_matrix_device: list %zu is not strictly ascending at entry %llu", i, w[2 * ns + i]);
	// rounds of at most kMatItems work items: the launches grow with the entries to search, not with the pairs
	std::vector<ntc::MatItem> items;
	items.reserve(ntc::kMatItems);
	auto run_round = [&]() -> int {
		if (items.empty()) return 0;
		HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ntc::MatItem), hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(ntc::sig_matrix_kernel, dim3((unsigned)items.size()), dim3(256), 0, st, d_lists, d_ns, (const ntc::MatItem*)d_items.get(), n_sigs,
		                   d_w.get() + 3 * ns);
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
	HIP_TRY(hipMemcpyAsync(counts.data(), d_w.get() + 3 * ns, cells * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (size_t i = 0; i < ns; ++i) {
		common_out[i * ns + i] = n[i];
		for (size_t j = i + 1; j < ns; ++j)
			common_out[i * ns + j] = common_out[j * ns + i] = counts[i * ns + j];
	}
	return 0;
}

} // extern "C"
