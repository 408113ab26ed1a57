// ntc_hpc.hip — homopolymer compression on the device (include/ntcard_hip.h: NTC_FLAG_HPC, ntc_hpc_compress_device): a stream compaction whose output
// length depends on the data.  Byte j of a sequence is dropped iff j > 0 and it has the base class (A, C, G, T = U, either case) of byte j - 1; every other
// byte is kept, in order, unchanged.  One compaction takes a run of whole sequences that lie behind one another in memory (offsets[0] .. offsets[n_seqs]).
//
// Positions: the source may start at any address, so everything is laid over the ALIGNED dwords of the source — position v = lead + j of source byte j,
// lead = the source address mod 4; dword g holds the positions 4 g .. 4 g + 3, positions below lead or from lead + n on hold no byte of a sequence and are
// never kept.  Only dwords that hold at least one sequence byte are loaded (dword g - 1 of a dword g > 0 always does).
// Five launches, none of which waits on a workgroup of its own launch:
//   mark     bit v of the bit array = position v starts a sequence (a run never continues across a boundary)
//   flag     a wave per CHUNK of 4096 positions, a dword per lane and step: the keep bits of its four positions from its dword, the byte in front of it
//            (the neighbouring lane's, by shuffle) and the start bits; the bit array is rewritten IN PLACE with the keep bits (eight lanes share a word
//            of it), and the chunk's kept bytes go to a table
//   scan     exclusive 64-bit prefix sums of the table, one workgroup
//   scatter  a wave per chunk again: ranks from four ballots per step (one per byte of the dword) and their prefix popcounts; the kept bytes are staged in
//            LDS at the phase of the output's dword grid, so that the global stores are whole aligned dwords — only the up to three bytes at either end of
//            a chunk's output, which share their dword with the neighbouring chunk, are stored as bytes
//   offsets  a thread per sequence: new offset = prefix of the chunk + popcount of the chunk's keep bits in front of the sequence's first position
#include <algorithm>

#include "ntc_kernels.hpp"

namespace ntc {

namespace {

constexpr uint32_t kHpcSteps = 16;                     // dwords per lane: 16 loads in flight
constexpr uint32_t kHpcChunkWords = 64u * kHpcSteps;   // a wave's chunk: 1024 dwords
constexpr uint32_t kHpcChunk = 4u * kHpcChunkWords;    // = 4096 positions
constexpr uint32_t kHpcRow = kHpcChunk + 16u;          // LDS bytes of a wave's staging row (the output's phase, 0 .. 3, in front)

struct HpcGeom {
	const uint32_t* words; // aligned dword 0: the one that holds the first source byte
	uint32_t lead;         // position of the first source byte in it
	uint64_t end;          // lead + n: the position behind the last source byte
	uint64_t n_words;      // ceil(end / 4)
	uint64_t n_chunks;     // ceil(n_words / kHpcChunkWords)
};

// 0 .. 3: A C G T/U of either case; 0xff: no class (N, IUPAC, CR, the control bytes the seed table takes for bases)
__device__ __forceinline__ uint32_t hpc_class(uint32_t b)
{
	const uint32_t x = b | 0x20u; // (b | 0x20 == 'a' only for 'A' and 'a', and so on)
	return x == 'a' ? 0u : x == 'c' ? 1u : x == 'g' ? 2u : (x == 't' || x == 'u') ? 3u : 0xffu;
}

// the positions of dword g that hold a source byte, as a 4-bit mask
__device__ __forceinline__ uint32_t hpc_valid4(const HpcGeom& g, uint64_t gi)
{
	if (gi >= g.n_words) return 0u;
	uint32_t m = gi == 0 ? (0xfu << g.lead) & 0xfu : 0xfu;
	if (4u * gi + 4u > g.end) m &= (1u << (uint32_t)(g.end - 4u * gi)) - 1u;
	return m;
}

// keep bits of the four bytes of w; prev: the byte in front of them (anything where the first valid position is a start)
__device__ __forceinline__ uint32_t hpc_keep4(uint32_t w, uint32_t prev, uint32_t start4, uint32_t valid4)
{
	uint32_t keep = 0, pc = hpc_class(prev);
#pragma unroll
	for (uint32_t i = 0; i < 4; ++i) {
		const uint32_t c = hpc_class((w >> (8u * i)) & 0xffu);
		keep |= (c != 0xffu && c == pc ? 0u : 1u) << i;
		pc = c;
	}
	return (keep | start4) & valid4;
}

__global__ __launch_bounds__(256) void hpc_mark_kernel(const uint64_t* __restrict__ off, uint64_t n_seqs, uint32_t lead, uint64_t n, uint32_t* __restrict__ bits)
{
	const uint64_t off0 = off[0];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_seqs; i += (uint64_t)gridDim.x * 256u) {
		const uint64_t p = off[i] - off0;
		if (p < n) atomicOr(&bits[(lead + p) >> 5], 1u << (uint32_t)((lead + p) & 31u)); // (empty sequences at the very end start nowhere)
	}
}

__global__ __launch_bounds__(256) void hpc_flag_kernel(HpcGeom g, uint32_t* __restrict__ bits, uint32_t* __restrict__ counts)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t chunk = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (chunk >= g.n_chunks) return;
	const uint64_t w0 = chunk * kHpcChunkWords;
	uint32_t v[kHpcSteps], sb[kHpcSteps];
#pragma unroll
	for (uint32_t i = 0; i < kHpcSteps; ++i) {
		const uint64_t gi = w0 + i * 64u + lane;
		const bool in = gi < g.n_words;
		v[i] = in ? g.words[gi] : 0u;
		sb[i] = in ? bits[gi >> 3] : 0u;
	}
	uint32_t carry = (lane == 0 && w0 > 0) ? g.words[w0 - 1] >> 24 : 0u; // the byte in front of the chunk
	uint32_t total = 0;
#pragma unroll
	for (uint32_t i = 0; i < kHpcSteps; ++i) {
		const uint64_t gi = w0 + i * 64u + lane;
		const uint32_t top = v[i] >> 24, up = (uint32_t)__shfl_up((int)top, 1);
		const uint32_t prev = lane == 0 ? carry : up;
		carry = (uint32_t)__shfl((int)top, 63);
		const uint32_t keep = hpc_keep4(v[i], prev, (sb[i] >> (4u * (uint32_t)(gi & 7u))) & 0xfu, hpc_valid4(g, gi));
		uint32_t nib = keep << (4u * (lane & 7u)); // eight lanes -> one word of the bit array
		nib |= (uint32_t)__shfl_xor((int)nib, 1);
		nib |= (uint32_t)__shfl_xor((int)nib, 2);
		nib |= (uint32_t)__shfl_xor((int)nib, 4);
		if ((lane & 7u) == 0 && gi < g.n_words) bits[gi >> 3] = nib;
		total += (uint32_t)__popc(keep);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		total += (uint32_t)__shfl_xor((int)total, o);
	if (lane == 0) counts[chunk] = total;
}

// pre[c] = the kept bytes of the chunks in front of c; pre[n_chunks] = all of them
__global__ __launch_bounds__(1024) void hpc_scan_kernel(const uint32_t* __restrict__ counts, uint64_t n_chunks, uint64_t* __restrict__ pre)
{
	__shared__ uint64_t part[1024];
	const uint64_t per = (n_chunks + 1023u) / 1024u;
	const uint64_t b = std::min<uint64_t>(threadIdx.x * per, n_chunks), e = std::min<uint64_t>(b + per, n_chunks);
	uint64_t sum = 0;
	for (uint64_t j = b; j < e; ++j)
		sum += counts[j];
	part[threadIdx.x] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t run = 0;
		for (uint32_t t = 0; t < 1024u; ++t) {
			const uint64_t s = part[t];
			part[t] = run;
			run += s;
		}
		pre[n_chunks] = run;
	}
	__syncthreads();
	uint64_t run = part[threadIdx.x];
	for (uint64_t j = b; j < e; ++j) {
		pre[j] = run;
		run += counts[j];
	}
}

__global__ __launch_bounds__(256) void hpc_scatter_kernel(HpcGeom g, const uint32_t* __restrict__ bits, const uint64_t* __restrict__ pre, unsigned char* __restrict__ out)
{
	__shared__ __attribute__((aligned(16))) unsigned char rows[4][kHpcRow];
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint64_t chunk = (uint64_t)blockIdx.x * 4u + wave;
	const bool live = chunk < g.n_chunks; // (a wave without a chunk keeps nothing, and still meets the barrier)
	const uint64_t base = live ? pre[chunk] : 0u;
	const uint32_t cnt = live ? (uint32_t)(pre[chunk + 1] - base) : 0u;
	const uint32_t a = (uint32_t)((reinterpret_cast<uintptr_t>(out) + base) & 3u); // the phase of the chunk's first output byte in its aligned dword
	unsigned char* row = rows[wave];
	const uint64_t w0 = chunk * kHpcChunkWords;
	uint32_t v[kHpcSteps], kb[kHpcSteps];
#pragma unroll
	for (uint32_t i = 0; i < kHpcSteps; ++i) {
		const uint64_t gi = w0 + i * 64u + lane;
		const bool in = live && gi < g.n_words;
		v[i] = in ? g.words[gi] : 0u;
		kb[i] = in ? (bits[gi >> 3] >> (4u * (uint32_t)(gi & 7u))) & 0xfu : 0u;
	}
	uint32_t run = a;
#pragma unroll
	for (uint32_t i = 0; i < kHpcSteps; ++i) {
		const uint32_t keep = kb[i];
		uint32_t below = 0, all = 0;
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j) {
			const uint64_t m = __builtin_amdgcn_ballot_w64(((keep >> j) & 1u) != 0u);
			below += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
			all += (uint32_t)__popcll(m);
		}
		uint32_t r = run + below; // (at most a + cnt - 1 for a kept byte: inside the row)
#pragma unroll
		for (uint32_t j = 0; j < 4; ++j)
			if ((keep >> j) & 1u) row[r++] = (unsigned char)(v[i] >> (8u * j));
		run += all;
	}
	__syncthreads();
	// row byte q, a <= q < a + cnt, is output byte base + q - a; q % 4 == 0 is dword-aligned in memory
	unsigned char* dst = out + base - a;
	const uint32_t end = a + cnt, nd = (end + 3u) / 4u;
	for (uint32_t d = lane; d < nd && cnt != 0; d += 64u) {
		const uint32_t lo = 4u * d, hi = lo + 4u;
		if (lo >= a && hi <= end) {
			*reinterpret_cast<uint32_t*>(dst + lo) = *reinterpret_cast<const uint32_t*>(row + lo);
		} else { // the first or the last dword of the chunk's output: the neighbouring chunk writes its other bytes
			for (uint32_t q = lo < a ? a : lo; q < (hi < end ? hi : end); ++q)
				dst[q] = row[q];
		}
	}
}

__global__ __launch_bounds__(256) void hpc_offsets_kernel(const uint64_t* __restrict__ off, uint64_t n_off, uint32_t lead, uint64_t n, const uint32_t* __restrict__ bits,
                                                          const uint64_t* __restrict__ pre, uint64_t n_chunks, uint64_t* __restrict__ off_out)
{
	const uint64_t off0 = off[0];
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_off; i += (uint64_t)gridDim.x * 256u) {
		const uint64_t p = off[i] - off0;
		if (p >= n) {
			off_out[i] = pre[n_chunks];
			continue;
		}
		const uint64_t v = lead + p, c = v / kHpcChunk;
		uint64_t r = pre[c];
		for (uint64_t w = c * (kHpcChunk / 32u); w < (v >> 5); ++w)
			r += (uint32_t)__popc(bits[w]);
		r += (uint32_t)__popc(bits[v >> 5] & ((1u << (uint32_t)(v & 31u)) - 1u));
		off_out[i] = r;
	}
}

// the carve-up of a compaction's scratch: [offsets in][offsets out][prefixes][table][bit array]
struct HpcAux {
	uint64_t* off_in;
	uint64_t* off_out;
	uint64_t* pre;
	uint32_t* counts;
	uint32_t* bits;
	uint64_t n_chunks, bit_words;
	size_t bytes;
};
HpcAux hpc_carve(void* aux, uint64_t n_bytes, uint64_t n_seqs)
{
	HpcAux x;
	const uint64_t n_words = (n_bytes + 3u + 3u) / 4u; // (lead <= 3)
	x.n_chunks = (n_words + kHpcChunkWords - 1u) / kHpcChunkWords;
	x.bit_words = x.n_chunks * (kHpcChunk / 32u);
	unsigned char* p = static_cast<unsigned char*>(aux);
	x.off_in = reinterpret_cast<uint64_t*>(p), p += (n_seqs + 1u) * 8u;
	x.off_out = reinterpret_cast<uint64_t*>(p), p += (n_seqs + 1u) * 8u;
	x.pre = reinterpret_cast<uint64_t*>(p), p += (x.n_chunks + 1u) * 8u;
	x.counts = reinterpret_cast<uint32_t*>(p), p += ((x.n_chunks + 1u) & ~1ull) * 4u;
	x.bits = reinterpret_cast<uint32_t*>(p), p += x.bit_words * 4u;
	x.bytes = (size_t)(p - static_cast<unsigned char*>(aux));
	return x;
}

} // namespace

size_t hpc_aux_bytes(uint64_t n_bytes, uint64_t n_seqs) { return hpc_carve(nullptr, n_bytes, n_seqs).bytes; }

const uint64_t* hpc_aux_offsets(const void* aux, uint64_t n_seqs) { return hpc_carve(const_cast<void*>(aux), 0, n_seqs).off_out; }

hipError_t launch_hpc_compact(const unsigned char* src, const uint64_t* h_off, uint64_t n_seqs, unsigned char* out, void* aux, hipStream_t st)
{
	const uint64_t n = h_off[n_seqs] - h_off[0];
	const HpcAux x = hpc_carve(aux, n, n_seqs);
	if (n == 0) return hipMemsetAsync(x.off_out, 0, (n_seqs + 1u) * 8u, st);
	const uintptr_t first = reinterpret_cast<uintptr_t>(src) + h_off[0];
	HpcGeom g;
	g.words = reinterpret_cast<const uint32_t*>(first & ~(uintptr_t)3);
	g.lead = (uint32_t)(first & 3u);
	g.end = g.lead + n;
	g.n_words = (g.end + 3u) / 4u;
	g.n_chunks = (g.n_words + kHpcChunkWords - 1u) / kHpcChunkWords; // (<= x.n_chunks, which allows for any lead)
	const uint64_t blocks = (g.n_chunks + 3u) / 4u;
	if (blocks > 0x7fffffffull) return hipErrorInvalidValue; // (32 TiB in one compaction; the engine works in rounds far below)
	hipError_t rc = hipMemcpyAsync(x.off_in, h_off, (n_seqs + 1u) * 8u, hipMemcpyHostToDevice, st);
	if (rc != hipSuccess) return rc;
	rc = hipMemsetAsync(x.bits, 0, x.bit_words * 4u, st);
	if (rc != hipSuccess) return rc;
	const unsigned seq_blocks = (unsigned)std::min<uint64_t>((n_seqs + 1u + 255u) / 256u, 256u * 8u);
	hipLaunchKernelGGL(hpc_mark_kernel, dim3(seq_blocks), dim3(256), 0, st, x.off_in, n_seqs, g.lead, n, x.bits);
	hipLaunchKernelGGL(hpc_flag_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, x.bits, x.counts);
	hipLaunchKernelGGL(hpc_scan_kernel, dim3(1), dim3(1024), 0, st, x.counts, g.n_chunks, x.pre);
	hipLaunchKernelGGL(hpc_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, x.bits, x.pre, out);
	hipLaunchKernelGGL(hpc_offsets_kernel, dim3(seq_blocks), dim3(256), 0, st, x.off_in, n_seqs + 1u, g.lead, n, x.bits, x.pre, g.n_chunks, x.off_out);
	return hipGetLastError();
}

} // namespace ntc
