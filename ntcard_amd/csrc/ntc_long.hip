// ntc_long.hip — long sequences for the tiled kernels (include/ntcard_hip.h: ntc_submit_long_device): the device-side re-layout of a sequence's
// overlapping pieces [j S, j S + L) into the tiled slot layout (cut_tiles_kernel), and of its remainder — or of whole sequences — into row slots
// (gather_slots_kernel).  Both read source bytes of ANY alignment: a lane loads the aligned dwords that hold its four bytes and shifts them
// together in registers, so only 4-byte words that hold at least one byte of the source are ever touched.
#include <algorithm>

#include "ntc_kernels.hpp"

namespace ntc {

namespace {

constexpr uint32_t kCutRun = 16;                 // chunks of a piece one workgroup moves: 256 contiguous source bytes per piece
constexpr uint32_t kCutRow = kCutRun * 16u + 16u; // LDS row of a piece, padded by one 16-byte slot: 64 rows read 16 bytes each without a bank conflict

// bytes [addr, addr + 4) of memory, addr of any alignment; only_lo: the bytes of the second aligned word are not wanted (it may lie behind the source)
__device__ __forceinline__ uint32_t load_unaligned_u32(uintptr_t addr, bool only_lo)
{
	const uint32_t s = (uint32_t)(addr & 3u);
	const uint32_t* w = reinterpret_cast<const uint32_t*>(addr - s);
	const uint32_t lo = w[0];
	const uint32_t hi = (s != 0u && !only_lo) ? w[1] : 0u;
	return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * s));
}

// Pieces -> tiles.  A workgroup takes 64 consecutive pieces (one lane group of a tile: 2048 % 64 == 0) x a run of up to kCutRun chunks.
//   where: piece p of the call belongs to the sequence s with seqs[s].first <= p < seqs[s + 1].first and starts at seqs[s].src + (p - seqs[s].first) * step.
//        Wave 0 finds the sequence of the workgroup's first piece — a 64-way search of the table, one probe per lane and step: three steps for 2^18
//        sequences —, loads the 64 entries behind it (every entry holds a piece, so the workgroup's pieces lie in these) and every lane searches them, in
//        LDS, for its own piece.  A round of a call passes the call's whole table and its first piece: it may begin and end in the middle of a sequence
//   in:  wave w reads the run of pieces 16 w .. 16 w + 15, one piece per step: 64 lanes x 4 B = the run's 256 contiguous bytes
//   out: per chunk one line group of the tile — 64 lanes x 16 B = 1 KiB contiguous — from LDS rows of kCutRow bytes
// Slots behind the last piece (the rest of the last tile) stay unwritten: the tiled kernels ignore them.
__global__ __launch_bounds__(256) void cut_tiles_kernel(const unsigned char* __restrict__ src, const LongSeq* __restrict__ seqs, uint32_t n_seqs, uint64_t first_piece,
                                                        uint64_t n_pieces, uint32_t step, uint32_t n_chunks, uint32_t n_runs, unsigned char* __restrict__ tiles)
{
	__shared__ __attribute__((aligned(16))) unsigned char rows_lds[64 * kCutRow];
	__shared__ uint64_t win_src[65], win_first[65]; // the table from the first piece's sequence on
	__shared__ uint64_t off_lds[64];  // source offset of the workgroup's pieces
	const uint64_t p0 = (uint64_t)(blockIdx.x / n_runs) * 64u; // (within the round)
	const uint32_t c0 = (blockIdx.x % n_runs) * kCutRun;
	const uint32_t nc = n_chunks - c0 < kCutRun ? n_chunks - c0 : kCutRun; // chunks of this run
	const uint32_t nb = nc * 16u;                                           // bytes per piece of this run
	const uint32_t n_rows = n_pieces - p0 < 64u ? (uint32_t)(n_pieces - p0) : 64u;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (wave == 0) {
		const uint64_t g0 = first_piece + p0; // the first piece, in the call's numbering
		uint32_t lo = 0, hi = n_seqs;          // seqs[lo].first <= g0 < seqs[hi].first (seqs[0].first == 0; the sentinel holds the call's pieces)
		while (hi - lo > 1u) {
			const uint32_t stride = (hi - lo + 63u) / 64u, i = lo + lane * stride;
			const uint32_t n_le = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(i < hi && seqs[i].first <= g0)); // (monotone: a prefix of the lanes; lane 0 is in it)
			hi = __builtin_amdgcn_readfirstlane(lo + n_le * stride < hi ? lo + n_le * stride : hi);
			lo = __builtin_amdgcn_readfirstlane(lo + (n_le - 1u) * stride);
		}
		// (entries lo .. lo + 64; behind the sentinel: first = ~0)
		uint64_t e_src = 0, e_first = ~0ull, l_src = 0, l_first = ~0ull;
		if (lo + lane <= n_seqs) e_src = seqs[lo + lane].src, e_first = seqs[lo + lane].first;
		if (lane == 0 && lo + 64u <= n_seqs) l_src = seqs[lo + 64u].src, l_first = seqs[lo + 64u].first;
		win_src[lane] = e_src, win_first[lane] = e_first;
		if (lane == 0) win_src[64] = l_src, win_first[64] = l_first;
	}
	__syncthreads();
	if (wave == 0 && lane < n_rows) {
		const uint64_t g = first_piece + p0 + lane;
		uint32_t a = 0, b = lane + 1u; // win_first[a] <= g < win_first[b]: every sequence of the table holds a piece, so piece lane is not behind entry lane
		while (b - a > 1u) {
			const uint32_t mid = (a + b) / 2u;
			if (win_first[mid] <= g) a = mid;
			else b = mid;
		}
		off_lds[lane] = win_src[a] + (g - win_first[a]) * step;
	}
	__syncthreads();
	const bool mine = 4u * lane < nb;
	uint32_t v[16];
#pragma unroll
	for (uint32_t i = 0; i < 16; ++i) {
		const uint32_t row = wave * 16u + i;
		v[i] = 0;
		if (row < n_rows && mine) {
			// (the last dword of a piece that ends with the source: its second aligned word holds a source byte whenever the address is unaligned)
			v[i] = load_unaligned_u32(reinterpret_cast<uintptr_t>(src) + off_lds[row] + 16u * (uint64_t)c0 + 4u * lane, false);
		}
	}
#pragma unroll
	for (uint32_t i = 0; i < 16; ++i) {
		const uint32_t row = wave * 16u + i;
		if (row < n_rows && mine) *reinterpret_cast<uint32_t*>(rows_lds + row * kCutRow + 4u * lane) = v[i];
	}
	__syncthreads();
	if (lane < n_rows) {
		const uint64_t p = p0 + lane;
		unsigned char* dst = tiles + (((p / kTileReads) * n_chunks + c0) * kTileReads + p % kTileReads) * 16u;
		for (uint32_t c = wave; c < nc; c += 4u)
			*reinterpret_cast<uint4*>(dst + (uint64_t)c * kTileReads * 16u) = *reinterpret_cast<const uint4*>(rows_lds + lane * kCutRow + 16u * c);
	}
}

// Spans -> row slots: slot i = the span's bytes, then 'A' up to the stride; meta[i] = bytes | window-start limit << 16 (what ntc_submit's packing loop
// writes on the host).  One wave per slot at a time: 64 lanes x 4 B of contiguous source per step.
__global__ __launch_bounds__(256) void gather_slots_kernel(const unsigned char* __restrict__ src, const LongSpan* __restrict__ spans, uint64_t n_slots,
                                                           uint32_t stride, unsigned char* __restrict__ slots, uint32_t* __restrict__ meta)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t wave0 = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * 4u;
	for (uint64_t i = wave0; i < n_slots; i += n_waves) {
		const LongSpan sp = spans[i];
		const uintptr_t base = reinterpret_cast<uintptr_t>(src) + sp.src;
		uint32_t* out = reinterpret_cast<uint32_t*>(slots + i * stride);
		for (uint32_t b = 4u * lane; b < stride; b += 256u) {
			uint32_t w = 0x41414141u;
			if (b < sp.bytes) {
				const uint32_t keep = sp.bytes - b; // source bytes from b on
				const uint32_t s = (uint32_t)((base + b) & 3u);
				w = load_unaligned_u32(base + b, s + keep <= 4u); // (the second aligned word would hold no byte of the span)
				if (keep < 4u) w = (w & ((1u << (8u * keep)) - 1u)) | (0x41414141u << (8u * keep));
			}
			out[b / 4u] = w;
		}
		if (lane == 0) meta[i] = sp.bytes | (sp.limit << 16);
	}
}

} // namespace

hipError_t launch_cut_tiles(const unsigned char* src, const LongSeq* seqs, uint32_t n_seqs, uint64_t first_piece, uint64_t n_pieces, uint32_t step,
                            uint32_t piece_len, unsigned char* tiles, hipStream_t st)
{
	if (n_pieces == 0) return hipSuccess;
	if (n_seqs == 0) return hipErrorInvalidValue;
	const uint32_t n_chunks = piece_len / 16u, n_runs = (n_chunks + kCutRun - 1u) / kCutRun;
	const uint64_t blocks = ((n_pieces + 63u) / 64u) * n_runs;
	if (blocks > 0x7fffffffull) return hipErrorInvalidValue; // (the engine cuts in rounds far below this)
	hipLaunchKernelGGL(cut_tiles_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, seqs, n_seqs, first_piece, n_pieces, step, n_chunks, n_runs, tiles);
	return hipGetLastError();
}

hipError_t launch_gather_slots(const unsigned char* src, const LongSpan* spans, uint64_t n_slots, uint32_t stride, unsigned char* slots, uint32_t* meta,
                               hipStream_t st)
{
	if (n_slots == 0) return hipSuccess;
	const uint64_t blocks = std::min<uint64_t>((n_slots + 3u) / 4u, 256u * 32u);
	hipLaunchKernelGGL(gather_slots_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, spans, n_slots, stride, slots, meta);
	return hipGetLastError();
}

} // namespace ntc
