// ntc_bbloom.hpp — the block arithmetic of the BLOCKED Bloom filters (include/ntcard_hip.h: ntc_bbloom_*; DESIGN.md §4 "Blocked filters"), shared by
// ntc_bbloom.hip (insert, query, hist) and ntc_cbloom.hip (the solid insert with a blocked destination).  All n_hash bits of a value lie in ONE aligned
// 512-bit block (Putze, Sanders, Singler 2007): one random cache line per k-mer instead of n_hash.
//   block      b = h_0 mod n_blocks, n_blocks = m_bits / 512: the exact remainder of ntc_bloom_walk.hpp
//   positions  p_i = (g >> (55 - 9 (i mod 4))) & 511, g = the multi-hash of index 1 + i / 4 (nthash.hpp:381-390): four 9-bit fields from the TOP 36 bits
//              of each multi-hash value, highest first.  The low bits of t ^ (t >> 27), t = h_0 c, depend only on the low bits of h_0 — the bits that
//              chose the block when n_blocks is a power of two
//   bit        loc_i = 512 b + p_i by the plain filter's rule: dword 16 b + (p_i >> 5), bit bloom_bit(p_i) — so the image is an ordinary bit image
#pragma once
#include "ntc_bloom_walk.hpp"

namespace ntc_bloom {

constexpr uint32_t kBlockBits = NTC_BBLOOM_BLOCK_BITS;
static_assert(kBlockBits == 512u, "a block is one 64-byte line: 16 dwords, 9-bit positions");

struct BlockedHashes {
	BloomMod mod; // by n_blocks
	uint32_t n_hash;
	uint64_t kmul; // k * multiSeed
	__device__ __forceinline__ uint64_t block(uint64_t h0) const { return bloom_loc(mod, h0); }
	// the multi-hash value that holds the fields of the positions 4 q .. 4 q + 3
	__device__ __forceinline__ uint64_t group(uint64_t h0, uint32_t q) const { return bloom_multi(h0, 1u + q, kmul); }
	__device__ __forceinline__ static uint32_t field(uint64_t g, uint32_t i) { return (uint32_t)(g >> (55u - 9u * (i & 3u))) & 511u; }
};
inline BlockedHashes bbloom_hashes(uint64_t m_bits, uint32_t n_hash, uint32_t k) { return BlockedHashes{bloom_mod(m_bits / kBlockBits), n_hash, (uint64_t)k * kMultiSeed}; }

// Sets the n_hash bits of h0.  The first position that falls into a dword collects the bits of every later position in the same dword (`done`: the
// dwords of the block already served), so bits of one k-mer that share a dword go in ONE atomic.  The later positions are evaluated again for it — four
// per multi-hash value, so up to four hashes cost one multiply in all.  As in bloom_set a PLAIN load decides whether the atomic is needed: bits only go
// 0 -> 1 during a build, a stale value can only show a bit clear that is already set — a redundant atomic, never a lost one.
__device__ __forceinline__ void bbloom_set(uint32_t* filter, const BlockedHashes& hs, uint64_t h0)
{
	uint32_t* blk = filter + 16u * hs.block(h0);
	uint32_t done = 0;
	uint64_t g = 0;
	for (uint32_t i = 0; i < hs.n_hash; ++i) {
		if ((i & 3u) == 0) g = hs.group(h0, i >> 2);
		const uint32_t p = BlockedHashes::field(g, i), d = p >> 5;
		if ((done >> d) & 1u) continue;
		done |= 1u << d;
		uint32_t bits = bloom_bit(p);
		uint64_t gj = g;
		for (uint32_t j = i + 1u; j < hs.n_hash; ++j) {
			if ((j & 3u) == 0) gj = hs.group(h0, j >> 2);
			const uint32_t pj = BlockedHashes::field(gj, j);
			bits |= (pj >> 5) == d ? bloom_bit(pj) : 0u;
		}
		uint32_t* w = blk + d;
		if ((*w & bits) != bits) (void)__hip_atomic_fetch_or(w, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// Whether all n_hash bits of h0 are set: leaves at the first clear bit.  Every load is in the one line the first load fetched.
__device__ __forceinline__ bool bbloom_test(const uint32_t* filter, const BlockedHashes& hs, uint64_t h0)
{
	const uint32_t* blk = filter + 16u * hs.block(h0);
	uint64_t g = 0;
	for (uint32_t i = 0; i < hs.n_hash; ++i) {
		if ((i & 3u) == 0) g = hs.group(h0, i >> 2);
		const uint32_t p = BlockedHashes::field(g, i);
		if ((blk[p >> 5] & bloom_bit(p)) == 0) return false;
	}
	return true;
}

// the view of a blocked filter (internal linkage, as BitsView)
namespace {
struct BlockedView {
	uint32_t* filter;
	BlockedHashes hs;
	__device__ __forceinline__ void insert(uint64_t h0) const { bbloom_set(filter, hs, h0); }
	__device__ __forceinline__ bool test(uint64_t h0) const { return bbloom_test(filter, hs, h0); }
	__device__ __forceinline__ unsigned char answer(uint64_t h0) const { return test(h0) ? 1 : 0; }
};
} // namespace
inline BlockedView blocked_view(const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k)
{
	return BlockedView{static_cast<uint32_t*>(const_cast<void*>(d_filter)), bbloom_hashes(m_bits, n_hash, k)};
}

// the checks every blocked-filter call shares, before a device is looked for: check_filter with the rule for m_bits of a filter in blocks
inline int check_blocked(const char* who, const void* d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k)
{
	return check_filter(who, d_filter, m_bits, n_hash, k, "m_bits", "filter", kBlockBits);
}

} // namespace ntc_bloom
