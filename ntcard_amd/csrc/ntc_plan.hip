// ntc_plan.hip — launch geometry and policy of the engine: pure host arithmetic, no HIP calls (ntc_engine.hpp)
#include "ntc_engine.hpp"

namespace ntc_eng {

// geometry of the partition passes (plan_log); A/B builds override them (tools/ab_build.sh <name> -DNTC_AB_G1=512): the product has no run-time knob
#ifndef NTC_AB_G1
#define NTC_AB_G1 256
#endif
#ifndef NTC_AB_PARTS2
#define NTC_AB_PARTS2 4
#endif
#ifndef NTC_AB_SLICE_BITS
#define NTC_AB_SLICE_BITS 15
#endif
constexpr uint32_t kApplyG1 = NTC_AB_G1, kApplyParts2 = NTC_AB_PARTS2, kApplySliceBits = NTC_AB_SLICE_BITS;

uint32_t ceil_log2(uint64_t x)
{
	uint32_t b = 0;
	while ((1ull << b) < x) ++b;
	return b;
}

// dynamic LDS per block of the simple kernel: its seed tables + the 4 waves' slots
size_t smem_simple(uint32_t stride) { return (size_t)ntc::kTableBytes + (size_t)ntc::kWavesPerBlock * 64u * stride; }

// blocks of the simple (validation) kernel a CU holds
unsigned hash_blocks_per_cu(size_t smem) { return (unsigned)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / smem)); }

// LDS bytes a spaced seed adds to K1's tables: SeedPlan::blob, and 16 B behind the last slot (the rolling form's toggle reads fetch the
// dword behind the 4 bytes they use, which for the incoming base of a read's last group lies behind the wave's last slot); 0 for plain k-mers
uint32_t seed_lds(const ntc::SeedPlan& sp) { return sp.k ? (uint32_t)sp.blob.size() * 4u + 16u : 0u; }

// per-k block of the K1 argument struct
// strand: 0 canonical; 1 forward / 2 reverse — the wanted strand's step terms and start value go FIRST, where K1's one-strand instantiations
// read them (the reverse step terms rotated right: nthash_tables.hpp, "one strand")
void fill_hfk(ntc::HfK& o, uint32_t k, uint32_t* sketch, unsigned long long* f1, const void* t1, uint32_t key_base, uint32_t strand)
{
	ntc::HashTables tab;
	uint32_t init[6];
	ntc::build_tables(k, tab);
	ntc::poly_a_state(k, init);
	o.k = k;
	o.init_f = init[2];
	o.init_r = init[5];
	o.strand = strand;
	o.key_base = key_base;
	o.pad2_ = 0;
	o.sketch = sketch;
	o.f1 = f1;
	o.t1 = t1;
	for (int slot = 0; slot < ntc::kMainSlots; ++slot) {
		o.tabh[slot][0] = tab.A[slot][1];
		o.tabh[slot][1] = tab.A[slot][3];
		if (strand == 2) o.tabh[slot][0] = ntc::hd_rotr(tab.A[slot][3]);
	}
	if (strand == 2) o.init_f = init[5];
}

// K1's arguments of a spaced-seed plane (a launch of its own: HfArgs holds one seed)
void set_seed_args(ntc::HfArgs& a, const ntc::SeedPlan& sp, const void* d_blob)
{
	a.gap = sp.n_dc;
	a.gapt = d_blob;
	a.seed_nroll = sp.n_roll;
	a.seed_extra = sp.extra_bytes();
	std::memcpy(a.tabg, sp.tabg, sizeof a.tabg);
	std::memcpy(a.roll_t, sp.roll_t, sizeof a.roll_t);
}

// block shape of K1 only: waves per CU and waves per block for a slot stride, 0 waves = does not fit
// seed_lds: the LDS a spaced seed adds (seed_lds(SeedPlan)), 0 for plain k-mers
void hf_shape(uint32_t stride, const uint32_t* ks, uint32_t n_k, uint32_t seed_lds, HfPlan& p, size_t& shared_out)
{
	const size_t per_wave = 64u * (size_t)stride; // the wave's 64 decoded slots; hit masks and the compaction queue are registers
	size_t shared = 16 + (size_t)seed_lds;
	for (uint32_t j = 0; j < n_k; ++j)
		shared += (size_t)ntc::t2_pairs(ks[j]) * 256u; // the closed-form tables of every fused k are resident
	// A workgroup's LDS (dynamic + the kernel's static tables) is allocated in granules of 1280 B, 128 of them per
	// CU (measured: 3 blocks of 43 granules do not co-reside, 3 of 42 do).  A plan that overestimates the resident
	// blocks leaves part of the persistent grid waiting for a second round, which costs far more than a wave less.
	const size_t granule = 1280, granules_per_cu = 128, static_lds = 1024 + 256 + 64;
	unsigned best_waves = 0;
	auto consider = [&](unsigned w) {
		const size_t alloc = (shared + w * per_wave + static_lds + granule - 1) / granule;
		if (alloc > granules_per_cu || shared + w * per_wave > kMaxDynLds) return;
		const unsigned waves = std::min<unsigned>(16, (unsigned)(granules_per_cu / alloc) * w); // 128 VGPRs: 4 waves per SIMD
		if (waves >= best_waves) { // ties: the larger block (fewer table copies)
			best_waves = waves;
			p.wpb = w;
		}
	};
	// whole multiples of the 4 SIMDs keep them evenly loaded (measured: 6 or 13 waves per block cost 5-12 %,
	// 3 blocks of 3 waves lose to 2 blocks of 4); smaller blocks only when not even 4 waves fit
	for (unsigned w = 4; w <= 16; w += 4)
		consider(w);
	for (unsigned w = 3; best_waves == 0 && w >= 1; --w)
		consider(w);
	p.waves_per_cu = best_waves;
	shared_out = shared;
}

// Slot stride the host packer uses for reads of up to `maxlen` bytes: a multiple of 4; an ODD number of dwords keeps
// the 64 lanes of a wave on distinct LDS banks when they read the same column of their slots (160 B = 40 dwords is
// an 8-way conflict, measured 8 % slower than 156 B), taken whenever it does not cost a wave of occupancy.
uint32_t pick_stride(uint64_t maxlen, const std::vector<uint32_t>& klist, uint32_t seed_lds)
{
	const uint32_t s0 = (uint32_t)((maxlen + 3) & ~3ull);
	if ((s0 / 4) & 1u) return s0;
	HfPlan a, b;
	size_t sh;
	hf_shape(s0, klist.data(), (uint32_t)std::min<size_t>(klist.size(), ntc::kMaxFusedK), seed_lds, a, sh);
	hf_shape(s0 + 4, klist.data(), (uint32_t)std::min<size_t>(klist.size(), ntc::kMaxFusedK), seed_lds, b, sh);
	return b.waves_per_cu >= a.waves_per_cu && b.waves_per_cu > 0 ? s0 + 4 : s0;
}

// A list of which a part is K1's: K1 stages the SAME tiles, 64 slots of 16 x ceil(len / 16) bytes per wave next to its closed-form tables.  Does that fit the
// CU's LDS for every such k on its own (run_batch splits a fused group that does not fit; a single k has to)?  Equal-length reads beyond ~2.4 kb do not:
// host batches then take row slots, whose packer cuts long sequences into overlapping chunks, and a device-resident tiled batch is refused BEFORE
// anything of it has been counted.
bool k1_fits_tiles(const ntc_engine* e, uint32_t read_len)
{
	if (e->ts_all) return true;
	const uint32_t stride = 16u * ((read_len + 15u) / 16u);
	for (size_t ki = 0; ki < e->klist.size(); ++ki) {
		if (e->k_tiled[ki] || !e->plain(ki)) continue; // (K1's spaced planes take the batch as row slots)
		HfPlan p;
		size_t shared = 0;
		hf_shape(stride, &e->klist[ki], 1, 0, p, shared);
		if (p.waves_per_cu == 0 || shared + p.wpb * (64u * (size_t)stride) > kMaxDynLds) return false;
	}
	return true;
}

// ntcard's -g seed 1^a 0^g 1^a (a, g >= 1) -> g; any other mask -> 0
uint32_t symmetric_gap(const std::string& m)
{
	const size_t a = m.find('0');
	if (a == 0 || a == std::string::npos || m.size() < 2 * a + 1) return 0;
	const size_t g = m.size() - 2 * a;
	return m == std::string(a, '1') + std::string(g, '0') + std::string(a, '1') ? (uint32_t)g : 0u;
}

// upper estimate of the k-mers of one k a read of `len` bases has sampled (both samples ~2^-sBits of the windows each, App. B of SURVEY.md)
double sampled_per_read(int64_t len, uint32_t k, uint32_t s_bits) { return (double)std::max<int64_t>(0, len - (int64_t)k + 1) * std::ldexp(1.15, 1 - (int)s_bits); }

// The first sizeable equal-length batch after a reset is cut in two: a small head goes first, the probe samples what it logged and decides log vs
// direct atomics on the device, and the bulk of the batch already runs in that mode.  The head is sized to log the ~2^20 entries the probe wants
// (0.6 M reads at sBits = 7, k = 32), in multiples of 2048 reads: in a tiled batch, whose tiles hold 2048 reads each, the rest starts at a tile boundary.
uint64_t probe_head_reads(double per_read) { return (((uint64_t)(1.25 * (1 << 20) / per_read) + 2047) / 2048) * 2048; }

// Suspects per K1h wave: room for EVERY candidate of the wave's share (reads dense with non-base bytes make every candidate a suspect:
// with a short list the launch fell back to K1f's slow path — 15 ms per 10 M reads at 2 % N).  The share: the
// blocks of a wave (plan_sketch_k1h: even shares of a workgroup's quota) + 1, all of
// them full (2048 reads x 16 windows); ntComp's patterns pass 3 / 256 of the windows at sBits = 7, their 8-bit prefixes 2 / 256 at
// sBits >= 8 (ntcard.cpp:132-145), measured 1.3 x that on reads with 10 % N (ties ride along): x 1.5, + 1024, at least 2048, at most
// 1 GiB per launch (beyond that a launch may still overflow: slow path, exact).  The batches of ONE launch share one list — a wave's region is
// its number in the launch, and every batch is walked by waves of its own — so a launch over eight batches needs one list, not eight.
uint32_t k1h_suspects_per_wave(uint32_t blocks_per_wave, uint32_t s_bits, uint32_t max_waves)
{
	const double lone_blocks = (double)blocks_per_wave + 1.0;
	const double per_block = 2048.0 * 16.0 * (s_bits == 7 ? 3.0 : 2.0) / 256.0;
	return (uint32_t)std::min<double>(std::max<double>(2048.0, 1.5 * lone_blocks * per_block + 1024.0), (double)((1ull << 30) / 16u / max_waves));
}

// Geometry of the hit log and of its partition passes for this engine's key space (keys are indices into the whole
// sketch array: k index, sample and bucket).  Returns false when the keys do not fit (then ntComp's increments stay
// direct atomics): more than 2^32 counters, or more than two 8-bit partition passes above a 2^15-counter slice.
bool plan_log(ntc_engine* e, uint64_t want_entries)
{
	const uint64_t counters = e->klist.size() * e->plane_elems();
	if (counters > (1ull << 32)) return false;
	auto& ap = e->ap;
	ap.key_bits = ceil_log2(counters);
	ap.slice_bits = std::min<uint32_t>(kApplySliceBits, ap.key_bits);
	const uint32_t pb = ap.key_bits - ap.slice_bits;
	if (pb > 16) return false;
	ap.b1 = pb <= 8 ? pb : (pb + 1) / 2; // two passes: balanced fan-out (longer runs per digit coalesce better than 256-way + 32-way); with the second
	                                     // pass's uint16 runs 7 + 6 bits still beat 6 + 7 and 5 + 8 (0.101 / 0.103 / 0.131 ms per step, profiles/r05_apply_geometry_sweep.txt)
	ap.b2 = pb - ap.b1;
	ap.n_slices = (uint32_t)((counters + (1ull << ap.slice_bits) - 1) >> ap.slice_bits);
	// default: four entries per counter, at most 2^30 (4 GiB at rBits = 27 and one k: the apply's sweep over the whole sketch is then
	// paid once per ~900 M sampled k-mers; 288 GB of HBM have room for the log and its two partition work areas, 12 GiB in all)
	uint64_t cap = want_entries ? want_entries : std::min<uint64_t>(1ull << 30, std::max<uint64_t>(1ull << 18, 4 * counters));
	cap = std::max<uint64_t>(cap, 1ull << 14);
	e->log_region_cap = (uint32_t)std::min<uint64_t>(32768, std::max<uint64_t>(256, cap / 8192)); // <= 65535: one run fits a 16-bit count pass
	e->log_regions = (uint32_t)std::max<uint64_t>(1, cap / e->log_region_cap);
	e->log_cap = (uint64_t)e->log_regions * e->log_region_cap;
	e->klog_regions = std::max<uint32_t>(1, std::min<uint32_t>(1024, e->log_regions / 8)); // 32 Mi entries at the default geometry; a full region falls back to atomics
	// pass 1: g1 workgroups, each owns every g1-th region and writes 2^b1 private runs; a run holds its expected
	// share of a FULL log + 25 % (+64); what does not fit is applied directly (exact), so the margin is about speed only
	ap.g1 = std::min<uint32_t>(e->log_regions, kApplyG1); // one 1024-thread workgroup per CU: few, long private runs (measured 128 … 4096)
	const uint64_t share1 = (uint64_t)((e->all_log_regions() + ap.g1 - 1) / ap.g1) * e->log_region_cap;
	ap.cap1 = (uint32_t)(((share1 >> ap.b1) * 5 / 4 + 64 + 7) & ~7ull); // (multiples of 8 keys: the count pass reads uint16 runs 16 bytes at a time)
	// pass 2: bucket b of pass 1 is split again by `parts2` workgroups
	ap.parts2 = kApplyParts2;
	const uint64_t share2 = ((((uint64_t)e->all_log_regions() * e->log_region_cap) >> ap.b1) * 5 / 4) / ap.parts2 + 1;
	ap.cap2 = (uint32_t)(((share2 >> ap.b2) * 13 / 10 + 64 + 7) & ~7ull);
	return true;
}

} // namespace ntc_eng

extern "C" int ntc_long_plan(uint32_t k, uint32_t piece_len, uint64_t len, uint64_t* pieces, uint64_t* rem_start)
{
	using ntc_eng::fail;
	if (!pieces || !rem_start) return fail(NTC_ERR_ARG, "ntc_long_plan: null argument");
	if (k < 1 || k > 65520u - 15u || (piece_len & 15u) || piece_len > 65520u || piece_len < k + 15u)
		return fail(NTC_ERR_ARG, "ntc_long_plan: piece_len %u: need a multiple of 16 with k + 15 = %u <= piece_len <= 65520", piece_len, k + 15u);
	const uint64_t step = piece_len - (k - 1u); // window starts per piece: every window of k bases lies in exactly one piece or in the remainder
	const uint64_t m = len >= piece_len ? (len - piece_len) / step + 1u : 0u;
	*pieces = m;
	*rem_start = m * step;
	return 0;
}
