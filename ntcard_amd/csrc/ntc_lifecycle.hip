// ntc_lifecycle.hip — an engine's life and what it answers: the error string, create / destroy / reset, sync and finish, nthll, the timing and
// state queries (ntc_engine.hpp)
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <new>

#include "ntc_engine.hpp"

using namespace ntc_eng;

namespace {
thread_local std::string g_err;

int vfail(int code, const char* fmt, va_list ap)
{
	char buf[512];
	vsnprintf(buf, sizeof buf, fmt, ap);
	g_err = buf;
	return code;
}
} // namespace

int ntc_eng::fail(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vfail(code, fmt, ap);
	va_end(ap);
	return code;
}

int ntc_internal_fail(int code, const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vfail(code, fmt, ap);
	va_end(ap);
	return code;
}

namespace {

// the checks ntc_create and ntc_create_seeded share (cfg->k holds n_k values)
int check_config(const ntc_config* cfg)
{
	constexpr uint32_t kKnownFlags = NTC_FLAG_SIMPLE_KERNEL | NTC_FLAG_DIRECT_ATOMICS | NTC_FLAG_ALWAYS_LOG | NTC_FLAG_PARTITION_ALWAYS | NTC_FLAG_LANE_KERNEL |
	                                 NTC_FLAG_REQUIRE_TILED | NTC_FLAG_DEFER_REDO | NTC_FLAG_STRAND_FORWARD | NTC_FLAG_STRAND_REVERSE | NTC_FLAG_STRAND_TILED | NTC_FLAG_HPC | NTC_FLAG_SIGNATURE;
	if (cfg->flags & ~kKnownFlags) // (ABI 4's NTC_FLAG_BITSLICE_KERNEL = 4 and NTC_FLAG_TILED_TEAMS = 256 selected kernels that no longer exist)
		return fail(NTC_ERR_ARG, "ntc_create: unknown flag bits 0x%x", cfg->flags & ~kKnownFlags);
	if ((cfg->flags & NTC_FLAG_STRAND_FORWARD) && (cfg->flags & NTC_FLAG_STRAND_REVERSE))
		return fail(NTC_ERR_ARG, "ntc_create: NTC_FLAG_STRAND_FORWARD and NTC_FLAG_STRAND_REVERSE exclude each other");
	if ((cfg->flags & NTC_FLAG_STRAND_TILED) && !(cfg->flags & (NTC_FLAG_STRAND_FORWARD | NTC_FLAG_STRAND_REVERSE)))
		return fail(NTC_ERR_ARG, "ntc_create: NTC_FLAG_STRAND_TILED needs NTC_FLAG_STRAND_FORWARD or NTC_FLAG_STRAND_REVERSE (it picks the kernels of a one-strand engine)");
	if ((cfg->flags & NTC_FLAG_SIGNATURE) && (cfg->flags & NTC_FLAG_SIMPLE_KERNEL))
		return fail(NTC_ERR_ARG, "ntc_create: NTC_FLAG_SIGNATURE needs the production kernel (the simple validation kernel keeps no sampled values)");
	for (uint32_t i = 0; i < cfg->n_k; ++i)
		if (cfg->k[i] < 1 || cfg->k[i] > kMaxK)
			return fail(NTC_ERR_ARG, "ntc_create: k=%u outside 1..%u", cfg->k[i], kMaxK);
	if (cfg->gap != 0) {
		if (cfg->n_k != 1) return fail(NTC_ERR_ARG, "ntc_create: gap seed does not support multiple k");
		if (cfg->gap % 2 != cfg->k[0] % 2 || cfg->gap >= cfg->k[0])
			return fail(NTC_ERR_ARG, "ntc_create: gap size and kmer must have the same modulus");
		if (cfg->flags & NTC_FLAG_SIMPLE_KERNEL)
			return fail(NTC_ERR_ARG, "ntc_create: spaced seeds need the production kernel");
	}
	if (cfg->r_bits < 8 || cfg->r_bits > 30) return fail(NTC_ERR_ARG, "ntc_create: r_bits %u outside 8..30", cfg->r_bits);
	if (cfg->s_bits < 2 || cfg->s_bits > 24) return fail(NTC_ERR_ARG, "ntc_create: s_bits %u outside 2..24", cfg->s_bits);
	if (cfg->log_entries > (1ull << 32)) return fail(NTC_ERR_ARG, "ntc_create: log_entries %llu above 2^32", (unsigned long long)cfg->log_entries);
	return 0;
}

// the masks of ntc_create_seeded / ntc_hll_create_ex: 1 .. NTC_MAX_K_LIST strings of '0' / '1' with at least one '1', 1 .. kMaxK long
int parse_masks(const char* who, uint32_t n_seeds, const char* const* seeds, std::vector<std::string>& masks, std::vector<uint32_t>& ks)
{
	if (n_seeds == 0 || n_seeds > NTC_MAX_K_LIST) return fail(NTC_ERR_ARG, "%s: need 1..%d seeds", who, NTC_MAX_K_LIST);
	masks.assign(n_seeds, std::string());
	ks.assign(n_seeds, 0u);
	for (uint32_t i = 0; i < n_seeds; ++i) {
		if (!seeds[i]) return fail(NTC_ERR_ARG, "%s: seed %u is null", who, i + 1);
		const size_t len = strnlen(seeds[i], (size_t)kMaxK + 1);
		if (len < 1 || len > kMaxK) return fail(NTC_ERR_ARG, "%s: seed %u: length outside 1..%u", who, i + 1, kMaxK);
		for (size_t j = 0; j < len; ++j)
			if (seeds[i][j] != '0' && seeds[i][j] != '1')
				return fail(NTC_ERR_ARG, "%s: seed %u: character %zu is neither '0' nor '1'", who, i + 1, j + 1);
		masks[i].assign(seeds[i], len);
		if (masks[i].find('1') == std::string::npos) return fail(NTC_ERR_ARG, "%s: seed %u has no '1'", who, i + 1);
		ks[i] = (uint32_t)len;
	}
	return 0;
}

// an engine under construction: any return before release() destroys it, with everything it owns so far
struct EngineDeleter {
	void operator()(ntc_engine* e) const { ntc_destroy(e); }
};
using EnginePtr = std::unique_ptr<ntc_engine, EngineDeleter>;

// what every kind of engine starts from: a valid device made current, its kernels' attributes set, an empty engine on `stream`
int new_engine(const char* who, int device, void* stream, EnginePtr& e)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
		return fail(NTC_ERR_DEVICE, "%s: no HIP device available (this library has no CPU fallback)", who);
	if (device < 0 || device >= ndev) return fail(NTC_ERR_ARG, "%s: device %d of %d", who, device, ndev);
	HIP_TRY(hipSetDevice(device));
	if (int rc = ensure_kernel_attrs(device)) return rc;
	e.reset(new (std::nothrow) ntc_engine());
	if (!e) return fail(NTC_ERR_MEMORY, "%s: out of host memory", who);
	e->device = device;
	e->stream = (hipStream_t)stream;
	return 0;
}

// the runs and run counts of the sketch update's two partition passes (plan_log)
bool reserve_partition_scratch(ntc_engine* e)
{
	const auto& ap = e->ap;
	const size_t runs1 = ap.b1 ? (size_t)ap.g1 << ap.b1 : 0, runs2 = ap.b2 ? ((size_t)ap.parts2 << ap.b1) << ap.b2 : 0;
	return (!runs1 || (e->d_s1.reserve(runs1 * ap.cap1 * ap.key_bytes(1)) && e->d_c1.reserve(runs1 * 4))) &&
	       (!runs2 || (e->d_s2.reserve(runs2 * ap.cap2 * ap.key_bytes(2)) && e->d_c2.reserve(runs2 * 4)));
}

// ntc_create / ntc_create_seeded past their argument checks; masks[i]: the spaced seed of plane i (empty: plain k-mers)
int create_engine(const ntc_config* cfg, const std::vector<std::string>& masks, bool seeded, ntc_engine** out)
{
	EnginePtr e;
	if (int rc = new_engine("ntc_create", cfg->device, cfg->stream, e)) return rc;
	const size_t nk = cfg->n_k;
	e->klist.assign(cfg->k, cfg->k + nk);
	e->seeded = seeded;
	e->strand = (cfg->flags & NTC_FLAG_STRAND_FORWARD) ? 1u : (cfg->flags & NTC_FLAG_STRAND_REVERSE) ? 2u : 0u;
	e->hpc = (cfg->flags & NTC_FLAG_HPC) != 0;
	e->sig = (cfg->flags & NTC_FLAG_SIGNATURE) != 0;
	e->masks.assign(nk, std::string());
	e->kgap.assign(nk, 0u);
	e->seeds.assign(nk, ntc::SeedPlan());
	for (size_t ki = 0; ki < masks.size(); ++ki) {
		const std::string& m = masks[ki];
		if (m.find('0') == std::string::npos) continue; // every position cared for: plain k-mers (K1h / K1 exactly as a k list)
		e->masks[ki] = m;
		e->kgap[ki] = symmetric_gap(m);
		ntc::build_seed_plan(m, e->seeds[ki]);
		ntc::strand_seed_plan(e->seeds[ki], e->strand);
		e->max_seed_lds = std::max(e->max_seed_lds, seed_lds(e->seeds[ki]));
	}
	e->r_bits = cfg->r_bits;
	e->s_bits = cfg->s_bits;
	e->kernel_kind = (cfg->flags & NTC_FLAG_SIMPLE_KERNEL) ? KIND_SIMPLE : KIND_HF;
	// (the order of the device allocations matters: the log below takes what the ones before it have left)
	const size_t sk_bytes = nk * e->plane_elems() * sizeof(uint32_t);
	if (!cfg->ext_sketch && !e->own_sketch.reserve(sk_bytes)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate %zu B sketch on device", sk_bytes);
	e->d_sketch = cfg->ext_sketch ? (uint32_t*)cfg->ext_sketch : e->own_sketch.get();
	if (!cfg->ext_f1 && !e->own_f1.reserve(nk * 8)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate F1 on device");
	e->d_f1 = cfg->ext_f1 ? (unsigned long long*)cfg->ext_f1 : e->own_f1.get();
	if (!e->d_skdirty.reserve(64 + 2 * 64 * 8)) // (the word, then ntc_log_export_device's cursors and offsets)
		return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate engine state on device");
	if (!e->d_phist.reserve(nk * 2 * 65536 * 4)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate histogram on device");
	e->d_t1.resize(nk);
	for (size_t ki = 0; ki < nk; ++ki) {
		std::vector<uint32_t> t1((size_t)ntc::t2_pairs(e->klist[ki]) * 64);
		ntc::build_t2(e->klist[ki], t1.data(), e->plain(ki) ? nullptr : e->masks[ki].c_str());
		ntc::strand_t2(e->klist[ki], t1.data(), e->strand);
		if (!e->d_t1[ki].upload(t1)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate the closed-form seed table on device");
	}
	e->d_seedt.resize(nk);
	for (size_t ki = 0; ki < nk; ++ki)
		if (!e->plain(ki) && !e->d_seedt[ki].upload(e->seeds[ki].blob)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate the spaced-seed table on device");
	e->adaptive = !(cfg->flags & NTC_FLAG_ALWAYS_LOG);
	e->partition_always = (cfg->flags & NTC_FLAG_PARTITION_ALWAYS) != 0;
	if (e->kernel_kind == KIND_HF && !(cfg->flags & NTC_FLAG_DIRECT_ATOMICS)) {
		// The log and the two partition work areas of the same total size (at the default of four entries per counter and rBits = 27:
		// 4 + 5.4 + 7 GiB) are allocated HERE, so that memory runs out at create time and not in the middle of a run; when it does, the
		// capacity is halved until it fits, and an engine that cannot even hold 2^18 entries increments with device atomics instead.
		uint64_t want = cfg->log_entries;
		while (plan_log(e.get(), want)) {
			if (e->d_log.reserve((size_t)e->all_log_regions() * e->log_region_cap * 4) && e->d_logfill.reserve((size_t)e->all_log_regions() * 4) &&
			    e->d_logmode.reserve(4) && e->d_logstats.reserve(24) && e->d_probe.reserve(4u << 20) && reserve_partition_scratch(e.get()))
				break;
			(void)hipGetLastError();
			for (auto* b : {&e->d_log, &e->d_logfill, &e->d_s1, &e->d_c1, &e->d_s2, &e->d_c2})
				b->reset();
			if (cfg->log_entries != 0) // an explicit request that does not fit is an error; otherwise: no log
				return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate the %llu-entry hit log and its partition areas on device", (unsigned long long)e->log_cap);
			if (e->log_cap <= (1ull << 18)) {
				e->log_regions = e->log_region_cap = e->klog_regions = 0;
				e->log_cap = 0;
				break;
			}
			want = e->log_cap / 2;
		}
	}
	// The tiled kernel pair K1h + K1f: every k of the list must be one K1h is generated for (k = 12 .. 32; ntcard's -g seed at k = 12 / gap 2 and k = 32 / gap 8); a list is
	// served by one launch per k over the same resident tiles.  Its hit-log keys and K1f's atomics are 32-bit counter indices.  Everything else —
	// row slots, other k, other seeds, nthll — is K1's (NTC_FLAG_LANE_KERNEL: tiled batches too, re-laid out as row slots).
	// A list may mix both kinds (`-k 16,24,32,48`, BASELINE config 4's `32,64,96,128`): K1h takes its k from the tiles, K1 stages the same tiles for the rest.
	// One strand: the canonical K1h walks both strands bit-sliced — without NTC_FLAG_STRAND_TILED no k of a strand engine is the pair's (tiled batches:
	// re-laid out, then K1).  With the flag the one-strand K1h kernels + K1f take the engine when EVERY plane is one of theirs; a list of which only a part
	// qualifies stays K1's as a whole (K1 has no one-strand instantiation that stages tiles).
	// NTC_FLAG_SIGNATURE: the 64-bit value is on hand in K1's resolve stage only — every plane of a signature engine is K1's, NTC_FLAG_STRAND_TILED or not.
	const bool strand_ok = e->strand == 0 || (cfg->flags & NTC_FLAG_STRAND_TILED);
	const bool ts_pre = e->kernel_kind == KIND_HF && !(cfg->flags & NTC_FLAG_LANE_KERNEL) && e->hll_bits == 0 && strand_ok && !e->sig &&
	                    nk * e->plane_elems() <= (1ull << 32);
	e->k_tiled.assign(nk, 0);
	e->ts_ok = false;
	e->ts_all = ts_pre;
	for (size_t ki = 0; ki < nk; ++ki) {
		e->k_tiled[ki] = ts_pre && (e->plain(ki) || e->kgap[ki] != 0) && ntc::sketch_k1h_supports(e->klist[ki], e->kgap[ki], e->s_bits, e->r_bits, e->strand) ? 1 : 0;
		e->ts_ok = e->ts_ok || e->k_tiled[ki];
		e->ts_all = e->ts_all && e->k_tiled[ki];
	}
	if (e->strand != 0 && !e->ts_all) { // a partly qualifying strand list: today's route for every k
		e->k_tiled.assign(nk, 0);
		e->ts_ok = false;
	}
	if (e->strand != 0 && e->ts_all)
		if (int rc = ensure_strand_kernel_attrs(e->device)) return rc;
	e->d_k1h_tabs.resize(nk);
	e->d_t4s.resize(nk);
	for (size_t ki = 0; ki < nk; ++ki) {
		if (!e->k_tiled[ki]) continue;
		const uint32_t k = e->klist[ki];
		std::vector<uint32_t> t4((size_t)ntc::t4_groups(k) * 256 * 4); // K1f: both strands' 64-bit terms, 4 bases per entry
		ntc::build_t4(k, t4.data(), e->plain(ki) ? nullptr : e->masks[ki].c_str());
		std::vector<uint32_t> tab((size_t)2 * ((k + 2) / 3) * 64);     // K1h's resolve pass: the low r_bits + sample bits, 3 bases per entry
		ntc::build_k1h_table(k, e->kgap[ki], e->r_bits, e->s_bits, tab.data());
		if (!e->d_t4s[ki].upload(t4) || !e->d_k1h_tabs[ki].upload(tab))
			return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate the closed-form tables of the tiled kernels on device");
	}
	if (e->sig)
		if (int rc = sig_setup(e.get())) return rc;
	e->ts_required = (cfg->flags & NTC_FLAG_REQUIRE_TILED) != 0;
	e->defer_redo = (cfg->flags & NTC_FLAG_DEFER_REDO) != 0;
	e->hfk.resize(nk);
	for (size_t ki = 0; ki < nk; ++ki)
		fill_hfk(e->hfk[ki], e->klist[ki], e->d_sketch + ki * e->plane_elems(), e->d_f1 + ki, e->d_t1[ki], (uint32_t)(ki * e->plane_elems()), e->strand);
	if (int rc = ntc_reset(e.get())) return rc;
	*out = e.release();
	return 0;
}

} // namespace

extern "C" {

uint32_t ntc_abi_version(void) { return NTC_ABI_VERSION; }
uint32_t ntc_max_k(void) { return kMaxK; }
const char* ntc_last_error(void) { return g_err.c_str(); }

int ntc_create(const ntc_config* cfg, ntc_engine** out)
{
	if (!cfg || !out) return fail(NTC_ERR_ARG, "ntc_create: null argument");
	*out = nullptr;
	if (cfg->n_k == 0 || cfg->n_k > NTC_MAX_K_LIST || !cfg->k)
		return fail(NTC_ERR_ARG, "ntc_create: need 1..%d k values", NTC_MAX_K_LIST);
	if (int rc = check_config(cfg)) return rc;
	std::vector<std::string> masks(cfg->n_k);
	if (cfg->gap != 0) masks[0] = ntc::gap_mask(cfg->k[0], cfg->gap); // "1"x(k-g)/2 "0"xg "1"x(k-g)/2, ntcard.cpp:407-413
	return create_engine(cfg, masks, false, out);
}

int ntc_create_seeded(const ntc_config* cfg, uint32_t n_seeds, const char* const* seeds, ntc_engine** out)
{
	if (!cfg || !out || !seeds) return fail(NTC_ERR_ARG, "ntc_create_seeded: null argument");
	*out = nullptr;
	if (cfg->n_k != 0 || cfg->k != nullptr || cfg->gap != 0)
		return fail(NTC_ERR_ARG, "ntc_create_seeded: n_k, k and gap of the config must be 0 (the k list is the seeds' lengths)");
	std::vector<std::string> masks;
	std::vector<uint32_t> ks;
	if (int rc = parse_masks("ntc_create_seeded", n_seeds, seeds, masks, ks)) return rc;
	bool spaced = false;
	for (const std::string& m : masks)
		spaced |= m.find('0') != std::string::npos;
	ntc_config c = *cfg;
	c.n_k = n_seeds;
	c.k = ks.data();
	if (int rc = check_config(&c)) return rc;
	if (spaced && (c.flags & NTC_FLAG_SIMPLE_KERNEL)) return fail(NTC_ERR_ARG, "ntc_create_seeded: spaced seeds need the production kernel");
	return create_engine(&c, masks, true, out);
}

int ntc_hll_create_ex(const ntc_hll_config* cfg, ntc_engine** out)
{
	if (!cfg || !out) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: null argument");
	*out = nullptr;
	// every argument first, the device afterwards
	constexpr uint32_t kHllFlags = NTC_FLAG_STRAND_FORWARD | NTC_FLAG_STRAND_REVERSE | NTC_FLAG_HPC;
	if (cfg->flags & ~kHllFlags)
		return fail(NTC_ERR_ARG, "ntc_hll_create_ex: unknown flag bits 0x%x (an nthll engine takes the strand flags and NTC_FLAG_HPC only)", cfg->flags & ~kHllFlags);
	if ((cfg->flags & NTC_FLAG_STRAND_FORWARD) && (cfg->flags & NTC_FLAG_STRAND_REVERSE))
		return fail(NTC_ERR_ARG, "ntc_hll_create_ex: NTC_FLAG_STRAND_FORWARD and NTC_FLAG_STRAND_REVERSE exclude each other");
	const bool has_k = cfg->n_k != 0 || cfg->k != nullptr, has_seeds = cfg->n_seeds != 0 || cfg->seeds != nullptr;
	if (has_k == has_seeds) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: need either a k list or a list of seeds, not %s", has_k ? "both" : "neither");
	std::vector<std::string> masks;
	std::vector<uint32_t> ks;
	if (has_k) {
		if (cfg->n_k == 0 || cfg->n_k > NTC_MAX_K_LIST || !cfg->k) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: need 1..%d k values", NTC_MAX_K_LIST);
		for (uint32_t i = 0; i < cfg->n_k; ++i)
			if (cfg->k[i] < 1 || cfg->k[i] > kMaxK) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: k=%u outside 1..%u", cfg->k[i], kMaxK);
		ks.assign(cfg->k, cfg->k + cfg->n_k);
		masks.assign(cfg->n_k, std::string());
	} else {
		if (!cfg->seeds) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: n_seeds = %u without seeds", cfg->n_seeds);
		if (int rc = parse_masks("ntc_hll_create_ex", cfg->n_seeds, cfg->seeds, masks, ks)) return rc;
	}
	if (cfg->n_bits < 4 || cfg->n_bits > 24) return fail(NTC_ERR_ARG, "ntc_hll_create_ex: n_bits %u outside 4..24", cfg->n_bits);
	EnginePtr e;
	if (int rc = new_engine("ntc_hll_create_ex", cfg->device, cfg->stream, e)) return rc;
	const size_t nk = ks.size();
	const uint32_t n_bits = cfg->n_bits;
	e->klist = ks;
	e->seeded = has_seeds;
	e->strand = (cfg->flags & NTC_FLAG_STRAND_FORWARD) ? 1u : (cfg->flags & NTC_FLAG_STRAND_REVERSE) ? 2u : 0u;
	e->hpc = (cfg->flags & NTC_FLAG_HPC) != 0;
	e->masks.assign(nk, std::string());
	e->kgap.assign(nk, 0u);
	e->seeds.assign(nk, ntc::SeedPlan());
	e->k_tiled.assign(nk, 0); // (no plane of an nthll engine is the tiled kernels')
	e->r_bits = 27;
	e->s_bits = 7;
	e->hll_bits = n_bits;
	e->kernel_kind = KIND_HF;
	for (size_t ki = 0; ki < nk; ++ki) {
		if (masks[ki].find('0') == std::string::npos) continue; // every position cared for: plain k-mers
		e->masks[ki] = masks[ki];
		e->kgap[ki] = symmetric_gap(masks[ki]);
		ntc::build_seed_plan(masks[ki], e->seeds[ki]);
		ntc::strand_seed_plan(e->seeds[ki], e->strand);
		e->max_seed_lds = std::max(e->max_seed_lds, seed_lds(e->seeds[ki]));
	}
	// plane ki: its own register file M[1 << n_bits] (uint32 on the device), its own F1 and its own threshold word
	if (!e->own_sketch.reserve((nk * sizeof(uint32_t)) << n_bits) || !e->own_f1.reserve(nk * 8) || !e->d_hll_thr.reserve(nk * 4))
		return fail(NTC_ERR_MEMORY, "ntc_hll_create_ex: device allocation failed");
	e->d_sketch = e->own_sketch;
	e->d_f1 = e->own_f1;
	e->d_t1.resize(nk);
	e->d_seedt.resize(nk);
	e->hfk.resize(nk);
	for (size_t ki = 0; ki < nk; ++ki) {
		std::vector<uint32_t> t1((size_t)ntc::t2_pairs(ks[ki]) * 64);
		ntc::build_t2(ks[ki], t1.data(), e->plain(ki) ? nullptr : e->masks[ki].c_str());
		ntc::strand_t2(ks[ki], t1.data(), e->strand);
		if (!e->d_t1[ki].upload(t1) || (!e->plain(ki) && !e->d_seedt[ki].upload(e->seeds[ki].blob)))
			return fail(NTC_ERR_MEMORY, "ntc_hll_create_ex: cannot allocate the seed tables on device");
		fill_hfk(e->hfk[ki], ks[ki], e->d_sketch + (ki << n_bits), e->d_f1 + ki, e->d_t1[ki], 0, e->strand);
	}
	if (int rc = ntc_reset(e.get())) return rc;
	*out = e.release();
	return 0;
}

// the one-k, canonical case of ntc_hll_create_ex
int ntc_hll_create(uint32_t k, uint32_t n_bits, int32_t device, void* stream, ntc_engine** out)
{
	if (!out) return fail(NTC_ERR_ARG, "ntc_hll_create: null argument");
	ntc_hll_config cfg;
	std::memset(&cfg, 0, sizeof cfg);
	cfg.n_k = 1;
	cfg.k = &k;
	cfg.n_bits = n_bits;
	cfg.device = device;
	cfg.stream = stream;
	return ntc_hll_create_ex(&cfg, out);
}

// everything the engine owns is freed by its members' destructors, once nothing of it is in flight any more
void ntc_destroy(ntc_engine* e)
{
	if (!e) return;
	(void)hipSetDevice(e->device);
	(void)hipStreamSynchronize(e->stream);
	e->mc.sync_lanes();
	delete e;
}

int ntc_reset(ntc_engine* e)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_reset: null engine");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (int rc = join_k1f(e)) return rc;
	HIP_TRY(hipMemsetAsync(e->d_sketch, 0, e->hll_bits ? (e->klist.size() * sizeof(uint32_t)) << e->hll_bits : e->klist.size() * e->plane_elems() * sizeof(uint32_t), e->stream));
	e->hll_reads_seen = 0;
	if (e->d_logfill) HIP_TRY(hipMemsetAsync(e->d_logfill, 0, (size_t)e->all_log_regions() * 4, e->stream));
	if (e->d_skdirty) HIP_TRY(hipMemsetAsync(e->d_skdirty, 0, 4, e->stream));
	e->sk_host_dirty = e->sk_exposed; // (a caller that has asked for the counters' address may write there at any time; ext_sketch: include/ntcard_hip.h)
	if (e->d_logmode) {
		HIP_TRY(hipMemsetAsync(e->d_logmode, 0, 4, e->stream));
		HIP_TRY(hipMemsetAsync(e->d_logstats, 0, 24, e->stream));
	}
	e->probed = false;
	e->log_pending = false;
	e->log_est = 0.0;
	HIP_TRY(hipMemsetAsync(e->d_f1, 0, e->klist.size() * 8, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (int rc = drain_events(e)) return rc;
	if (e->sig)
		if (int rc = sig_reset(e)) return rc;
	for (auto& t : e->timers) t.ms = 0.0, t.count = 0; // (drain_events has emptied their spans)
	e->applies = 0;
	e->long_pieces = e->long_seqs = 0;
	e->hpc_bytes_in = e->hpc_bytes_out = 0;
	return 0;
}

int ntc_sync(ntc_engine* e)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_sync: null engine");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (int rc = join_k1f(e)) return rc;   // (K1f reads the batches too)
	if (int rc = sig_flush(e)) return rc;  // (NTC_FLAG_SIGNATURE: the value log into the tables; a table that cannot grow fails here)
	HIP_TRY(hipStreamSynchronize(e->stream));
	return drain_events(e);
}

int ntc_flush(ntc_engine* e)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_flush: null engine");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return apply_log(e);
}

int ntc_finish(ntc_engine* e, uint16_t* t_counter_out, uint32_t* p_hist_out, uint64_t* f1_out)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_finish: null engine");
	if (e->hll_bits) return fail(NTC_ERR_STATE, "ntc_finish: this is an nthll engine, use ntc_hll_finish");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	const size_t nk = e->klist.size();
	const uint64_t per_sample = 1ull << e->r_bits;
	if (int rc = apply_log(e)) return rc; // pending increments first: compEst reads the counters (ntcard.cpp:240-247)
	if (int rc = sig_flush(e)) return rc;
	if (t_counter_out && !e->d_out16.reserve(2 * per_sample * sizeof(uint16_t))) return fail(NTC_ERR_MEMORY, "ntc_finish: cannot allocate uint16 staging");
	if (p_hist_out || t_counter_out) {
		HIP_TRY(hipMemsetAsync(e->d_phist, 0, nk * 2 * 65536 * 4, e->stream));
		for (size_t ki = 0; ki < nk; ++ki) {
			HIP_TRY(ntc::launch_finalize(e->d_sketch + ki * e->plane_elems(), per_sample,
			                             e->d_phist + ki * 2 * 65536, t_counter_out ? e->d_out16.get() : nullptr, e->stream));
			if (t_counter_out)
				HIP_TRY(hipMemcpyAsync(t_counter_out + ki * 2 * per_sample, e->d_out16, 2 * per_sample * sizeof(uint16_t),
				                       hipMemcpyDeviceToHost, e->stream));
		}
		if (p_hist_out)
			HIP_TRY(hipMemcpyAsync(p_hist_out, e->d_phist, nk * 2 * 65536 * 4, hipMemcpyDeviceToHost, e->stream));
	}
	if (f1_out) HIP_TRY(hipMemcpyAsync(f1_out, e->d_f1, nk * 8, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return drain_events(e);
}

int ntc_hll_finish(ntc_engine* e, uint8_t* regs_out, uint64_t* f1_out)
{
	if (!e || !e->hll_bits) return fail(NTC_ERR_STATE, "ntc_hll_finish: not an nthll engine");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	std::vector<uint32_t> regs(e->klist.size() << e->hll_bits); // every plane, in list order
	HIP_TRY(hipMemcpyAsync(regs.data(), e->d_sketch, regs.size() * 4, hipMemcpyDeviceToHost, e->stream));
	if (f1_out) HIP_TRY(hipMemcpyAsync(f1_out, e->d_f1, e->klist.size() * 8, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (regs_out)
		for (size_t i = 0; i < regs.size(); ++i)
			regs_out[i] = (uint8_t)regs[i];
	return drain_events(e);
}

int ntc_device_state(ntc_engine* e, void** d_sketch_u32, uint64_t* n_counters, void** d_f1_u64)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_device_state: null engine");
	{
		std::lock_guard<std::mutex> lk(e->mu);
		HIP_TRY(hipSetDevice(e->device));
		if (int rc = apply_log(e)) return rc; // the caller is about to read or reduce the counters
	}
	if (d_sketch_u32) {
		*d_sketch_u32 = e->d_sketch;
		e->sk_host_dirty = e->sk_exposed = true; // (the caller may add to the counters: nothing is known about them any more)
	}
	if (n_counters) *n_counters = e->klist.size() * e->plane_elems();
	if (d_f1_u64) *d_f1_u64 = e->d_f1;
	return 0;
}

namespace {
// the timing getters: drain the finished spans, then report a sum and (optionally) a count
int timing(ntc_engine* e, const char* who, Timer t, double* ms_out, uint64_t* count_out = nullptr)
{
	if (!e) return fail(NTC_ERR_ARG, "%s: null engine", who);
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (int rc = drain_events(e)) return rc;
	if (ms_out) *ms_out = e->timers[t].ms;
	if (count_out) *count_out = t == T_APPLY ? e->applies : e->timers[t].count;
	return 0;
}
} // namespace

int ntc_kernel_time(ntc_engine* e, double* ms_total, uint64_t* launches) { return timing(e, "ntc_kernel_time", T_HASH, ms_total, launches); }
int ntc_apply_time(ntc_engine* e, double* ms_total, uint64_t* applies) { return timing(e, "ntc_apply_time", T_APPLY, ms_total, applies); }
int ntc_fixup_time(ntc_engine* e, double* ms_total) { return timing(e, "ntc_fixup_time", T_K1F, ms_total); }

int ntc_merge_allocations(ntc_engine* e, uint64_t* n)
{
	if (!e || !n) return fail(NTC_ERR_ARG, "ntc_merge_allocations: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	*n = e->merge_allocs;
	return 0;
}

int ntc_long_stats(ntc_engine* e, uint64_t* pieces, uint64_t* sequences)
{
	if (!e || !pieces || !sequences) return fail(NTC_ERR_ARG, "ntc_long_stats: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	*pieces = e->long_pieces;
	*sequences = e->long_seqs;
	return 0;
}

int ntc_long_time(ntc_engine* e, double* cut_ms, double* gather_ms)
{
	if (int rc = timing(e, "ntc_long_time", T_LONG_CUT, cut_ms)) return rc;
	return timing(e, "ntc_long_time", T_LONG_GATHER, gather_ms);
}

int ntc_hpc_stats(ntc_engine* e, uint64_t* bytes_in, uint64_t* bytes_out)
{
	if (!e || !bytes_in || !bytes_out) return fail(NTC_ERR_ARG, "ntc_hpc_stats: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	*bytes_in = e->hpc_bytes_in;
	*bytes_out = e->hpc_bytes_out;
	return 0;
}

int ntc_hpc_time(ntc_engine* e, double* ms) { return timing(e, "ntc_hpc_time", T_HPC, ms); }

int ntc_update_mode(ntc_engine* e, uint32_t* mode_out)
{
	if (!e || !mode_out) return fail(NTC_ERR_ARG, "ntc_update_mode: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	*mode_out = 1; // engines without a log increment directly
	if (e->d_logmode) {
		HIP_TRY(hipMemcpyAsync(mode_out, e->d_logmode, 4, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	return 0;
}

int ntc_set_profiling(ntc_engine* e, int enable)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_set_profiling: null engine");
	std::lock_guard<std::mutex> lk(e->mu);
	e->profiling = enable != 0;
	return 0;
}

} // extern "C"
