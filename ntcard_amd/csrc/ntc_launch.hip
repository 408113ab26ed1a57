// ntc_launch.hip — everything that enters the engine's stream: the hash launches of row-slot and tiled batches, K1f, the sketch update, and the
// timed spans around them (ntc_engine.hpp).  Every function here runs under the engine's lock.
#include "ntc_engine.hpp"

namespace ntc_eng {

int device_cus(int dev, unsigned& out)
{
	static std::mutex mu;
	static std::vector<int> cus; // per device, queried once (hipGetDeviceProperties is slow)
	std::lock_guard<std::mutex> lk(mu);
	if (dev < 0) return fail(NTC_ERR_ARG, "bad device %d", dev);
	if ((size_t)dev >= cus.size()) cus.resize(dev + 1, 0);
	if (cus[dev] == 0) {
		hipDeviceProp_t p;
		HIP_TRY(hipGetDeviceProperties(&p, dev));
		cus[dev] = p.multiProcessorCount;
	}
	out = (unsigned)cus[dev];
	return 0;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel function, not of a launch: it
// is raised ONCE per device to the most any plan can ask for (under a process-wide lock), so that engines driven from
// different threads never lower each other's limit between "set" and "launch".
int ensure_kernel_attrs(int dev)
{
	static std::mutex mu;
	static std::vector<char> done;
	std::lock_guard<std::mutex> lk(mu);
	if ((size_t)dev >= done.size()) done.resize(dev + 1, 0);
	if (done[dev]) return 0;
	HIP_TRY(ntc::set_sketch_hf_smem_limit(kMaxDynLds));
	HIP_TRY(ntc::set_hash_smem_limit(kMaxDynLds));
	HIP_TRY(ntc::set_apply_smem_limit());
	HIP_TRY(ntc::set_sketch_k1h_smem_limit());
	done[dev] = 1;
	return 0;
}

// the one-strand K1h kernels' attribute, once per device, for the first engine that will launch them (NTC_FLAG_STRAND_TILED)
int ensure_strand_kernel_attrs(int dev)
{
	static std::mutex mu;
	static std::vector<char> done;
	std::lock_guard<std::mutex> lk(mu);
	if ((size_t)dev >= done.size()) done.resize(dev + 1, 0);
	if (done[dev]) return 0;
	HIP_TRY(ntc::set_sketch_k1h_strand_smem_limit());
	done[dev] = 1;
	return 0;
}

int hf_plan(int dev, uint64_t n_slots, uint32_t stride, const uint32_t* ks, uint32_t n_k, uint32_t seed_lds, HfPlan& p)
{
	unsigned cus = 0;
	if (int rc = device_cus(dev, cus)) return rc;
	size_t shared = 0;
	hf_shape(stride, ks, n_k, seed_lds, p, shared);
	if (p.waves_per_cu == 0)
		return fail(NTC_ERR_ARG, "slot stride %u with k=%u needs more than 160 KiB of LDS per wave", stride, ks[0]);
	p.smem = shared + p.wpb * (64u * (size_t)stride);
	if (p.smem > kMaxDynLds) return fail(NTC_ERR_ARG, "slot stride %u with k=%u needs %zu B of LDS per block", stride, ks[0], p.smem);
	const unsigned per_cu = std::max(1u, p.waves_per_cu / p.wpb);
	const uint64_t need = (n_slots + 64ull * p.wpb - 1) / (64ull * p.wpb);
	p.grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cus * per_cu));
	return 0;
}

// grid for the simple (validation) kernel: enough blocks to fill the chip, not more than the work
int hash_grid(int dev, uint64_t n_slots, uint32_t stride, unsigned& grid, size_t& smem)
{
	unsigned cus = 0;
	if (int rc = device_cus(dev, cus)) return rc;
	smem = smem_simple(stride);
	if (smem > kMaxDynLds) return fail(NTC_ERR_ARG, "slot stride %u needs %zu B of LDS per block (> 160 KiB)", stride, smem);
	const uint64_t need = (n_slots + 64 * ntc::kWavesPerBlock - 1) / (64 * ntc::kWavesPerBlock);
	grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(need, (uint64_t)cus * hash_blocks_per_cu(smem)));
	return 0;
}

// ---- timed spans ----
// opens `s` when the engine is profiling: at `borrow`, an event the stream has just recorded, or at an event of its own
int open_span(ntc_engine* e, Span& s, hipEvent_t borrow)
{
	if (!e->profiling) return 0;
	if (borrow) {
		s.ev0 = borrow;
		s.owns0 = false;
	} else {
		HIP_TRY(hipEventCreate(&s.ev0));
		HIP_TRY(hipEventRecord(s.ev0, e->stream));
	}
	return 0;
}

// closes an open span on `st` and files it under `into`; *recorded = its end event (null: the span was not open)
int close_span(Span& s, hipStream_t st, std::vector<Span>& into, hipEvent_t* recorded)
{
	if (recorded) *recorded = nullptr;
	if (!s.ev0) return 0;
	HIP_TRY(hipEventCreate(&s.ev1));
	HIP_TRY(hipEventRecord(s.ev1, st));
	if (recorded) *recorded = s.ev1;
	into.push_back(std::move(s));
	s = Span();
	return 0;
}

// the end of a bracketed run of tiled hash launches (ntc_engine::run)
int close_run(ntc_engine* e, hipEvent_t* recorded) { return close_span(e->run, e->stream, e->timers[T_HASH].spans, recorded); }

namespace {
int open_run(ntc_engine* e, hipEvent_t borrow = nullptr) // (borrow: the event a K1f in the middle of a k list has just left)
{
	if (!e->profiling || e->run.ev0) return 0;
	e->run.submits = 0; // (a bracket re-opened in the middle of a k list adds none: its submit is counted already)
	return open_span(e, e->run, borrow);
}
} // namespace

int drain_events(ntc_engine* e)
{
	if (int rc = close_run(e)) return rc;
	// every span first (a span may borrow its first event from another list's), then the events go
	for (auto& t : e->timers)
		for (const Span& s : t.spans) {
			float ms = 0.f;
			HIP_TRY(hipEventSynchronize(s.ev1));
			HIP_TRY(hipEventElapsedTime(&ms, s.ev0, s.ev1));
			t.ms += ms;
			t.count += s.submits;
		}
	for (auto& t : e->timers) t.spans.clear();
	return 0;
}

namespace {
int flush_deferred(ntc_engine* e) // the hash launches of the batches that wait in e->deferred
{
	if (e->deferred.empty() || e->in_flush) return 0;
	e->in_flush = true; // (run_tiled_segs calls join_k1f itself when it runs out of hand-over sets)
	std::vector<TiledSeg> segs;
	segs.swap(e->deferred);
	const int rc = run_tiled_segs(e, segs.data(), (uint32_t)segs.size(), segs.size());
	e->in_flush = false;
	return rc;
}
} // namespace

// K1f over the K1h launches that still wait for it (asynchronous on the engine's stream).  Before anything reads the counters or F1, touches the
// sketch without atomics (the apply's sweep does), or hands the batches back to the caller.
// *last = the event recorded behind the last thing this call launched (K1f's end, or the hash bracket's), or null
int join_k1f(ntc_engine* e, hipEvent_t* last)
{
	if (last) *last = nullptr;
	if (int rc = flush_deferred(e)) return rc;
	hipEvent_t closed = nullptr; // (the end of the hash launches' bracket, recorded this very moment, is K1f's start too)
	if (int rc = close_run(e, &closed)) return rc;
	if (last) *last = closed;
	if (e->k1f_n == 0) return 0;
	unsigned cus = 0;
	if (int rc = device_cus(e->device, cus)) return rc;
	Span sp;
	if (int rc = open_span(e, sp, closed)) return rc;
	const uint32_t n = e->k1f_n;
	e->k1f_n = 0;
	HIP_TRY(ntc::launch_k1h_fixup(e->k1f_batch, n, cus, e->stream));
	return close_span(sp, e->stream, e->timers[T_K1F].spans, last);
}

namespace {
// a log that this batch's `est` entries could fill up is applied first; then the entries are booked
int book_log(ntc_engine* e, double est)
{
	if (e->log_pending && e->log_est + est > 0.85 * (double)e->log_cap)
		if (int rc = apply_log(e)) return rc;
	e->log_est += est;
	e->log_pending = true;
	return 0;
}
} // namespace

// Apply the pending hit log to the sketch (asynchronous on the engine's stream): partition, count, add, clear.
int apply_log(ntc_engine* e)
{
	hipEvent_t before = nullptr; // (the event behind K1f / the hash bracket, if this call has just recorded one: the apply's start)
	if (int rc = join_k1f(e, &before)) return rc;
	if (!e->d_log || !e->log_pending) return 0;
	const auto& ap = e->ap;
	const uint32_t nb1 = 1u << ap.b1, nb2 = 1u << ap.b2;
	const size_t runs1 = (size_t)ap.g1 * nb1, runs2 = (size_t)nb1 * ap.parts2 * nb2;
	if (ap.b1 && !e->d_s1 && !(e->d_s1.reserve(runs1 * ap.cap1 * ap.key_bytes(1)) && e->d_c1.reserve(runs1 * 4)))
		return fail(NTC_ERR_MEMORY, "cannot allocate %zu B of partition scratch on device", runs1 * ap.cap1 * ap.key_bytes(1));
	if (ap.b2 && !e->d_s2 && !(e->d_s2.reserve(runs2 * ap.cap2 * ap.key_bytes(2)) && e->d_c2.reserve(runs2 * 4)))
		return fail(NTC_ERR_MEMORY, "cannot allocate %zu B of partition scratch on device", runs2 * ap.cap2 * ap.key_bytes(2));
	Span sp;
	if (int rc = open_span(e, sp, before)) return rc;
	// little in the log (decided on the device: fewer than 4 M entries): plain atomics, and the passes below find it empty
	// (an engine whose every k is K1h's always logs, so the host's estimate of a large log is good enough to go straight to the partition passes — which are exact
	// for a small log too, only slower —: two tiny kernels and a stream bubble less per apply)
	if (!e->partition_always && !(e->ts_all && e->log_est >= (double)(64u << 20)))
		HIP_TRY(ntc::launch_log_atomics(e->d_log, e->d_logfill, e->log_region_cap, e->all_log_regions(), (uint32_t*)(e->d_logstats + 2), e->d_sketch, e->d_skdirty, e->stream));
	ntc::CountArgs c;
	std::memset(&c, 0, sizeof c);
	c.slice_bits = ap.slice_bits;
	c.n_slices = ap.n_slices;
	c.sketch = e->d_sketch;
	c.first = e->sk_host_dirty ? 0u : 1u; // nothing the host knows of has touched the sketch since the reset: the device word decides
	c.sk_dirty = e->d_skdirty;
	if (ap.b1 == 0) {
		c.in = e->d_log;
		c.in_cnt = e->d_logfill;
		c.in_cap = e->log_region_cap;
		c.n_in = e->all_log_regions();
		c.mode = 0;
	} else {
		ntc::SplitArgs s1;
		std::memset(&s1, 0, sizeof s1);
		s1.in = e->d_log;
		s1.in_cnt = e->d_logfill;
		s1.in_cap = e->log_region_cap;
		s1.n_in = e->all_log_regions();
		s1.mode = 0;
		s1.sk_dirty = e->d_skdirty;
		s1.shift = ap.key_bits - ap.b1;
		s1.bits = ap.b1;
		s1.out = e->d_s1;
		s1.out_cnt = e->d_c1;
		s1.out_cap = ap.cap1;
		s1.sketch = e->d_sketch;
		s1.narrow = ap.b2 == 0;
		// between two passes the keys travel three to a 64-bit word (what the first pass leaves of a key is <= 21 bits: 2.7 B per key written and
		// read instead of 4; the run's capacity in words is half its capacity in keys — the same bytes)
		const bool packed = ap.b2 != 0 && ap.key_bits - ap.b1 <= 21;
		if (packed) {
			s1.pack_out = 1;
			s1.out_cap = ap.cap1 / 2;
		}
		HIP_TRY(ntc::launch_split(s1, ap.g1, e->stream));
		if (ap.b2 == 0) {
			c.in = e->d_s1;
			c.in_cnt = e->d_c1;
			c.in_cap = ap.cap1;
			c.n_in = ap.g1 * nb1;
			c.mode = 1;
			c.nb1 = nb1;
			c.nwg1 = ap.g1;
			c.in16 = 1;
		} else {
			ntc::SplitArgs s2;
			std::memset(&s2, 0, sizeof s2);
			s2.in = e->d_s1;
			s2.in_cnt = e->d_c1;
			s2.in_cap = ap.cap1;
			s2.n_in = ap.g1 * nb1;
			s2.mode = 1;
			s2.parts = ap.parts2;
			s2.nb_in = nb1;
			s2.shift = ap.slice_bits;
			s2.bits = ap.b2;
			s2.out = e->d_s2;
			s2.out_cnt = e->d_c2;
			s2.out_cap = ap.cap2;
			s2.sketch = e->d_sketch;
			s2.sk_dirty = e->d_skdirty;
			s2.narrow = 1;
			if (packed) {
				s2.pack_in = 1;
				s2.in_cap = ap.cap1 / 2;
				s2.hi_shift = ap.key_bits - ap.b1;
			}
			HIP_TRY(ntc::launch_split(s2, nb1 * ap.parts2, e->stream));
			c.in = e->d_s2;
			c.in_cnt = e->d_c2;
			c.in_cap = ap.cap2;
			c.n_in = nb1 * ap.parts2 * nb2;
			c.mode = 2;
			c.parts = ap.parts2;
			c.nb2 = nb2;
			c.in16 = 1;
		}
	}
	unsigned cus = 0;
	if (int rc = device_cus(e->device, cus)) return rc;
	if (c.mode != 0) { // (the count pass reads partition runs, not the log: it clears the log's fill words itself)
		c.clear_fill = e->d_logfill;
		c.n_clear = e->all_log_regions();
	}
	HIP_TRY(ntc::launch_count(c, std::min<unsigned>(ap.n_slices, (ap.slice_bits >= 15 ? 2u : 4u) * cus), e->stream));
	e->sk_host_dirty = true;
	if (c.mode == 0) HIP_TRY(hipMemsetAsync(e->d_logfill, 0, (size_t)e->all_log_regions() * 4, e->stream));
	if (int rc = close_span(sp, e->stream, e->timers[T_APPLY].spans)) return rc;
	e->log_pending = false;
	e->log_est = 0.0;
	e->applies += 1;
	return 0;
}

// ---- row-slot batches ----
namespace {
struct SlotBatch {
	const unsigned char* slots;
	const uint32_t* meta;
	uint64_t n;
	uint32_t read_len, stride;
	bool tiled;
};

// nthll: refresh the "can still matter" threshold between sub-batches that double in size, so the
// expensive resolve stage only sees a vanishing fraction of the k-mers once the registers warm up.
// Planes: one launch per plane per sub-batch, each against its own threshold word, refreshed from that plane's registers (DESIGN.md §4 "nthll forms").
int run_hll(ntc_engine* e, const SlotBatch& b)
{
	const size_t nk = e->klist.size();
	std::vector<HfPlan> plans(nk); // every plane's launch shape first (waves per CU do not depend on the slot count): a mask whose tables do not fit fails HERE, nothing counted
	for (size_t ki = 0; ki < nk; ++ki)
		if (int rc = hf_plan(e->device, std::min<uint64_t>(b.n, 16384), b.stride, &e->klist[ki], 1, seed_lds(e->seeds[ki]), plans[ki])) return rc;
	for (uint64_t done = 0; done < b.n;) {
		uint64_t n = std::max<uint64_t>(16384, e->hll_reads_seen);
		n = std::min<uint64_t>((n + 63) & ~63ull, b.n - done); // whole waves: a sub-batch starts on a 16-byte aligned slot
		for (size_t ki = 0; ki < nk; ++ki) {
			uint32_t* const regs = e->d_sketch + (ki << e->hll_bits);
			HIP_TRY(ntc::launch_hll_threshold(regs, 1u << e->hll_bits, e->d_hll_thr + ki, e->stream));
			ntc::HfArgs a;
			std::memset(&a, 0, sizeof a);
			a.slots = b.slots + done * b.stride;
			a.meta = b.meta ? b.meta + done : nullptr;
			a.n_slots = n;
			a.stride = b.stride;
			a.read_len = b.read_len;
			a.r_bits = 27;
			a.s_bits = 7;
			a.n_k = 1;
			a.hll_bits = e->hll_bits;
			a.hll_thr = e->d_hll_thr + ki;
			if (!e->plain(ki)) set_seed_args(a, e->seeds[ki], e->d_seedt[ki]);
			a.ks[0] = e->hfk[ki];
			HfPlan hp;
			if (int rc = hf_plan(e->device, n, b.stride, &e->klist[ki], 1, seed_lds(e->seeds[ki]), hp)) return rc;
			HIP_TRY(ntc::launch_sketch_hf(a, hp.grid, hp.wpb, hp.smem, e->stream));
		}
		done += n;
		e->hll_reads_seen += n;
	}
	return 0;
}

// K1 over the k [first, first + n) of the list: one launch (the batch is staged and decoded once per group); a group whose closed-form tables would
// push the CU below 12 waves (and below what its members reach alone) is split in two
int launch_k1_group(ntc_engine* e, const SlotBatch& b, size_t first, size_t n)
{
	HfPlan hp;
	if (int rc = hf_plan(e->device, b.n, b.stride, &e->klist[first], (uint32_t)n, seed_lds(e->seeds[first]), hp)) {
		if (n == 1) return rc;
		hp.waves_per_cu = 0;
	}
	unsigned worst_single = 16; // waves per CU of the least favourable member launched on its own
	for (size_t j = 0; n > 1 && j < n; ++j) {
		HfPlan one;
		size_t sh;
		hf_shape(b.stride, &e->klist[first + j], 1, seed_lds(e->seeds[first + j]), one, sh);
		worst_single = std::min(worst_single, one.waves_per_cu);
	}
	if (n > 1 && hp.waves_per_cu < 12 && hp.waves_per_cu < worst_single) {
		if (int rc = launch_k1_group(e, b, first, n / 2)) return rc;
		return launch_k1_group(e, b, first + n / 2, n - n / 2);
	}
	ntc::HfArgs a;
	std::memset(&a, 0, sizeof a);
	a.slots = b.slots;
	a.meta = b.meta;
	a.n_slots = b.n;
	a.stride = b.stride;
	a.read_len = b.read_len;
	a.tiled = b.tiled ? 1u : 0u;
	a.r_bits = e->r_bits;
	a.s_bits = e->s_bits;
	a.n_k = (uint32_t)n;
	if (!e->plain(first)) set_seed_args(a, e->seeds[first], e->d_seedt[first]);
	for (size_t j = 0; j < n; ++j)
		a.ks[j] = e->hfk[first + j];
	if (e->d_log) {
		a.log = e->d_log;
		a.log_fill = e->d_logfill;
		a.log_regions = e->log_regions;
		a.log_region_cap = e->log_region_cap;
		a.log_mode = e->d_logmode;
	}
	a.sketch0 = e->d_sketch;
	a.sk_dirty = e->d_skdirty;
	if (e->sig) sig_args(e, a, first, n);
	HIP_TRY(ntc::launch_sketch_hf(a, hp.grid, hp.wpb, hp.smem, e->stream));
	return 0;
}

int run_k1(ntc_engine* e, const SlotBatch& b, const std::vector<uint8_t>* skip)
{
	auto mine = [&](size_t ki) { return !(skip && (*skip)[ki]); };
	if (e->sig) {
		// NTC_FLAG_SIGNATURE: a plane's value log must hold every WINDOW of a launch (ntc_signature.hip) — a batch with more is counted in several launches
		const uint32_t len = b.meta ? b.stride : b.read_len, kmin = *std::min_element(e->klist.begin(), e->klist.end());
		const uint64_t per = len >= kmin ? (uint64_t)(len - kmin + 1u) : 1u, max_slots = sig_max_slots(e, per);
		if (b.n > max_slots) {
			for (uint64_t done = 0; done < b.n; done += max_slots)
				if (int rc = run_batch(e, b.slots + done * b.stride, b.meta ? b.meta + done : nullptr, std::min<uint64_t>(max_slots, b.n - done), b.read_len, b.stride, b.tiled, skip))
					return rc;
			return 0;
		}
	}
	double per_slot = 0.0;
	for (size_t ki = 0; ki < e->klist.size(); ++ki)
		if (mine(ki)) per_slot += sampled_per_read(b.meta ? b.stride : b.read_len, e->klist[ki], e->s_bits);
	// the probe's head first (probe_head_reads); a batch that is not several heads long (large sBits, small batches) is not cut: the probe then
	// runs once enough has been logged
	if (e->d_log && e->adaptive && !e->probed && b.meta == nullptr && per_slot > 0.0) {
		const uint64_t head = probe_head_reads(per_slot);
		if (e->log_est < (double)(1u << 20) && b.n >= 4 * head) {
			if (int rc = run_batch(e, b.slots, nullptr, head, b.read_len, b.stride, b.tiled, skip)) return rc;
			return run_batch(e, b.slots + head * b.stride, nullptr, b.n - head, b.read_len, b.stride, b.tiled, skip);
		}
	}
	if (e->sig) { // (behind the probe's cut: every launch books itself)
		const uint32_t len = b.meta ? b.stride : b.read_len, kmin = *std::min_element(e->klist.begin(), e->klist.end());
		if (int rc = sig_book(e, sig_need(e, b.n, len >= kmin ? (uint64_t)(len - kmin + 1u) : 1u))) return rc;
	}
	// this batch's sampled k-mers + what every wave may leave unused at the end of a region
	if (e->d_log)
		if (int rc = book_log(e, 64.0 * 4096 + (double)b.n * per_slot)) return rc;
	Span sp; // the hash kernels of this batch only: an apply has its own span
	if (int rc = open_span(e, sp)) return rc;
	for (size_t first = 0; first < e->klist.size();) { // runs of this call's k, up to kMaxFusedK per launch (a spaced seed: a launch of its own)
		if (!mine(first)) {
			++first;
			continue;
		}
		size_t n = 1;
		while (n < ntc::kMaxFusedK && first + n < e->klist.size() && mine(first + n) && e->plain(first) && e->plain(first + n))
			++n;
		if (int rc = launch_k1_group(e, b, first, n)) return rc;
		first += n;
	}
	if (int rc = close_span(sp, e->stream, e->timers[T_HASH].spans)) return rc;
	if (e->d_log && e->adaptive && !e->probed && e->log_est >= (double)(1u << 20)) { // enough logged since the reset: sample the log, decide log vs atomics
		e->probed = true;
		HIP_TRY(ntc::launch_log_probe(e->d_log, e->d_logfill, e->log_region_cap, std::min<uint32_t>(e->log_regions, 1024), 256, e->d_probe, 1u << 20,
		                              e->d_logstats, e->d_logmode, e->stream));
	}
	return 0;
}

int run_simple(ntc_engine* e, const SlotBatch& b) // the validation kernel: one launch per k
{
	unsigned grid = 0;
	size_t smem = 0;
	if (int rc = hash_grid(e->device, b.n, b.stride, grid, smem)) return rc;
	for (size_t ki = 0; ki < e->klist.size(); ++ki) {
		ntc::HashArgs a;
		std::memset(&a, 0, sizeof a);
		a.slots = b.slots;
		a.meta = b.meta;
		a.n_slots = b.n;
		a.stride = b.stride;
		a.read_len = b.read_len;
		a.k = e->klist[ki];
		a.r_bits = e->r_bits;
		a.s_bits = e->s_bits;
		a.sketch = e->d_sketch + ki * e->plane_elems();
		a.f1 = e->d_f1 + ki;
		ntc::build_tables(a.k, a.tab);
		ntc::poly_a_state(a.k, a.init);
		a.strand = e->strand;
		a.t1 = e->d_t1[ki]; // (the simple kernel has no spaced seeds: ntc_create refuses them with NTC_FLAG_SIMPLE_KERNEL)
		Span sp;
		if (int rc = open_span(e, sp)) return rc;
		HIP_TRY(ntc::launch_hash(0, a, grid, smem, e->stream));
		if (int rc = close_span(sp, e->stream, e->timers[T_HASH].spans)) return rc;
	}
	return 0;
}
} // namespace

int run_batch(ntc_engine* e, const unsigned char* d_slots, const uint32_t* d_meta, uint64_t n_slots, uint32_t read_len, uint32_t stride, bool tiled,
              const std::vector<uint8_t>* skip)
{
	if (n_slots == 0) return 0;
	if (int rc = close_run(e)) return rc;
	const SlotBatch b{d_slots, d_meta, n_slots, read_len, stride, tiled};
	if (e->kernel_kind != KIND_HF) return run_simple(e, b);
	return e->hll_bits ? run_hll(e, b) : run_k1(e, b, skip);
}

// ---- tiled batches: K1h + K1f (include/ntcard_hip.h: ntc_submit_tiled_device), K1 for the k they are not built for ----
namespace {
// the slot table (len | len << 16 per read) of a ragged tiled batch, for K1
int tiled_meta(ntc_engine* e, const TiledSeg& sg, const uint32_t** d_meta)
{
	if ((size_t)sg.n_reads * 4 > e->d_tmeta.cap) {
		HIP_TRY(hipStreamSynchronize(e->stream));
		if (!e->d_tmeta.reserve((size_t)sg.n_reads * 4, 4u << 20)) return fail(NTC_ERR_MEMORY, "cannot allocate the slot table of a ragged tiled batch on device");
	}
	HIP_TRY(ntc::launch_tails_to_meta(sg.d_tails, sg.n_reads, (sg.read_len + 15u) / 16u, e->d_tmeta, e->stream));
	*d_meta = e->d_tmeta;
	return 0;
}

// a tiled batch for K1: re-laid out as row-major slots on the device (exact; not a fast path).  d_meta: the reads' lengths of a ragged batch
// (tiled_meta); skip: the k of the list that are not this call's
int run_tiled_as_rows(ntc_engine* e, const TiledSeg& sg, const uint32_t* d_meta = nullptr, const std::vector<uint8_t>* skip = nullptr)
{
	const uint32_t stride = pick_stride(sg.read_len, e->klist, e->max_seed_lds);
	const size_t need = (size_t)sg.n_reads * stride + 16;
	if (need > e->d_untile.cap) {
		HIP_TRY(hipStreamSynchronize(e->stream));
		if (!e->d_untile.reserve(need)) return fail(NTC_ERR_MEMORY, "cannot allocate %zu B of row-major scratch on device", need);
	}
	HIP_TRY(ntc::launch_untile(sg.d_tiles, e->d_untile, sg.n_reads, sg.read_len, stride, e->stream));
	return run_batch(e, e->d_untile, d_meta, sg.n_reads, sg.read_len, stride, false, skip);
}

using Segs = std::vector<TiledSeg>;

// Step 1, validate and route: true = the batches were refused or went to K1 as a whole (rc says how that ended)
bool route_tiled(ntc_engine* e, const Segs& segs, bool any_tails, int& rc)
{
	rc = 0;
	if (!e->ts_all && e->ts_required)
		rc = fail(NTC_ERR_ARG, "ntc_submit_tiled_device: the tiled kernel is not available for this configuration (NTC_FLAG_REQUIRE_TILED)");
	else if (!e->ts_ok && any_tails && !e->seeded && e->strand == 0 && !e->sig) // (a strand or signature engine is K1's by contract: its ragged batches are re-laid out)
		rc = fail(NTC_ERR_ARG, "ntc_submit_tiled_ragged_device: the tiled kernels are not built for any k of this configuration");
	else if (!e->ts_ok) { // this configuration is K1's
		for (size_t i = 0; i < segs.size() && !rc; ++i) {
			const uint32_t* d_meta = nullptr;
			if (segs[i].d_tails) rc = tiled_meta(e, segs[i], &d_meta);
			if (!rc) rc = run_tiled_as_rows(e, segs[i], d_meta);
		}
	} else if (!e->ts_all) {
		for (const auto& sg : segs)
			if (!k1_fits_tiles(e, sg.read_len)) {
				rc = fail(NTC_ERR_ARG, "tiled batch of %u-base reads: the k of this list that the general kernel serves cannot stage such tiles in LDS (submit the reads through ntc_submit / ntc_submit_spans, which cut long sequences into chunks); nothing was counted", sg.read_len);
				return true;
			}
		return false;
	} else {
		return false;
	}
	return true;
}

// Step 2, split: more bins than one launch takes go in groups; a batch beyond K1h's 32-bit offsets goes in halves.  true = done that way
bool split_tiled(ntc_engine* e, const Segs& segs, uint32_t max_segs, bool k1f_now, int& rc)
{
	rc = 0;
	if (segs.size() > max_segs) {
		for (size_t i = 0; i < segs.size() && !rc; i += max_segs)
			rc = run_tiled_segs(e, segs.data() + i, (uint32_t)std::min<size_t>(max_segs, segs.size() - i), 1, k1f_now);
		return true;
	}
	for (const auto& sg : segs) {
		// K1h addresses its bit arrays (one word per tile, chunk / block and lane) with 32-bit byte offsets: a batch of several hundred GB is cut in
		// two at a tile boundary, as often as it takes (any prefix of a tiled buffer is a batch)
		const uint64_t n_tiles = (sg.n_reads + ntc::kTileReads - 1) / ntc::kTileReads;
		const uint64_t rows = (uint64_t)(sg.read_len + 15u) / 16u + 2u; // chunks, and at most chunks + 1 blocks, per tile
		if (n_tiles * rows * 256u < (1ull << 32)) continue;
		for (const auto& s2 : segs) { // (such a set of batches goes one by one, halves first)
			if (rc) break;
			if (&s2 != &sg) {
				rc = run_tiled_segs(e, &s2, 1, 1, k1f_now);
				continue;
			}
			const uint64_t head_tiles = n_tiles / 2, head_reads = head_tiles * ntc::kTileReads;
			const TiledSeg head{sg.d_tiles, head_reads, sg.read_len, sg.d_tails, sg.cut_k};
			const TiledSeg rest{sg.d_tiles + ntc_tiled_bytes(head_reads, sg.read_len), sg.n_reads - head_reads, sg.read_len, sg.d_tails ? sg.d_tails + head_tiles * 16 : nullptr, sg.cut_k};
			rc = run_tiled_segs(e, &head, 1, 1, k1f_now);
			if (!rc) rc = run_tiled_segs(e, &rest, 1, 1, k1f_now);
		}
		return true;
	}
	return false;
}

// Step 3, the probe's head.  A list of which a part is K1's: K1 appends to the hit log or increments with device atomics, whichever the probe of the FIRST
// sizeable batch finds cheaper for this data (run_k1).  The probe needs a log whose sampled entries come from few reads — the head of the batch, hashed by
// both kernels before the rest: the batch is cut as run_k1 cuts a row-slot batch.  true = done that way
bool probe_head_tiled(ntc_engine* e, const Segs& segs, bool k1f_now, int& rc)
{
	if (e->ts_all || !e->d_log || !e->adaptive || e->probed || segs.size() != 1 || segs[0].d_tails || !(e->log_est < (double)(1u << 20))) return false;
	const TiledSeg& sg = segs[0];
	double per_read = 0.0;
	for (uint32_t k : e->klist)
		per_read += sampled_per_read(sg.len_for(k), k, e->s_bits);
	if (!(per_read > 0.0)) return false;
	const uint64_t head = probe_head_reads(per_read);
	if (sg.n_reads < 4 * head) return false;
	const TiledSeg first{sg.d_tiles, head, sg.read_len, nullptr, sg.cut_k};
	const TiledSeg rest{sg.d_tiles + ntc_tiled_bytes(head, sg.read_len), sg.n_reads - head, sg.read_len, nullptr, sg.cut_k};
	rc = run_tiled_segs(e, &first, 1, 1, k1f_now);
	if (!rc) rc = run_tiled_segs(e, &rest, 1, 1, k1f_now);
	return true;
}

// One K1h k of a call: the batches with a window of this k (none in a shorter read, ntHashIterator.hpp:61-64) and their share of the launch, planned ONCE —
// the hand-over sets are sized from it and the launch fills in the rest of hs.  hs[i].read_len is the batch's length FOR THIS k (TiledSeg::len_for: pieces of
// long sequences under a list are trimmed, their chunks are not); blocks, nb_magic, the hand-over arrays and K1f's arguments all follow from it
struct K1hPlan {
	size_t ki;
	uint32_t na;
	const TiledSeg* act[ntc::kK1hSegs];
	ntc::K1hArgs hs[ntc::kK1hSegs];
};
// what a hand-over set must hold for the most demanding k of the list: sized before the first launch, so that the sets of a deferring engine never
// grow in the middle of a run
struct K1hNeed {
	size_t dirty = 0, tie = 0, sus = 0; // bytes
	uint32_t sus_cap = 0;               // suspects per wave
	uint32_t max_waves = 0;
};

void plan_k1h(const ntc_engine* e, const Segs& segs, unsigned cus, std::vector<K1hPlan>& plans, K1hNeed& need)
{
	need.max_waves = cus * ntc::sketch_k1h_waves(); // (one workgroup per CU)
	for (size_t ki = 0; ki < e->klist.size(); ++ki) {
		const uint32_t k = e->klist[ki];
		if (!e->k_tiled[ki]) continue; // K1's
		K1hPlan p;
		p.ki = ki;
		p.na = 0;
		std::memset(p.hs, 0, sizeof p.hs);
		for (const auto& sg : segs)
			if (sg.len_for(k) >= k) {
				p.hs[p.na].n_tiles = (uint32_t)((sg.n_reads + ntc::kTileReads - 1) / ntc::kTileReads);
				p.hs[p.na].read_len = sg.len_for(k);
				p.act[p.na++] = &sg;
			}
		if (p.na == 0) continue;
		ntc::K1hArgs shares[ntc::kK1hSegs];
		(void)ntc::plan_sketch_k1h(p.hs, p.na, k, cus, shares);
		for (uint32_t i = 0; i < p.na; ++i) {
			const uint32_t n_chunks = (p.act[i]->read_len + 15u) / 16u, nb = ntc::sketch_k1h_blocks(k, p.hs[i].read_len);
			need.dirty = std::max(need.dirty, (size_t)p.hs[i].n_tiles * n_chunks * 256);
			need.tie = std::max(need.tie, (size_t)p.hs[i].n_tiles * nb * 256);
			need.sus_cap = std::max(need.sus_cap, k1h_suspects_per_wave(shares[i].blocks_per_wave, e->s_bits, need.max_waves));
		}
		plans.push_back(p);
	}
	if (const char* ev = std::getenv("NTC_K1H_SUS_CAP")) { // tests: a short list forces the overflow path
		const long v = std::strtol(ev, nullptr, 10);
		if (v >= 1 && v <= (long)need.sus_cap) need.sus_cap = (uint32_t)v;
	}
	need.sus = (size_t)need.max_waves * need.sus_cap * 16;
}

// with_sus: the first set of a launch holds the launch's suspect list
bool set_too_small(const ntc_engine::K1hSet& s, const K1hNeed& need, bool with_sus)
{
	return need.dirty > s.d_dirty.cap || need.tie > s.d_tie.cap || (with_sus && need.sus > s.d_sus.cap);
}

// the hand-over arrays of one set (K1h + K1f: the two bit arrays between them and the suspect list are scratch of a launch pair)
int ensure_set(ntc_engine* e, ntc_engine::K1hSet& s, const K1hNeed& need, bool with_sus)
{
	if (set_too_small(s, need, with_sus)) HIP_TRY(hipStreamSynchronize(e->stream));
	if (!s.d_dirty.reserve(need.dirty) || !s.d_tie.reserve(need.tie))
		return fail(NTC_ERR_MEMORY, "cannot allocate %zu B of scratch for the tiled kernel on device", need.dirty + need.tie);
	if (with_sus && !s.d_sus.reserve(need.sus))
		return fail(NTC_ERR_MEMORY, "cannot allocate the %zu-byte suspect list of the tiled kernel on device", need.sus);
	if (!s.d_sus_count) {
		if (!s.d_sus_count.reserve((size_t)need.max_waves * 4) || !s.d_fix_state.reserve(16))
			return fail(NTC_ERR_MEMORY, "cannot allocate the suspect list of the tiled kernel on device");
		HIP_TRY(hipMemsetAsync(s.d_fix_state, 0, 16, e->stream));
		HIP_TRY(hipMemsetAsync(s.d_sus_count, 0, (size_t)need.max_waves * 4, e->stream));
	}
	return 0;
}

// Step 5, the hand-over sets of the `na` launches from set e->k1f_n on.  An engine that defers K1f sizes ALL its sets at the first launch of a batch
// geometry (a set that grows later would stall the stream in the middle of a run).  no_room: it was a set that failed (not the K1f in front of it)
int ensure_sets(ntc_engine* e, uint32_t na, const K1hNeed& need, bool defer, bool& no_room)
{
	no_room = false;
	bool grow = false;
	for (uint32_t i = 0; i < na; ++i) {
		const auto& s = e->k1h_set[e->k1f_n + i];
		grow |= set_too_small(s, need, i == 0) || !s.d_sus_count;
	}
	if (!grow) return 0;
	if (e->k1f_n != 0) // the sets ahead are in use by launches whose K1f is still to come
		if (int rc = join_k1f(e)) return rc;
	for (uint32_t si = 0; si < (defer ? ntc::kK1fBatch : na); ++si) // (launches of one batch each — K1's share of a list, single submits — may start at any set)
		if (int rc = ensure_set(e, e->k1h_set[si], need, si == 0 || na == 1)) {
			no_room = true;
			return rc;
		}
	return 0;
}

// Step 6, one K1h launch over the batches of p; its K1f follows at once unless `defer`
int launch_k1h(ntc_engine* e, K1hPlan& p, const K1hNeed& need, unsigned cus, bool defer)
{
	const size_t ki = p.ki;
	const uint32_t k = e->klist[ki], na = p.na;
	for (uint32_t i = 0; i < na; ++i) {
		auto& set = e->k1h_set[e->k1f_n + i];
		ntc::K1hArgs& h = p.hs[i];
		h.sus = e->k1h_set[e->k1f_n].d_sus; // (the launch's list: that of its first set)
		h.sus_count = e->k1h_set[e->k1f_n].d_sus_count;
		h.sus_cap = need.sus_cap; // (<= the allocation's)
		h.launch_id = ++e->k1h_launch_id;
		if (h.launch_id == 0) h.launch_id = ++e->k1h_launch_id;
		h.fix_state = set.d_fix_state;
		h.tiles = p.act[i]->d_tiles;
		h.log = e->d_log;
		h.log_fill = e->d_logfill;
		h.sketch0 = e->d_sketch;
		h.sk_dirty = e->d_skdirty;
		h.f1 = e->d_f1 + ki;
		h.dirty = set.d_dirty;
		h.tie = set.d_tie;
		h.n_chunks = (p.act[i]->read_len + 15u) / 16u;
		h.nv_last = (uint32_t)(p.act[i]->n_reads - (uint64_t)(h.n_tiles - 1) * ntc::kTileReads);
		h.key_base = (uint32_t)(ki * e->plane_elems());
		h.rmask2 = (uint32_t)((2ull << e->r_bits) - 1ull);
		h.log_regions = e->d_log ? e->log_regions : 0u;
		h.log_region_cap = e->log_region_cap;
		h.table = e->d_k1h_tabs[ki];
		h.s_bits = e->s_bits;
		h.r_bits = e->r_bits;
		h.tails = p.act[i]->d_tails;
	}
	ntc::K1hArgs launched[ntc::kK1hSegs];
	uint32_t n_waves = 0;
	if (int rc = open_run(e)) return rc; // (a K1f in ensure_sets may have closed the bracket)
	HIP_TRY(ntc::launch_sketch_k1h_multi(p.hs, na, k, e->kgap[ki], cus, e->stream, launched, &n_waves, e->strand));
	for (uint32_t i = 0; i < na; ++i) {
		auto& it = e->k1f_batch.item[e->k1f_n++];
		it.a = launched[i];
		it.t4 = e->d_t4s[ki];
		it.k = k;
		it.n_waves = launched[i].n_wg * ntc::sketch_k1h_waves(); // (its suspect regions: those of the workgroups that walked it)
		it.klog = e->d_log ? e->d_log + (size_t)e->log_regions * e->log_region_cap : nullptr;
		it.klog_fill = e->d_log ? e->d_logfill + e->log_regions : nullptr;
		it.klog_n = e->d_log ? e->klog_regions : 0u;
		it.klog_cap = e->log_region_cap;
		it.strand = e->strand;
	}
	return defer ? 0 : join_k1f(e); // the caller may change the batches once the stream has passed this call: K1f now
}

// Step 7, the k of the list K1h is not built for: K1 over the same tiles (staged straight from the tiled layout).  K1's spaced planes stage row slots
// (a re-layout pass): their skip list is everything but them
int run_k1_share(ntc_engine* e, const Segs& segs)
{
	std::vector<uint8_t> skip_tiles(e->k_tiled), skip_rows(e->klist.size(), 1);
	bool any_tiles = false, any_rows = false;
	for (size_t ki = 0; ki < e->klist.size(); ++ki)
		if (!e->k_tiled[ki] && !e->plain(ki)) {
			skip_tiles[ki] = 1;
			skip_rows[ki] = 0;
			any_rows = true;
		} else {
			any_tiles |= !e->k_tiled[ki];
		}
	for (const auto& sg : segs) {
		// a ragged batch: K1 takes every read's length from a slot table, built here from the tiles' prefix tables — the batch stays on tiles,
		// K1h + K1f serve their k from it and K1 the rest
		const uint32_t* d_meta = nullptr;
		if (sg.d_tails)
			if (int rc = tiled_meta(e, sg, &d_meta)) return rc;
		if (any_tiles)
			if (int rc = run_batch(e, sg.d_tiles, d_meta, sg.n_reads, sg.read_len, 16u * ((sg.read_len + 15u) / 16u), true, &skip_tiles)) return rc;
		if (any_rows)
			if (int rc = run_tiled_as_rows(e, sg, d_meta, &skip_rows)) return rc;
	}
	return 0;
}
} // namespace

// K1h + K1f over up to kK1hSegs tiled batches of different geometry in ONE launch per k (launch_sketch_k1h_multi): the length bins of a ragged read set
// share the launch's workgroups in proportion to their blocks instead of queueing as small launches, each of which would pay the waves' start-up again
int run_tiled_segs(ntc_engine* e, const TiledSeg* segs_in, uint32_t n_in, uint64_t n_submits, bool k1f_now)
{
	Segs segs;
	bool any_tails = false, any_trim = false; // any_trim: pieces that some k of the list takes shorter than they are — only K1h + K1f count those
	for (uint32_t i = 0; i < n_in; ++i)
		if (segs_in[i].n_reads) {
			segs.push_back(segs_in[i]);
			any_tails |= segs_in[i].d_tails != nullptr;
			for (uint32_t k : e->klist)
				any_trim |= segs_in[i].len_for(k) != segs_in[i].read_len;
		}
	if (segs.empty()) return 0;
	int rc = 0;
	if (route_tiled(e, segs, any_tails, rc)) return rc;
	unsigned cus = 0;
	if ((rc = device_cus(e->device, cus))) return rc;
	// (a launch gives every batch at least one workgroup, and the suspect lists are sized for cus x 8 regions: no more batches than CUs)
	const uint32_t max_segs = std::min<uint32_t>(std::min<uint32_t>(ntc::kK1hSegs, ntc::kK1fBatch), std::max(1u, cus));
	if (split_tiled(e, segs, max_segs, k1f_now, rc) || probe_head_tiled(e, segs, k1f_now, rc)) return rc;
	std::vector<K1hPlan> plans;
	K1hNeed need;
	plan_k1h(e, segs, cus, plans, need);
	if (e->d_log) {
		// Step 4: candidates of these batches, every k of K1h's (run_k1 books K1's share), + what every logging wave may leave unused at the end of a region
		double est = 0;
		for (const K1hPlan& p : plans) {
			for (uint32_t i = 0; i < p.na; ++i)
				est += (double)p.act[i]->n_reads * sampled_per_read(p.hs[i].read_len, e->klist[p.ki], e->s_bits);
			est += 64.0 * 4096;
		}
		if ((rc = book_log(e, est))) return rc;
	}
	// ntRead's loop over kList (ntcard.cpp:147-158): one launch per k over the same resident batches
	const bool defer = e->defer_redo && !k1f_now;
	bool counted = false; // this submit counts as one launch of ntc_kernel_time once its first kernel is queued (not at all when read_len < every k)
	for (K1hPlan& p : plans) {
		hipEvent_t after = nullptr;
		if (e->k1f_n + p.na > ntc::kK1fBatch) // no sets left for these launches: K1f over the waiting ones first
			if ((rc = join_k1f(e, &after))) return rc;
		if ((rc = open_run(e, after))) return rc;
		if (e->profiling && !counted) {
			e->run.submits += n_submits;
			counted = true;
		}
		bool no_room = false;
		if (int rc_sets = ensure_sets(e, p.na, need, defer, no_room)) {
			// no memory for K1h's hand-over arrays (8 sets with NTC_FLAG_DEFER_REDO: up to ~0.5 GB each per 10 M reads): the
			// batches are K1's, unless the caller insists on the tiled kernels or part of the k list has been launched already
			if (!no_room || e->ts_required || &p != &plans.front() || any_tails || any_trim) return rc_sets;
			if ((rc = close_run(e))) return rc;
			for (const auto& sg : segs)
				if ((rc = run_tiled_as_rows(e, sg))) return rc;
			return 0;
		}
		if ((rc = launch_k1h(e, p, need, cus, defer))) return rc;
	}
	if (!e->profiling)
		if ((rc = close_run(e))) return rc; // (profiling was switched off inside a run)
	return e->ts_all ? 0 : run_k1_share(e, segs);
}

// a device-resident tiled batch under NTC_FLAG_DEFER_REDO, every k K1h's: it waits for up to seven more (one K1h launch per k over all of them)
int defer_or_run_tiled(ntc_engine* e, const TiledSeg& sg)
{
	if (!(e->defer_redo && e->ts_all)) return run_tiled_segs(e, &sg, 1);
	e->deferred.push_back(sg);
	if (e->deferred.size() >= std::min<size_t>(ntc::kK1hSegs, ntc::kK1fBatch)) return flush_deferred(e);
	return 0;
}

} // namespace ntc_eng
