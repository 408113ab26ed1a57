// ntc_merge.hip — one sketch out of several: ntc_merge_counters (host arrays), ntc_merge_devices (the engines of one process, peer copies) and the
// hit-log exchange of the owner merge, ntc_log_export_device / ntc_log_replace_device (ntc_engine.hpp)
#include "ntc_engine.hpp"

using namespace ntc_eng;

extern "C" {

int ntc_merge_counters(ntc_engine* e, const uint16_t* t_counter, const uint64_t* f1)
{
	if (!e || !t_counter) return fail(NTC_ERR_ARG, "ntc_merge_counters: null argument");
	if (e->hll_bits) return fail(NTC_ERR_STATE, "ntc_merge_counters: not for an nthll engine");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	const size_t nk = e->klist.size();
	const uint64_t per_k = e->plane_elems(); // counters per k (both samples)
	if (!e->d_out16.reserve(per_k * sizeof(uint16_t)))
		return fail(NTC_ERR_MEMORY, "ntc_merge_counters: cannot allocate uint16 staging");
	for (size_t ki = 0; ki < nk; ++ki) {
		HIP_TRY(hipMemcpyAsync(e->d_out16, t_counter + ki * per_k, per_k * sizeof(uint16_t), hipMemcpyHostToDevice, e->stream));
		HIP_TRY(ntc::launch_add_counters(e->d_sketch + ki * per_k, e->d_out16, per_k, e->stream));
		e->sk_host_dirty = true;
	}
	if (f1) {
		std::vector<unsigned long long> cur(nk);
		HIP_TRY(hipMemcpyAsync(cur.data(), e->d_f1, nk * 8, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
		for (size_t ki = 0; ki < nk; ++ki)
			cur[ki] += f1[ki];
		HIP_TRY(hipMemcpyAsync(e->d_f1, cur.data(), nk * 8, hipMemcpyHostToDevice, e->stream));
	}
	HIP_TRY(hipStreamSynchronize(e->stream));
	return 0;
}

// ---- multi-GPU merge in ONE host process -------------------------------------------------------
// The reference's threads all increment one shared t_Counter (ntcard.cpp:142-143,445) and add their k-mer counts into
// one totalKmers (ntcard.cpp:464-466); with one private sketch per engine the same state is the element-wise SUM of the
// sketches (MAX for nthll's registers, nthll.cpp:238-243).  t_Counter wraps at 16 bits, so only the low halves of the
// per-engine counters matter: (sum_e c_e) mod 2^16 == (sum_e (c_e mod 2^16)) mod 2^16.  The merge is the same exchange
// bench.py runs between processes with RCCL's all-to-all (ntcard_amd/parallel.py), written with peer copies because here
// all devices belong to one process: every engine narrows its counters to 16 bits, slice j of every engine goes to engine
// j's device — all N x (N-1) copies are in flight together, each on its own point-to-point xGMI link, 2 B x counters / N
// per link —, engine j adds its N slices with wrapping 16-bit adds, the summed slices are gathered on engine 0's device
// (again one slice per link) and widened into engine 0's sketch.  No communicator, no library beyond HIP; devices without
// peer access are served by hipMemcpyPeerAsync's staged path.  nthll's register file (2^nBits dwords) and F1 are tiny:
// copied to the root device and folded there (max / sum, full width).
namespace {
struct MergePeer {
	ntc_engine* e = nullptr;
	uint16_t* narrow = nullptr; // [counters]      this engine's counters mod 2^16
	uint16_t* recv = nullptr;   // [n][slice]      slice `me` of every engine; the sum ends up in recv[0 .. slice)
	std::vector<hipStream_t> lanes; // one copy stream per peer: the copies into this device run side by side
	hipEvent_t narrowed = nullptr, summed = nullptr;
	std::vector<hipEvent_t> arrived;
};
hipError_t copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st)
{
	if (bytes == 0) return hipSuccess;
	return dst_dev == src_dev ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}
void enable_peer_access(const std::vector<MergePeer>& peers)
{
	for (const MergePeer& a : peers)
		for (const MergePeer& b : peers) {
			int can = 0;
			if (a.e->device == b.e->device || hipDeviceCanAccessPeer(&can, a.e->device, b.e->device) != hipSuccess || !can) continue;
			(void)hipSetDevice(a.e->device);
			(void)hipDeviceEnablePeerAccess(b.e->device, 0); // hipErrorPeerAccessAlreadyEnabled is fine
			(void)hipGetLastError();
		}
}
void release_peers(std::vector<MergePeer>& peers) // (buffers, streams and events belong to the engines' merge caches: only wait)
{
	for (MergePeer& p : peers) {
		if (!p.e) continue;
		(void)hipSetDevice(p.e->device);
		for (hipStream_t s : p.lanes)
			if (s) (void)hipStreamSynchronize(s);
		(void)hipStreamSynchronize(p.e->stream);
	}
}
// full-width fold of a small array of every engine into the root's (nthll registers: max; F1: sum)
int fold_small(ntc_engine* const* engines, int32_t n, bool regs)
{
	ntc_engine* root = engines[0];
	const size_t bytes = regs ? (root->klist.size() * 4) << root->hll_bits : root->klist.size() * 8; // (nthll: every plane's register file)
	void* tmp = nullptr;
	HIP_TRY(hipSetDevice(root->device));
	HIP_TRY(hipMalloc(&tmp, bytes));
	int rc = 0;
	for (int32_t i = 1; i < n && !rc; ++i) {
		const void* src = regs ? (const void*)engines[i]->d_sketch : (const void*)engines[i]->d_f1;
		hipError_t h = copy_between(tmp, root->device, src, engines[i]->device, bytes, root->stream);
		if (h == hipSuccess)
			h = regs ? ntc::launch_fold_u32(root->d_sketch, (const uint32_t*)tmp, bytes / 4, true, root->stream)
			         : ntc::launch_fold_u64((unsigned long long*)root->d_f1, (const unsigned long long*)tmp, bytes / 8, root->stream);
		if (h != hipSuccess) rc = fail(NTC_ERR_DEVICE, "ntc_merge_devices: folding engine %d failed: %s", i, hipGetErrorString(h));
	}
	(void)hipStreamSynchronize(root->stream);
	(void)hipFree(tmp);
	return rc;
}
} // namespace

int ntc_merge_devices(ntc_engine* const* engines, int32_t n_engines)
{
	if (!engines || n_engines < 1) return fail(NTC_ERR_ARG, "ntc_merge_devices: need at least one engine");
	ntc_engine* root = engines[0];
	if (!root) return fail(NTC_ERR_ARG, "ntc_merge_devices: null engine");
	for (int32_t i = 0; i < n_engines; ++i) {
		ntc_engine* e = engines[i];
		if (!e || e->klist != root->klist || e->masks != root->masks || e->strand != root->strand || e->hpc != root->hpc || e->sig != root->sig || e->r_bits != root->r_bits || e->s_bits != root->s_bits || e->hll_bits != root->hll_bits)
			return fail(NTC_ERR_ARG, "ntc_merge_devices: engine %d is not configured like engine 0", i);
		for (int32_t j = 0; j < i; ++j)
			if (engines[j] == e) return fail(NTC_ERR_ARG, "ntc_merge_devices: engine %d listed twice", i);
	}
	// every engine stays locked (in address order) from the applies to the last copy: a submit on one of them from another thread would
	// race with the narrow / widen kernels on its sketch
	std::vector<ntc_engine*> order(engines, engines + n_engines);
	std::sort(order.begin(), order.end());
	std::vector<std::unique_lock<std::mutex>> locks;
	for (ntc_engine* e : order)
		locks.emplace_back(e->mu);
	// 1. pending increments first, everything quiescent
	for (int32_t i = 0; i < n_engines; ++i) {
		HIP_TRY(hipSetDevice(engines[i]->device));
		if (int rc = apply_log(engines[i])) return rc;
		if (int rc = sig_flush(engines[i])) return rc;
		HIP_TRY(hipStreamSynchronize(engines[i]->stream));
	}
	if (n_engines == 1) return 0;
	const uint32_t n = (uint32_t)n_engines;
	// 2. F1 (and nthll's registers) at full width
	if (int rc = fold_small(engines, n_engines, false)) return rc;
	if (root->hll_bits) {
		if (int rc = fold_small(engines, n_engines, true)) return rc;
	} else {
		// 3. the counters: 16-bit slices, all-to-all, wrapping sums, gather, widen
		const uint64_t counters = root->klist.size() * root->plane_elems();
		const uint64_t slice = ((counters + n - 1) / n + 7) & ~7ull; // elements per slice (16-byte multiples); the last one may be short or empty
		auto len_of = [&](uint32_t j) { return (uint64_t)j * slice >= counters ? 0ull : std::min<uint64_t>(slice, counters - (uint64_t)j * slice); };
		std::vector<MergePeer> peers(n);
		auto run = [&]() -> int {
			for (uint32_t i = 0; i < n; ++i) {
				MergePeer& p = peers[i];
				p.e = engines[i];
				HIP_TRY(hipSetDevice(p.e->device));
				auto& mc = p.e->mc;
				for (auto grow : {std::make_pair(&mc.narrow, (size_t)counters * 2), std::make_pair(&mc.recv, (size_t)n * slice * 2)}) {
					if (grow.first->cap >= grow.second) continue;
					if (!grow.first->reserve(grow.second))
						return fail(NTC_ERR_MEMORY, "ntc_merge_devices: cannot allocate the %llu-byte exchange buffer on device %d", (unsigned long long)grow.second, p.e->device);
					++p.e->merge_allocs;
				}
				while (mc.lanes.size() < n) {
					hipStream_t st = nullptr;
					hipEvent_t ev = nullptr;
					HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
					if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { // lanes and arrived stay the same length
						(void)hipStreamDestroy(st);
						return fail(NTC_ERR_DEVICE, "ntc_merge_devices: cannot create an event on device %d", p.e->device);
					}
					mc.lanes.push_back(st);
					mc.arrived.push_back(ev);
					p.e->merge_allocs += 2;
				}
				if (!mc.narrowed) {
					HIP_TRY(hipEventCreateWithFlags(&mc.narrowed, hipEventDisableTiming));
					++p.e->merge_allocs;
				}
				if (!mc.summed) { // (tested on its own: a failure here must be retried by the next merge)
					HIP_TRY(hipEventCreateWithFlags(&mc.summed, hipEventDisableTiming));
					++p.e->merge_allocs;
				}
				p.narrow = mc.narrow;
				p.recv = mc.recv;
				p.lanes.assign(mc.lanes.begin(), mc.lanes.begin() + n);
				p.arrived.assign(mc.arrived.begin(), mc.arrived.begin() + n);
				p.narrowed = mc.narrowed;
				p.summed = mc.summed;
			}
			enable_peer_access(peers);
			for (MergePeer& p : peers) { // narrow
				HIP_TRY(hipSetDevice(p.e->device));
				HIP_TRY(ntc::launch_narrow_u16(p.e->d_sketch, p.narrow, counters, p.e->stream));
				HIP_TRY(hipEventRecord(p.narrowed, p.e->stream));
			}
			for (uint32_t j = 0; j < n; ++j) { // all-to-all: slice j of engine i -> engine j, on j's lane i
				MergePeer& dst = peers[j];
				HIP_TRY(hipSetDevice(dst.e->device));
				for (uint32_t t = 0; t < n; ++t) {
					const uint32_t i = (j + t) % n; // staggered start: at every moment the devices talk to distinct partners
					const MergePeer& src = peers[i];
					HIP_TRY(hipStreamWaitEvent(dst.lanes[i], src.narrowed, 0));
					HIP_TRY(copy_between(dst.recv + (uint64_t)i * slice, dst.e->device, src.narrow + (uint64_t)j * slice, src.e->device, len_of(j) * 2, dst.lanes[i]));
					HIP_TRY(hipEventRecord(dst.arrived[i], dst.lanes[i]));
					HIP_TRY(hipStreamWaitEvent(dst.e->stream, dst.arrived[i], 0));
				}
				HIP_TRY(ntc::launch_sum_slices_u16(dst.recv, slice, n, len_of(j), dst.e->stream));
				HIP_TRY(hipEventRecord(dst.summed, dst.e->stream));
			}
			// gather on the root: its own `narrow` is free once every peer has taken its slice of it — simpler: the root's lanes wait for
			// those copies (arrived events of slice 0 on every peer) before overwriting
			MergePeer& r0 = peers[0];
			HIP_TRY(hipSetDevice(r0.e->device));
			for (uint32_t j = 0; j < n; ++j) {
				for (uint32_t q = 0; q < n; ++q)
					HIP_TRY(hipStreamWaitEvent(r0.lanes[j], peers[q].arrived[0], 0)); // engine 0's slices have left `narrow`
				HIP_TRY(hipStreamWaitEvent(r0.lanes[j], peers[j].summed, 0));
				HIP_TRY(copy_between(r0.narrow + (uint64_t)j * slice, r0.e->device, peers[j].recv, peers[j].e->device, len_of(j) * 2, r0.lanes[j]));
				HIP_TRY(hipEventRecord(r0.arrived[j], r0.lanes[j])); // (re-used: slice j of the sum has arrived)
				HIP_TRY(hipStreamWaitEvent(r0.e->stream, r0.arrived[j], 0));
			}
			HIP_TRY(ntc::launch_widen_u16(r0.narrow, r0.e->d_sketch, counters, r0.e->stream));
			r0.e->sk_host_dirty = true;
			for (MergePeer& p : peers) {
				HIP_TRY(hipSetDevice(p.e->device));
				for (hipStream_t s : p.lanes)
					HIP_TRY(hipStreamSynchronize(s));
				HIP_TRY(hipStreamSynchronize(p.e->stream));
			}
			return 0;
		};
		const int rc = run();
		release_peers(peers);
		if (rc) return rc;
	}
	// NTC_FLAG_SIGNATURE: the compacted pairs of engines 1 .. travel to engine 0's device and are injected there (counts add up)
	if (root->sig)
		for (int32_t i = 1; i < n_engines; ++i)
			if (int rc = sig_merge_from(root, engines[i])) return rc;
	// 4. everything now lives in engine 0 (counters as their value mod 2^16, which is all t_Counter ever held): the others start
	//    from zero again, the sum stays what it was
	locks.clear(); // (ntc_reset takes the engine's lock itself)
	for (int32_t i = 1; i < n_engines; ++i)
		if (int rc = ntc_reset(engines[i])) return rc;
	HIP_TRY(hipSetDevice(root->device));
	return 0;
}

int ntc_log_export_device(ntc_engine* e, uint32_t n_parts, void* d_keys_u32, const uint64_t* part_offset, uint64_t* counts_out)
{
	if (!e || !counts_out) return fail(NTC_ERR_ARG, "ntc_log_export_device: null argument");
	if (n_parts < 1 || n_parts > 64) return fail(NTC_ERR_ARG, "ntc_log_export_device: n_parts %u outside 1..64", n_parts);
	if (d_keys_u32 && !part_offset) return fail(NTC_ERR_ARG, "ntc_log_export_device: keys without part offsets");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (!e->d_log || e->hll_bits) return fail(NTC_ERR_STATE, "ntc_log_export_device: this engine has no hit log");
	const uint64_t counters = e->klist.size() * e->plane_elems();
	if (counters % n_parts) return fail(NTC_ERR_ARG, "ntc_log_export_device: %u parts do not divide %llu counters", n_parts, (unsigned long long)counters);
	if (int rc = join_k1f(e)) return rc; // (K1f's suspects are log entries too)
	// the sketch must still hold the zeros of the last reset: everything counted so far is in the log
	uint32_t dirty = 0;
	HIP_TRY(hipMemcpyAsync(&dirty, e->d_skdirty, 4, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (e->sk_host_dirty || dirty != 0u)
		return fail(NTC_ERR_STATE, "ntc_log_export_device: the sketch already holds counts (a sketch update ran, or a kernel incremented it directly): merge counters instead");
	unsigned long long* const d_cursor = reinterpret_cast<unsigned long long*>(e->d_skdirty + 16);
	unsigned long long* const d_off = d_cursor + 64;
	unsigned long long h_off[64] = {0};
	if (part_offset)
		for (uint32_t p = 0; p < n_parts; ++p)
			h_off[p] = part_offset[p];
	hipError_t rc = hipMemsetAsync(d_cursor, 0, 64 * 8, e->stream);
	if (rc == hipSuccess) rc = hipMemcpyAsync(d_off, h_off, 64 * 8, hipMemcpyHostToDevice, e->stream);
	if (rc == hipSuccess)
		rc = ntc::launch_log_export(e->d_log, e->d_logfill, e->log_region_cap, e->all_log_regions(), n_parts, (uint32_t)(counters / n_parts), (uint32_t*)d_keys_u32, d_off,
		                            d_cursor, e->stream);
	unsigned long long h_cnt[64] = {0};
	if (rc == hipSuccess) rc = hipMemcpyAsync(h_cnt, d_cursor, 64 * 8, hipMemcpyDeviceToHost, e->stream);
	if (rc == hipSuccess) rc = hipStreamSynchronize(e->stream);
	if (rc != hipSuccess) return fail(NTC_ERR_DEVICE, "ntc_log_export_device: %s", hipGetErrorString(rc));
	for (uint32_t p = 0; p < n_parts; ++p)
		counts_out[p] = h_cnt[p];
	return 0;
}

int ntc_log_replace_device(ntc_engine* e, const void* d_keys_u32, uint64_t n_keys)
{
	if (!e || (!d_keys_u32 && n_keys)) return fail(NTC_ERR_ARG, "ntc_log_replace_device: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (!e->d_log || e->hll_bits) return fail(NTC_ERR_STATE, "ntc_log_replace_device: this engine has no hit log");
	const uint64_t room = (uint64_t)e->all_log_regions() * e->log_region_cap;
	if (n_keys > room) return fail(NTC_ERR_ARG, "ntc_log_replace_device: %llu keys do not fit the %llu-entry log", (unsigned long long)n_keys, (unsigned long long)room);
	if (int rc = join_k1f(e)) return rc; // (nothing may append behind this point)
	if (n_keys) HIP_TRY(hipMemcpyAsync(e->d_log, d_keys_u32, n_keys * 4, hipMemcpyDeviceToDevice, e->stream));
	HIP_TRY(ntc::launch_log_set_fill(e->d_logfill, e->all_log_regions(), e->log_region_cap, n_keys, e->stream));
	e->log_pending = n_keys != 0;
	e->log_est = (double)n_keys;
	return 0;
}


} // extern "C"
