// ntc_signature.hip — NTC_FLAG_SIGNATURE: per plane, every sampled 64-bit value with its exact count (include/ntcard_hip.h; DESIGN.md §4 "Signatures").
//
// K1's signature instantiations (ntc_sketch_hf.hip, kSig) append the value of every sampled k-mer to the plane's u64 value log, in chunks a wave books with
// one cursor atomic each (the unused rest of a chunk is zeroed): no CAS loop in K1's registers.  The kernels here move the log into the plane's container, an open-addressing table
//     uint64 keys[slots] (0 = empty: no sampled value is 0)  +  uint32 counts[slots],   slots a power of two,
// home slot = the top bits of h * 0x9E3779B97F4A7C15 (the bits ntComp's patterns fix — the top s + 1 of h — only add a constant to the product), linear probing,
// a 64-bit atomicCAS claims a slot, atomicAdd counts.  The host keeps every table at most half full BEFORE a launch inserts into it (sig_room), so no probe
// runs round a full table and no kernel waits on another workgroup.  The same kernel re-inserts a table into its successor (growth), takes device or host
// pairs (ntc_signature_inject*) and a peer's compacted pairs (ntc_merge_devices).  ntc_signature / ntc_signature_device compact a table and sort the compaction on
// the device (ntc_sig_sort.hip).  Vector stores and plain C++ only; every launch is on the engine's stream.
#include <cerrno>

#include "ntc_sig_device.hpp"

namespace ntc {

namespace {

constexpr unsigned long long kSigMul = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kSigBlocks = 4096; // grid cap of sig_insert_kernel and sig_compact_kernel

// one pair into the table; kSat: the count may be anything (inject, rehash, merge) — a CAS loop that saturates; else add <= 64 and the launch adds fewer than
// 2^31 in all (the log's capacity), so a counter below 2^31 cannot wrap under plain atomicAdd and only one at or above it takes the loop
template <bool kSat>
__device__ __forceinline__ void sig_put(const SigTable& t, unsigned long long h, uint32_t add, uint32_t shift)
{
	const uint64_t mask = t.slots - 1;
	uint64_t s = (h * kSigMul) >> shift;
	for (;;) {
		unsigned long long cur = __hip_atomic_load(t.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == 0ull) {
			cur = atomicCAS(t.keys + s, 0ull, h);
			if (cur == 0ull) {
				atomicAdd(t.live, 1ull);
				cur = h;
			}
		}
		if (cur == h) break;
		s = (s + 1) & mask;
	}
	uint32_t* c = t.counts + s;
	if (!kSat && __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0x80000000u) {
		atomicAdd(c, add);
		return;
	}
	uint32_t old = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	for (;;) {
		const uint32_t want = old > 0xffffffffu - add ? 0xffffffffu : old + add;
		if (want == old) break;
		const uint32_t seen = atomicCAS(c, old, want);
		if (seen == old) break;
		old = seen;
	}
}

template <bool kSat>
__global__ __launch_bounds__(256) void sig_insert_kernel(const SigTable t, const unsigned long long* __restrict__ in_keys, const uint32_t* __restrict__ in_counts,
                                                         uint64_t n, uint32_t shift)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	const uint64_t rounds = (n + step - 1) / step; // every wave runs the same number of rounds: the ballots below see whole waves
	for (uint64_t r = 0, i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounds; ++r, i += step) {
		unsigned long long h = 0;
		uint32_t add = 0;
		if (i < n) {
			h = in_keys[i];
			add = in_counts ? in_counts[i] : 1u;
		}
		bool go = h != 0ull && add != 0u;
		if constexpr (!kSat) {
			// one hot value (a homopolymer, a repeat): the lanes that hold the first lane's value send ONE add instead of 64 to the same address
			const unsigned long long first = wave_first(h);
			const uint64_t same = __builtin_amdgcn_ballot_w64(go && h == first);
			if (go && h == first) {
				go = lanes_below(same) == 0u;
				add = (uint32_t)__popcll(same);
			}
		}
		if (go) sig_put<kSat>(t, h, add, shift);
	}
}

__global__ __launch_bounds__(256) void sig_compact_kernel(const SigTable t, unsigned long long* __restrict__ out_keys, uint32_t* __restrict__ out_counts,
                                                          unsigned long long* __restrict__ cursor)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	const uint64_t rounds = (t.slots + step - 1) / step;
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t r = 0, i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rounds; ++r, i += step) {
		const unsigned long long h = i < t.slots ? t.keys[i] : 0ull;
		const uint64_t m = __builtin_amdgcn_ballot_w64(h != 0ull);
		if (m == 0) continue;
		unsigned long long b = 0;
		if (lane == 0) b = atomicAdd(cursor, (unsigned long long)__popcll(m));
		const uint64_t at = wave_first(b) + lanes_below(m);
		if (h != 0ull) {
			out_keys[at] = h;
			out_counts[at] = t.counts[i];
		}
	}
}

} // namespace

hipError_t launch_sig_insert(const SigTable& t, const unsigned long long* in_keys, const uint32_t* in_counts, uint64_t n, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	uint32_t bits = 0;
	while ((1ull << bits) < t.slots)
		++bits;
	if ((1ull << bits) != t.slots || bits < 1) return hipErrorInvalidValue;
	if (in_counts == nullptr) // the value log, or a list of single occurrences: fewer than 2^31 adds of 1
		hipLaunchKernelGGL(sig_insert_kernel<false>, dim3(capped_grid(n, kSigBlocks)), dim3(256), 0, st, t, in_keys, in_counts, n, 64u - bits);
	else
		hipLaunchKernelGGL(sig_insert_kernel<true>, dim3(capped_grid(n, kSigBlocks)), dim3(256), 0, st, t, in_keys, in_counts, n, 64u - bits);
	return hipGetLastError();
}

hipError_t launch_sig_compact(const SigTable& t, unsigned long long* out_keys, uint32_t* out_counts, unsigned long long* cursor, hipStream_t st)
{
	hipLaunchKernelGGL(sig_compact_kernel, dim3(capped_grid(t.slots, kSigBlocks)), dim3(256), 0, st, t, out_keys, out_counts, cursor);
	return hipGetLastError();
}

} // namespace ntc

namespace ntc_eng {

namespace {

constexpr uint64_t kSigDefaultSlots = 1ull << 16, kSigDefaultLog = 1ull << 27, kSigMaxLog = 1ull << 30; // (fewer than 2^31 adds per insert launch: sig_put)

// the state words of plane pl: {log cursor, live keys of the table, values in the log} (K1 reaches the third through the cursor's address)
constexpr size_t kSigWords = 3;
unsigned long long* sig_cursor(const ntc_engine* e, size_t pl) { return e->d_sigstate.get() + kSigWords * pl; }
unsigned long long* sig_live(const ntc_engine* e, size_t pl) { return e->d_sigstate.get() + kSigWords * pl + 1; }
unsigned long long* sig_scratch(const ntc_engine* e) { return e->d_sigstate.get() + kSigWords * e->klist.size(); }

ntc::SigTable sig_table(const ntc_engine* e, size_t pl)
{
	const auto& p = e->sig_planes[pl];
	return ntc::SigTable{p.keys.get(), p.counts.get(), p.slots, sig_live(e, pl)};
}

// {cursor, live, values} of every plane (waits for the stream); live_ub becomes exact
int sig_read_state(ntc_engine* e, std::vector<unsigned long long>& st)
{
	st.assign(kSigWords * e->klist.size(), 0ull);
	HIP_TRY(hipMemcpyAsync(st.data(), e->d_sigstate, st.size() * 8, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	for (size_t pl = 0; pl < e->sig_planes.size(); ++pl)
		e->sig_planes[pl].live_ub = st[kSigWords * pl + 1];
	return 0;
}

int sig_alloc_table(ntc_engine* e, ntc_engine::SigPlane& p, uint64_t slots)
{
	if (!p.keys.reserve(slots * 8) || !p.counts.reserve(slots * 4)) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "signature: cannot allocate a table of %llu slots (%llu B) on device; no value was dropped, the engine's counts stay valid up to the last call that succeeded",
		            (unsigned long long)slots, (unsigned long long)(slots * 12));
	}
	p.slots = slots;
	HIP_TRY(hipMemsetAsync(p.keys, 0, slots * 8, e->stream));
	HIP_TRY(hipMemsetAsync(p.counts, 0, slots * 4, e->stream));
	return 0;
}

// the plane's table takes `add` more keys and stays at most half full — live_ub must be current (sig_read_state) where growth is to be avoided.  Growing
// re-inserts the old table into one of 2^j times its size and waits for the stream.  The new table counts its keys in the scratch word; the plane's own
// live word and the old table are replaced only once everything has succeeded, so a failure at any step leaves the plane as it was
int sig_room(ntc_engine* e, size_t pl, uint64_t add)
{
	auto& p = e->sig_planes[pl];
	const uint64_t need = p.live_ub + add;
	if (2 * need <= p.slots) return 0;
	uint64_t slots = p.slots;
	uint64_t doublings = 0;
	while (2 * need > slots)
		slots *= 2, ++doublings;
	ntc_engine::SigPlane next;
	if (int rc = sig_alloc_table(e, next, slots)) return rc;
	auto rehash = [&]() -> int {
		Span sp;
		if (int rc = open_span(e, sp)) return rc;
		HIP_TRY(hipMemsetAsync(sig_scratch(e), 0, 8, e->stream));
		HIP_TRY(ntc::launch_sig_insert(ntc::SigTable{next.keys.get(), next.counts.get(), next.slots, sig_scratch(e)}, p.keys, p.counts, p.slots, e->stream));
		if (int rc = close_span(sp, e->stream, e->timers[T_SIG_GROW].spans)) return rc;
		HIP_TRY(hipStreamSynchronize(e->stream)); // (the new table is complete before the old one goes)
		HIP_TRY(hipMemcpyAsync(sig_live(e, pl), sig_scratch(e), 8, hipMemcpyDeviceToDevice, e->stream));
		return 0;
	};
	if (int rc = rehash()) {
		(void)hipStreamSynchronize(e->stream); // (nothing of `next` in flight when it is freed)
		return rc;
	}
	std::swap(p.keys, next.keys);
	std::swap(p.counts, next.counts);
	p.slots = slots;
	(void)hipStreamSynchronize(e->stream); // (before the old table, now in `next`, is freed)
	e->sig_grows += doublings;
	return 0;
}

// (hashes, counts) of a plane, unsorted, into the engine's scratch; *n = how many.  The log must be flushed.
int sig_compact(ntc_engine* e, size_t pl, uint64_t* n)
{
	std::vector<unsigned long long> st;
	if (int rc = sig_read_state(e, st)) return rc;
	*n = st[kSigWords * pl + 1];
	if (*n == 0) return 0;
	if (!e->d_sigtmp_k.reserve(*n * 8) || !e->d_sigtmp_c.reserve(*n * 4)) return fail(NTC_ERR_MEMORY, "signature: cannot allocate %llu B of scratch on device", (unsigned long long)(*n * 12));
	HIP_TRY(hipMemsetAsync(sig_scratch(e), 0, 8, e->stream));
	HIP_TRY(ntc::launch_sig_compact(sig_table(e, pl), e->d_sigtmp_k, e->d_sigtmp_c, sig_scratch(e), e->stream));
	return 0;
}

// n device pairs into plane pl (stream-ordered unless the table has to grow)
int sig_inject_device(ntc_engine* e, size_t pl, const unsigned long long* d_keys, const uint32_t* d_counts, uint64_t n)
{
	if (n == 0) return 0;
	auto& p = e->sig_planes[pl];
	if (2 * (p.live_ub + n) > p.slots) { // the bound says it may not fit: the exact figure first
		std::vector<unsigned long long> st;
		if (int rc = sig_read_state(e, st)) return rc;
	}
	if (int rc = sig_room(e, pl, n)) return rc;
	for (uint64_t done = 0; done < n;) { // (a counted insert takes any number of pairs; pairs without counts fewer than 2^31 per launch: sig_put)
		const uint64_t m = std::min<uint64_t>(n - done, kSigMaxLog);
		HIP_TRY(ntc::launch_sig_insert(sig_table(e, pl), d_keys + done, d_counts ? d_counts + done : nullptr, m, e->stream));
		done += m;
	}
	p.live_ub += n;
	return 0;
}

int sig_check(ntc_engine* e, uint32_t plane, const char* who)
{
	if (!e) return fail(NTC_ERR_ARG, "%s: null engine", who);
	if (!e->sig) return fail(NTC_ERR_STATE, "%s: the engine was created without NTC_FLAG_SIGNATURE", who);
	if (plane >= e->klist.size()) return fail(NTC_ERR_ARG, "%s: plane %u of %zu", who, plane, e->klist.size());
	return 0;
}

// the plane's pairs, strictly ascending by hash, in the engine's scratch: *k, *c (valid until the engine compacts again), *n of them.  Pending work is brought in,
// the table is compacted and the compaction sorted on the device (ntc_sig_sort.hip); cap < n, or no memory for the scratch: an error before anything moves
int sig_sorted(ntc_engine* e, uint32_t plane, uint64_t cap, const char* who, uint64_t* n, const unsigned long long** k, const uint32_t** c)
{
	if (int rc = join_k1f(e)) return rc;
	if (int rc = sig_flush(e)) return rc;
	std::vector<unsigned long long> st;
	if (int rc = sig_read_state(e, st)) return rc;
	const uint64_t live = st[kSigWords * plane + 1];
	if (cap < live) return fail(NTC_ERR_ARG, "%s: plane %u holds %llu values, the arrays have room for %llu", who, plane, (unsigned long long)live, (unsigned long long)cap);
	if (live >> 32) return fail(NTC_ERR_ARG, "%s: plane %u holds %llu values (fewer than 2^32 are sorted)", who, plane, (unsigned long long)live);
	if (live > ntc::sig_sort_one_launch() &&
	    (!e->d_sigalt_k.reserve(live * 8) || !e->d_sigalt_c.reserve(live * 4) || !e->d_sigsort.reserve(ntc::sig_sort_aux_bytes(live)))) {
		(void)hipGetLastError();
		return fail(NTC_ERR_MEMORY, "%s: cannot allocate %llu B of sort scratch on device; nothing was written", who, (unsigned long long)(live * 12 + ntc::sig_sort_aux_bytes(live)));
	}
	if (int rc = sig_compact(e, plane, n)) return rc;
	bool in_alt = false;
	Span sp;
	if (int rc = open_span(e, sp)) return rc;
	HIP_TRY(ntc::sig_sort(e->d_sigtmp_k, e->d_sigtmp_c, e->d_sigalt_k, e->d_sigalt_c, *n, e->d_sigsort.get(), e->stream, &in_alt));
	if (int rc = close_span(sp, e->stream, e->timers[T_SIG_SORT].spans)) return rc;
	*k = in_alt ? e->d_sigalt_k.get() : e->d_sigtmp_k.get();
	*c = in_alt ? e->d_sigalt_c.get() : e->d_sigtmp_c.get();
	return 0;
}

// ntc_signature (kind = device to host) and ntc_signature_device (device to device): the plane's sorted pairs into the caller's arrays
int sig_copy_out(ntc_engine* e, uint32_t plane, void* hashes, void* counts, uint64_t cap, uint64_t* n_out, hipMemcpyKind kind, const char* who)
{
	if (int rc = sig_check(e, plane, who)) return rc;
	if (!n_out || (!hashes && cap)) return fail(NTC_ERR_ARG, "%s: null argument", who);
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	uint64_t got = 0;
	const unsigned long long* k = nullptr;
	const uint32_t* c = nullptr;
	if (int rc = sig_sorted(e, plane, cap, who, &got, &k, &c)) return rc;
	if (got) {
		HIP_TRY(hipMemcpyAsync(hashes, k, got * 8, kind, e->stream));
		if (counts) HIP_TRY(hipMemcpyAsync(counts, c, got * 4, kind, e->stream));
	}
	HIP_TRY(hipStreamSynchronize(e->stream)); // (the arrays are complete, and the engine's scratch is free again)
	*n_out = got;
	return drain_events(e);
}

// a query of timers: every span that has ended is read first
int sig_times(ntc_engine* e, const char* who, Timer a, double* a_ms, Timer b = kTimers, double* b_ms = nullptr)
{
	if (int rc = sig_check(e, 0, who)) return rc;
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (int rc = drain_events(e)) return rc;
	if (a_ms) *a_ms = e->timers[a].ms;
	if (b_ms) *b_ms = e->timers[b].ms;
	return 0;
}

uint64_t env_u64(const char* name)
{
	const char* v = std::getenv(name);
	if (!v || !*v) return 0;
	char* end = nullptr;
	errno = 0;
	const unsigned long long x = std::strtoull(v, &end, 10);
	return (errno || !end || *end) ? 0 : (uint64_t)x;
}

} // namespace

int sig_setup(ntc_engine* e)
{
	const size_t nk = e->klist.size();
	e->sig_init_slots = kSigDefaultSlots;
	if (const uint64_t v = env_u64("NTC_SIG_SLOTS"))
		if (v >= 64 && (v & (v - 1)) == 0 && v <= (1ull << 40)) e->sig_init_slots = v;
	e->sig_log_limit = kSigDefaultLog;
	if (const uint64_t v = env_u64("NTC_SIG_LOG_ENTRIES")) e->sig_log_limit = std::min<uint64_t>(v, kSigMaxLog);
	e->sig_chunk = e->sig_log_limit >= (1ull << 24) ? 1024u : 64u; // (a small log — tests — is not spent on the waves' chunks)
	e->sig_planes.clear();
	e->sig_planes.resize(nk);
	if (!e->d_sigstate.reserve((kSigWords * nk + 1) * 8)) return fail(NTC_ERR_MEMORY, "ntc_create: cannot allocate the signature state on device");
	return 0;
}

int sig_reset(ntc_engine* e)
{
	HIP_TRY(hipMemsetAsync(e->d_sigstate, 0, (kSigWords * e->klist.size() + 1) * 8, e->stream));
	for (auto& p : e->sig_planes) {
		p.keys.reset(); // (the stream is idle: ntc_reset has waited, create has launched nothing on them)
		p.counts.reset();
		p.live_ub = 0;
		if (int rc = sig_alloc_table(e, p, e->sig_init_slots)) return rc;
	}
	e->sig_booked = 0;
	e->sig_grows = 0;
	return 0;
}

// A launch over n slots runs at most ceil(n / 64) + 15 waves (one wave per 64 slots, the last workgroup of up to 16 waves may be partly idle) and never
// more than a full chip of them; every wave leaves at most one chunk partly unused
uint64_t sig_need(const ntc_engine* e, uint64_t n, uint64_t per)
{
	unsigned cus = 0;
	if (device_cus(e->device, cus) != 0 || cus == 0) cus = 1024; // (cannot fail behind a create; a generous bound if it does)
	const uint64_t waves = std::min<uint64_t>((n + 63) / 64 + 15, (uint64_t)cus * 16);
	return n * per + waves * e->sig_chunk;
}

uint64_t sig_max_slots(ntc_engine* e, uint64_t per)
{
	const uint64_t cap = std::max<uint64_t>(e->sig_log_limit, sig_need(e, 4, per));
	// m slots need at most m * per + (m / 64 + 16) * chunk entries
	const uint64_t fixed = 16ull * e->sig_chunk;
	uint64_t m = (cap - fixed) * 64 / (64 * per + e->sig_chunk);
	m = m >= 64 ? m & ~63ull : m & ~3ull; // whole waves where possible; always a multiple of 4 slots (16-byte aligned sub-batches)
	return std::max<uint64_t>(m, 4);
}

int sig_book(ntc_engine* e, uint64_t windows)
{
	if (windows == 0) return 0;
	if (e->sig_booked != 0 && e->sig_booked + windows > e->sig_log_cap)
		if (int rc = sig_flush(e)) return rc;
	if (windows > e->sig_log_cap) { // grow-only, as far as the batches ask for (up to the limit, which sig_max_slots keeps them under)
		if (int rc = sig_flush(e)) return rc;
		HIP_TRY(hipStreamSynchronize(e->stream));
		const uint64_t cap = std::max<uint64_t>(windows, std::min<uint64_t>(2 * e->sig_log_cap, e->sig_log_limit));
		e->sig_log_cap = 0;
		if (!e->d_siglog.reserve(e->klist.size() * cap * 8)) {
			(void)hipGetLastError();
			return fail(NTC_ERR_MEMORY, "signature: cannot allocate the value log (%zu planes x %llu entries) on device; nothing of this batch was counted", e->klist.size(), (unsigned long long)cap);
		}
		e->sig_log_cap = cap;
	}
	e->sig_booked += windows;
	return 0;
}

void sig_args(const ntc_engine* e, ntc::HfArgs& a, size_t first, size_t n)
{
	for (size_t j = 0; j < n; ++j) {
		a.sig_log[j] = e->d_siglog.get() + (first + j) * e->sig_log_cap;
		a.sig_cursor[j] = sig_cursor(e, first + j);
	}
	a.sig_cap = e->sig_log_cap;
	a.sig_chunk = e->sig_chunk;
}

int sig_flush(ntc_engine* e)
{
	if (!e->sig || e->sig_booked == 0) return 0;
	if (int rc = close_run(e)) return rc;
	std::vector<unsigned long long> st;
	if (int rc = sig_read_state(e, st)) return rc; // the logs' fill and the tables' live keys: exact from here on
	for (size_t pl = 0; pl < e->sig_planes.size(); ++pl)
		if (st[kSigWords * pl] > e->sig_log_cap)
			return fail(NTC_ERR_STATE, "signature: plane %zu booked %llu entries of a log of %llu (internal error: the surplus is lost)", pl, st[kSigWords * pl], (unsigned long long)e->sig_log_cap);
	for (size_t pl = 0; pl < e->sig_planes.size(); ++pl) {
		const uint64_t entries = st[kSigWords * pl], values = st[kSigWords * pl + 2]; // entries: the chunks booked, zeroed rests included
		if (entries == 0) continue;
		if (int rc = sig_room(e, pl, values)) return rc; // (on failure the log stays booked: a later flush tries again)
		Span sp;
		if (int rc = open_span(e, sp)) return rc;
		HIP_TRY(ntc::launch_sig_insert(sig_table(e, pl), e->d_siglog.get() + pl * e->sig_log_cap, nullptr, entries, e->stream));
		HIP_TRY(hipMemsetAsync(sig_cursor(e, pl), 0, 8, e->stream));
		HIP_TRY(hipMemsetAsync(sig_cursor(e, pl) + 2, 0, 8, e->stream));
		if (int rc = close_span(sp, e->stream, e->timers[T_SIG_INSERT].spans)) return rc;
		e->sig_planes[pl].live_ub += values;
	}
	e->sig_booked = 0;
	return 0;
}

int sig_merge_from(ntc_engine* root, ntc_engine* other)
{
	for (size_t pl = 0; pl < root->klist.size(); ++pl) {
		uint64_t n = 0;
		HIP_TRY(hipSetDevice(other->device));
		if (int rc = sig_compact(other, pl, &n)) return rc;
		if (n == 0) continue;
		HIP_TRY(hipStreamSynchronize(other->stream));
		HIP_TRY(hipSetDevice(root->device));
		DevBuf<unsigned long long> k;
		DevBuf<uint32_t> c;
		if (!k.reserve(n * 8) || !c.reserve(n * 4)) return fail(NTC_ERR_MEMORY, "ntc_merge_devices: cannot allocate %llu B for a peer's signature", (unsigned long long)(n * 12));
		if (root->device == other->device) {
			HIP_TRY(hipMemcpyAsync(k, other->d_sigtmp_k, n * 8, hipMemcpyDeviceToDevice, root->stream));
			HIP_TRY(hipMemcpyAsync(c, other->d_sigtmp_c, n * 4, hipMemcpyDeviceToDevice, root->stream));
		} else {
			HIP_TRY(hipMemcpyPeerAsync(k, root->device, other->d_sigtmp_k, other->device, n * 8, root->stream));
			HIP_TRY(hipMemcpyPeerAsync(c, root->device, other->d_sigtmp_c, other->device, n * 4, root->stream));
		}
		if (int rc = sig_inject_device(root, pl, k, c, n)) return rc;
		HIP_TRY(hipStreamSynchronize(root->stream)); // (k, c go away)
	}
	return 0;
}

} // namespace ntc_eng

using namespace ntc_eng;

extern "C" {

int ntc_signature_size(ntc_engine* e, uint32_t plane, uint64_t* n)
{
	if (int rc = sig_check(e, plane, "ntc_signature_size")) return rc;
	if (!n) return fail(NTC_ERR_ARG, "ntc_signature_size: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	if (int rc = join_k1f(e)) return rc;
	if (int rc = sig_flush(e)) return rc;
	std::vector<unsigned long long> st;
	if (int rc = sig_read_state(e, st)) return rc;
	*n = st[kSigWords * plane + 1];
	return 0;
}

int ntc_signature(ntc_engine* e, uint32_t plane, uint64_t* hashes, uint32_t* counts, uint64_t cap, uint64_t* n_out)
{
	return sig_copy_out(e, plane, hashes, counts, cap, n_out, hipMemcpyDeviceToHost, "ntc_signature");
}

int ntc_signature_device(ntc_engine* e, uint32_t plane, void* d_hashes, void* d_counts, uint64_t cap, uint64_t* n_out)
{
	return sig_copy_out(e, plane, d_hashes, d_counts, cap, n_out, hipMemcpyDeviceToDevice, "ntc_signature_device");
}

int ntc_signature_inject_device(ntc_engine* e, uint32_t plane, const void* d_hashes, const void* d_counts, uint64_t n)
{
	if (int rc = sig_check(e, plane, "ntc_signature_inject_device")) return rc;
	if (!d_hashes && n) return fail(NTC_ERR_ARG, "ntc_signature_inject_device: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return sig_inject_device(e, plane, (const unsigned long long*)d_hashes, (const uint32_t*)d_counts, n);
}

int ntc_signature_inject(ntc_engine* e, uint32_t plane, const uint64_t* hashes, const uint32_t* counts, uint64_t n)
{
	if (int rc = sig_check(e, plane, "ntc_signature_inject")) return rc;
	if (!hashes && n) return fail(NTC_ERR_ARG, "ntc_signature_inject: null argument");
	if (n == 0) return 0;
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	DevBuf<unsigned long long> k; // (buffers of the call: the engine's scratch may hold a compaction another call is about to read)
	DevBuf<uint32_t> c;
	if (!k.reserve(n * 8) || (counts && !c.reserve(n * 4))) return fail(NTC_ERR_MEMORY, "ntc_signature_inject: cannot allocate %llu B on device", (unsigned long long)(n * 12));
	HIP_TRY(hipMemcpyAsync(k, hashes, n * 8, hipMemcpyHostToDevice, e->stream));
	if (counts) HIP_TRY(hipMemcpyAsync(c, counts, n * 4, hipMemcpyHostToDevice, e->stream));
	const int rc = sig_inject_device(e, plane, k, counts ? c.get() : nullptr, n);
	HIP_TRY(hipStreamSynchronize(e->stream)); // (the host arrays and k, c are free on return)
	return rc;
}

int ntc_signature_stats(ntc_engine* e, uint64_t* slots, uint64_t* grows)
{
	if (int rc = sig_check(e, 0, "ntc_signature_stats")) return rc;
	if (!slots || !grows) return fail(NTC_ERR_ARG, "ntc_signature_stats: null argument");
	std::lock_guard<std::mutex> lk(e->mu);
	*slots = 0;
	for (const auto& p : e->sig_planes)
		*slots += p.slots;
	*grows = e->sig_grows;
	return 0;
}

int ntc_signature_time(ntc_engine* e, double* insert_ms, double* grow_ms) { return sig_times(e, "ntc_signature_time", T_SIG_INSERT, insert_ms, T_SIG_GROW, grow_ms); }

int ntc_signature_sort_time(ntc_engine* e, double* ms) { return sig_times(e, "ntc_signature_sort_time", T_SIG_SORT, ms); }

int ntc_signature_header(ntc_engine* e, uint32_t plane, ntc_sig_header* h)
{
	if (int rc = sig_check(e, plane, "ntc_signature_header")) return rc;
	if (!h) return fail(NTC_ERR_ARG, "ntc_signature_header: null argument");
	std::memset(h, 0, sizeof *h);
	h->k = e->klist[plane];
	h->gap = e->seeded ? 0u : e->kgap[plane];
	h->strand = e->strand;
	h->hpc = e->hpc ? 1u : 0u;
	h->s_bits = e->s_bits;
	const std::string m = e->plain(plane) ? std::string(h->k, '1') : e->masks[plane];
	std::memcpy(h->mask, m.data(), std::min<size_t>(m.size(), NTC_SIG_MASK_MAX - 1));
	return 0;
}

} // extern "C"
