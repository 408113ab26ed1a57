// ntc_submit.hip — the ntc_submit* entry points: device-resident batches as they come; host reads packed into a staging pair (tiles for the
// tiled kernels, length bins for ragged sets, row slots for the rest) and copied behind the engine's stream; long sequences cut into pieces on the
// device (ntc_submit_long_device; ntc_engine.hpp)
#include "ntc_engine.hpp"

using namespace ntc_eng;

namespace {

// A staging pair on loan to one submitting thread: packing happens outside the engine's lock, only copy + launch take it
struct StageLease {
	ntc_engine* e = nullptr;
	ntc_engine::StageSlot* sl = nullptr;
	StageLease() = default;
	StageLease(const StageLease&) = delete;
	StageLease& operator=(const StageLease&) = delete;
	~StageLease()
	{
		if (!sl) return;
		{
			std::lock_guard<std::mutex> lk(e->stage_mu);
			sl->busy = false;
		}
		e->stage_cv.notify_one();
	}
};

// take a free staging pair; wait (this thread only) until the GPU is done with its previous contents; grow it to stage_bytes (doubling)
int lease_stage(ntc_engine* e, size_t stage_bytes, StageLease& lease)
{
	HIP_TRY(hipSetDevice(e->device));
	{
		std::unique_lock<std::mutex> lk(e->stage_mu);
		auto free_slot = [&]() -> ntc_engine::StageSlot* {
			for (auto& c : e->stage)
				if (!c.busy) return &c;
			return nullptr;
		};
		e->stage_cv.wait(lk, [&] { return free_slot() != nullptr; });
		lease.e = e;
		lease.sl = free_slot();
		lease.sl->busy = true;
	}
	auto& sl = *lease.sl;
	if (sl.done == nullptr) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
	if (sl.used) HIP_TRY(hipEventSynchronize(sl.done));
	const size_t h_cap = std::max(stage_bytes, sl.h_stage.cap * 2), d_cap = std::max(stage_bytes, sl.d_stage.cap * 2);
	if (!sl.h_stage.reserve(stage_bytes, h_cap)) return fail(NTC_ERR_MEMORY, "ntc_submit: cannot pin %zu B", h_cap);
	if (!sl.d_stage.reserve(stage_bytes, d_cap)) return fail(NTC_ERR_MEMORY, "ntc_submit: cannot allocate %zu B on device", d_cap);
	return 0;
}

// behind the copies and launches of a leased pair (under e->mu).  The copies are in flight whatever the launches said (rc): the pair may only be
// reused after them, and nothing may still read the pinned side when it is handed out again
int end_stage_use(ntc_engine* e, ntc_engine::StageSlot& sl, int rc)
{
	sl.used = true;
	if (hipEventRecord(sl.done, e->stream) != hipSuccess) (void)hipStreamSynchronize(e->stream);
	return rc;
}

int stage_copy_failed(ntc_engine* e)
{
	(void)hipStreamSynchronize(e->stream);
	return fail(NTC_ERR_DEVICE, "ntc_submit: host to device copy failed");
}

// read i = bytes [ptr_of(i), ptr_of(i) + len_of(i)): ntc_submit (concatenated reads + offsets) and ntc_submit_spans (spans of
// a caller buffer, e.g. the sequence lines inside a block of a FASTQ file) pack into the pinned staging pair the same way
// (len_of / ptr_of are template callables: the packing loops call them once or twice per read, inlined).
// Equal-length reads of a host batch go to the device in the TILED layout: the packing loop writes each read's 16-byte pieces
// where ntc_submit_tiled_device expects them, so the reads the reference's parsers hand to ntRead (ntcard.cpp:182,203,230) reach the
// tiled kernels like a device-resident producer's do.
// ragged == false: every read is `len` bases long.  ragged == true: the reads are 16 C - 15 .. 16 C bases long, C = len / 16, and come
// LONGEST FIRST (so every tile is sorted): the tiles are followed, in the same staging buffer, by tails[tile][16] — the reads of the tile with more than d
// bases in their last piece — and the batch goes to ntc_submit_tiled_ragged_device's path.
// A host batch may hold several bins (HostBin: reads idx[0 .. n) of the caller's numbering, or 0 .. n when idx == nullptr): they are packed one behind the other into ONE
// staging buffer, copied once and hashed by ONE launch per k (run_tiled_segs).
struct HostBin {
	const uint64_t* idx;
	uint64_t n;
	uint32_t len;  // every read's length, or 16 C for a ragged bin
	bool ragged;
};
template <class LenFn, class PtrFn> int submit_tiled_host(ntc_engine* e, const HostBin* bins, uint32_t n_bins, const LenFn& len_of, const PtrFn& ptr_of)
{
	// sections: [tiles of bin 0][tails of bin 0][tiles of bin 1] ... (tile sections are multiples of 32 KiB, tails of 64 B: everything stays 16-byte aligned)
	std::vector<size_t> off(n_bins), tile_bytes(n_bins);
	size_t need = 0;
	for (uint32_t b = 0; b < n_bins; ++b) {
		off[b] = need;
		tile_bytes[b] = (size_t)ntc_tiled_bytes(bins[b].n, bins[b].len);
		need += tile_bytes[b] + (bins[b].ragged ? (size_t)((bins[b].n + ntc::kTileReads - 1) / ntc::kTileReads) * 64 : 0);
	}
	StageLease lease;
	if (int rc = lease_stage(e, need, lease)) return rc;
	auto& sl = *lease.sl;
	// ---- pack: piece c of read i of a bin -> ((tile * C + c) * 2048 + i % 2048) * 16 of the bin's section ----
	for (uint32_t b = 0; b < n_bins; ++b) {
		const HostBin& hb = bins[b];
		unsigned char* hs = sl.h_stage + off[b];
		const uint32_t C = (hb.len + 15u) / 16u;
		uint32_t* tails = reinterpret_cast<uint32_t*>(hs + tile_bytes[b]);
		if (hb.ragged) std::memset(tails, 0, (size_t)((hb.n + ntc::kTileReads - 1) / ntc::kTileReads) * 64);
		for (uint64_t i = 0; i < hb.n; ++i) {
			const uint64_t r = hb.idx ? hb.idx[i] : i;
			const char* src = ptr_of(r);
			const uint32_t tail = (uint32_t)(hb.ragged ? len_of(r) : hb.len) - (C - 1u) * 16u; // 1 .. 16 bases in the last piece
			unsigned char* dst = hs + ((i / ntc::kTileReads) * C * ntc::kTileReads + i % ntc::kTileReads) * 16u;
			for (uint32_t c = 0; c + 1u < C; ++c)
				std::memcpy(dst + (size_t)c * ntc::kTileReads * 16u, src + 16u * c, 16);
			unsigned char* last = dst + (size_t)(C - 1u) * ntc::kTileReads * 16u;
			std::memcpy(last, src + 16u * (C - 1u), tail);
			std::memset(last + tail, 'A', 16u - tail);
			if (hb.ragged)
				for (uint32_t d = 0; d < tail; ++d)
					++tails[(i / ntc::kTileReads) * 16u + d];
		}
	}
	std::lock_guard<std::mutex> lk(e->mu);
	if (hipMemcpyAsync(sl.d_stage, sl.h_stage, need, hipMemcpyHostToDevice, e->stream) != hipSuccess) return stage_copy_failed(e);
	std::vector<TiledSeg> segs(n_bins);
	for (uint32_t b = 0; b < n_bins; ++b)
		segs[b] = TiledSeg{sl.d_stage + off[b], bins[b].n, bins[b].len, bins[b].ragged ? reinterpret_cast<const uint32_t*>(sl.d_stage + off[b] + tile_bytes[b]) : nullptr};
	return end_stage_use(e, sl, run_tiled_segs(e, segs.data(), n_bins, 1, true)); // (the staging pair is recycled: its K1f may not be deferred)
}

// ---- row slots: the plan that ntc_submit's host packing and ntc_submit_long_device's gather both follow ----
// one slot per read, or — once a read is longer than cap_chunk — chunks of cap_chunk bytes that overlap by kmax - 1
struct RowPlan {
	uint32_t kmin = 0, kmax = 0, cap_chunk = 0, stride = 0;
	uint32_t ch = 0; // window starts per chunk
	uint64_t maxlen = 0, len0 = 0, n_slots = 0;
	bool uniform = true, chunked = false;
	std::vector<uint32_t> order; // not empty: the reads longest first
};

// false: no read can produce a k-mer (ntHashIterator.hpp:61-64)
template <class LenFn> bool plan_rows(const ntc_engine* e, uint64_t n_reads, const LenFn& len_of, RowPlan& p)
{
	p.kmax = *std::max_element(e->klist.begin(), e->klist.end());
	p.kmin = *std::min_element(e->klist.begin(), e->klist.end());
	p.len0 = len_of(0);
	for (uint64_t i = 0; i < n_reads; ++i) {
		const uint64_t l = len_of(i);
		p.maxlen = std::max(p.maxlen, l);
		p.uniform &= (l == p.len0);
	}
	if (p.maxlen < p.kmin) return false;
	p.cap_chunk = std::max<uint32_t>(kSlotCapMin, ((2 * p.kmax + 64) + 3) & ~3u);
	p.chunked = p.maxlen > p.cap_chunk;
	p.stride = pick_stride(p.chunked ? p.cap_chunk : p.maxlen, e->klist, e->max_seed_lds);
	p.ch = p.cap_chunk - (p.kmax - 1);
	if (!p.chunked) {
		p.n_slots = n_reads;
	} else {
		for (uint64_t i = 0; i < n_reads; ++i) {
			const uint64_t l = len_of(i);
			if (l < p.kmin) continue;
			p.n_slots += l <= p.cap_chunk ? 1 : (l - (p.kmax - 1) + p.ch - 1) / p.ch;
		}
	}
	// Reads of different lengths are packed longest first (counting sort: counting is order-independent, ntcard.cpp:142-143).
	// 64 consecutive slots form a wave, and a wave whose reads are equally long takes the kernel's fast path: with 5 % of
	// trimmed reads scattered through a batch almost every wave would be ragged (0.95 vs 0.76 ms per 8 M reads).
	if (!p.chunked && !p.uniform && n_reads < 0xffffffffull) {
		std::vector<uint64_t> first(p.maxlen + 2, 0);
		for (uint64_t i = 0; i < n_reads; ++i)
			++first[p.maxlen - len_of(i) + 1];
		for (uint64_t l = 1; l <= p.maxlen + 1; ++l)
			first[l] += first[l - 1];
		p.order.resize(n_reads);
		for (uint64_t i = 0; i < n_reads; ++i)
			p.order[first[p.maxlen - len_of(i)]++] = (uint32_t)i;
	}
	return true;
}

// the slots of a plan, in slot order: emit(read, first byte, bytes, window-start limit) -> 0 or an error, which ends the walk
template <class LenFn, class Emit> int emit_rows(const RowPlan& p, uint64_t n_reads, const LenFn& len_of, const Emit& emit)
{
	for (uint64_t j = 0; j < n_reads; ++j) {
		const uint64_t i = p.order.empty() ? j : p.order[j];
		const uint64_t l = len_of(i);
		if (p.chunked && l < p.kmin) continue;
		if (!p.chunked || l <= p.cap_chunk) {
			if (int rc = emit(i, (uint64_t)0, l, l)) return rc;
			continue;
		}
		for (uint64_t start = 0; start + (p.kmax - 1) < l || start == 0; start += p.ch) {
			const uint64_t nbytes = std::min<uint64_t>(p.cap_chunk, l - start);
			const bool last = start + p.cap_chunk >= l;
			if (int rc = emit(i, start, nbytes, last ? nbytes : (uint64_t)p.ch)) return rc;
			if (last) break;
		}
	}
	return 0;
}

// reads -> row slots (one slot per read, long sequences in overlapping chunks) -> K1
template <class LenFn, class PtrFn> int submit_rows(ntc_engine* e, uint64_t n_reads, const LenFn& len_of, const PtrFn& ptr_of)
{
	RowPlan p;
	if (!plan_rows(e, n_reads, len_of, p)) return 0;
	const uint64_t n_slots = p.n_slots;
	const uint32_t stride = p.stride;
	StageLease lease;
	if (int rc = lease_stage(e, (size_t)n_slots * stride + 16, lease)) return rc;
	auto& sl = *lease.sl;
	const bool need_meta = p.chunked || !p.uniform;
	if (need_meta && !(sl.h_meta.reserve(n_slots * 4, sl.h_meta.cap * 2) && sl.d_meta.reserve(n_slots * 4, sl.d_meta.cap * 2)))
		return fail(NTC_ERR_MEMORY, "ntc_submit: cannot allocate slot metadata");
	// ---- pack (the copy the ABI promises: caller's buffers are free on return) ----
	unsigned char* hs = sl.h_stage;
	uint64_t slot = 0;
	// one slot: nbytes of the read from `start`, padded; its meta word = bytes | window-start limit << 16
	(void)emit_rows(p, n_reads, len_of, [&](uint64_t i, uint64_t start, uint64_t nbytes, uint64_t limit) {
		unsigned char* dst = hs + slot * stride;
		std::memcpy(dst, ptr_of(i) + start, nbytes);
		std::memset(dst + nbytes, 'A', stride - nbytes);
		if (need_meta) sl.h_meta[slot] = (uint32_t)nbytes | ((uint32_t)limit << 16);
		++slot;
		return 0;
	});
	if (slot != n_slots) return fail(NTC_ERR_STATE, "ntc_submit: internal slot plan mismatch (%llu != %llu)", (unsigned long long)slot, (unsigned long long)n_slots);
	// ---- enqueue: copy + kernels, in order on the engine's stream (asynchronous; ntc_sync / ntc_finish wait) ----
	std::lock_guard<std::mutex> lk(e->mu);
	if (hipMemcpyAsync(sl.d_stage, hs, (size_t)n_slots * stride, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
	    (need_meta && hipMemcpyAsync(sl.d_meta, sl.h_meta, n_slots * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess))
		return stage_copy_failed(e);
	return end_stage_use(e, sl, run_batch(e, sl.d_stage, need_meta ? sl.d_meta.get() : nullptr, n_slots, (uint32_t)p.len0, stride));
}

// ---- long sequences as pieces (include/ntcard_hip.h: ntc_submit_long_device; DESIGN.md §4 "Long sequences") ----
// A sequence of n >= L bytes is cut, ON THE DEVICE, into m = ntc_long_plan(kmax, ..) full pieces [j S, j S + L), S = L - (kmax - 1): an equal-length tiled
// batch of "reads" for K1h + K1f.  Every k of the list counts the windows that START in a piece's first S bytes — those of a read of L - (kmax - k) bases
// (TiledSeg::cut_k) — so every window of k bases lies in exactly one piece or in the remainder [m S, n).  Remainders that hold a window of kmin and sequences
// shorter than L are gathered into row slots (the plan above) for K1.  An engine that does not qualify (long_fast) gathers every sequence whole:
// ntc_submit's results from device-resident bytes.
constexpr uint32_t kLongPieceDefault = 1008;   // profiles/long_seq.txt
constexpr uint64_t kLongMinNever = ~0ull;
constexpr uint64_t kLongMinDefault = 32768;   // host batches: full pieces from which the sequences of >= 2 pieces take this path (profiles/long_seq.txt: slower
                                               // than row slots at 8 Ki pieces, level at 16 Ki, 19 % faster at 32 Ki); NTC_LONG_MIN=0: never
constexpr uint64_t kLongRoundBytes = 1ull << 30; // scratch of one round: a 30 GB sequence set is cut and counted 1 GiB of tiles at a time
constexpr uint32_t kLongMaxSpread = 15;         // kmax - kmin of a list: the trimmed length of every k stays within the piece's last chunk, the ordinary
                                                 // equal-length case of the tiled kernels (150 bp reads: 10 chunks, 10 bases in the last)

uint32_t long_kmax(const ntc_engine* e) { return *std::max_element(e->klist.begin(), e->klist.end()); }
uint32_t long_kmin(const ntc_engine* e) { return *std::min_element(e->klist.begin(), e->klist.end()); }

// every plane K1h's, and one plane (the tiled -g seeds among them) or a list of plain k within kLongMaxSpread
bool long_fast(const ntc_engine* e)
{
	if (!e->ts_all) return false;
	if (e->klist.size() == 1) return true;
	for (size_t ki = 0; ki < e->klist.size(); ++ki)
		if (!e->plain(ki)) return false;
	return long_kmax(e) - long_kmin(e) <= kLongMaxSpread;
}

int grow_long(ntc_engine* e, size_t need)
{
	if (need <= e->d_long.cap) return 0;
	HIP_TRY(hipStreamSynchronize(e->stream));
	if (!e->d_long.reserve(need)) return fail(NTC_ERR_MEMORY, "cannot allocate %zu B of scratch for long sequences on device", need);
	return 0;
}

// under e->mu: the rounds of one call — cut + K1h + K1f over the pieces, gather + K1 over the row slots; d_seqs / d_spans: the call's tables on the device
int run_long_rounds(ntc_engine* e, const unsigned char* d_src, const ntc::LongSeq* d_seqs, uint64_t n_pieces, uint64_t n_cut_seqs, const ntc::LongSpan* d_spans,
                    uint64_t n_slots, const RowPlan& rp, uint32_t L)
{
	const uint32_t kmax = long_kmax(e), cut_k = e->klist.size() > 1 ? kmax : 0u; // (one plane: the pieces are ordinary reads)
	uint64_t round = kLongRoundBytes;
	if (const char* ev = std::getenv("NTC_LONG_ROUND_BYTES")) round = std::max(1ll, std::strtoll(ev, nullptr, 10)); // tests: several rounds of a small input
	if (n_pieces) {
		const uint64_t per_round = std::max<uint64_t>(1, round / ((uint64_t)L * ntc::kTileReads)) * ntc::kTileReads; // whole tiles
		for (uint64_t first = 0; first < n_pieces; first += per_round) {
			const uint64_t np = std::min(per_round, n_pieces - first);
			if (int rc = grow_long(e, (size_t)ntc_tiled_bytes(np, L))) return rc;
			if (int rc = close_run(e)) return rc;
			Span sp;
			if (int rc = open_span(e, sp)) return rc;
			HIP_TRY(ntc::launch_cut_tiles(d_src, d_seqs, (uint32_t)n_cut_seqs, first, np, L - (kmax - 1u), L, e->d_long, e->stream));
			if (int rc = close_span(sp, e->stream, e->timers[T_LONG_CUT].spans)) return rc;
			const TiledSeg sg{e->d_long, np, L, nullptr, cut_k};
			if (int rc = run_tiled_segs(e, &sg, 1, 1, true)) return rc; // (the tiles are recycled by the next round: their K1f may not be deferred)
			e->long_pieces += np;
		}
		e->long_seqs += n_cut_seqs;
	}
	if (n_slots) {
		const uint64_t per_round = std::max<uint64_t>(64, (round / (rp.stride + 4u)) & ~63ull);
		for (uint64_t first = 0; first < n_slots; first += per_round) {
			const uint64_t ns = std::min(per_round, n_slots - first);
			const size_t rows_bytes = ((size_t)ns * rp.stride + 16 + 15) & ~(size_t)15; // the slots, then their meta words
			if (int rc = grow_long(e, rows_bytes + (size_t)ns * 4)) return rc;
			if (int rc = close_run(e)) return rc;
			uint32_t* d_meta = reinterpret_cast<uint32_t*>(e->d_long + rows_bytes);
			Span sp;
			if (int rc = open_span(e, sp)) return rc;
			HIP_TRY(ntc::launch_gather_slots(d_src, d_spans + first, ns, rp.stride, e->d_long, d_meta, e->stream));
			if (int rc = close_span(sp, e->stream, e->timers[T_LONG_GATHER].spans)) return rc;
			if (int rc = run_batch(e, e->d_long, d_meta, ns, (uint32_t)rp.len0, rp.stride)) return rc;
		}
	}
	return 0;
}

// sequence i = the len_of(i) bytes from d_src + off_of(i).  The tables (16 B per sequence with a full piece, 16 B per row slot) are built in the leased pair's
// meta buffers: the pieces' offsets are derived from them on the device (cut_tiles_kernel), so the host's work and the bytes it sends do not grow with the pieces.
// h2d_bytes != 0: d_src is the pair's device side, whose first h2d_bytes the host has filled (ntc_submit's long sequences)
template <class LenFn, class OffFn>
int submit_long_leased(ntc_engine* e, ntc_engine::StageSlot& sl, const unsigned char* d_src, size_t h2d_bytes, uint64_t n_seqs, const LenFn& len_of,
                       const OffFn& off_of, uint32_t L)
{
	const bool fast = long_fast(e);
	const uint32_t kmin = long_kmin(e);
	const uint64_t S = fast ? L - (long_kmax(e) - 1u) : 1u;
	struct Item {
		uint64_t src, len;
	};
	std::vector<Item> items;        // what goes to row slots: remainders that hold a window of kmin, sequences without a full piece
	std::vector<ntc::LongSeq> cuts; // the sequences with a full piece
	uint64_t n_pieces = 0;
	for (uint64_t i = 0; i < n_seqs; ++i) {
		const uint64_t n = len_of(i);
		const uint64_t m = fast && n >= L ? (n - L) / S + 1u : 0u; // (ntc_long_plan)
		if (m != 0) cuts.push_back(ntc::LongSeq{off_of(i), n_pieces});
		n_pieces += m;
		if (m == 0 || n - m * S >= kmin) items.push_back(Item{off_of(i) + m * S, n - m * S});
	}
	const uint64_t n_cut_seqs = cuts.size();
	if (n_cut_seqs >= (1ull << 31)) return fail(NTC_ERR_ARG, "ntc_submit_long_device: %llu sequences with a full piece in one call (at most 2^31 - 1)", (unsigned long long)n_cut_seqs);
	cuts.push_back(ntc::LongSeq{0, n_pieces}); // the sentinel
	const auto item_len = [&](uint64_t i) { return items[i].len; };
	RowPlan rp;
	const uint64_t n_slots = !items.empty() && plan_rows(e, items.size(), item_len, rp) ? rp.n_slots : 0;
	if (n_pieces == 0 && n_slots == 0) return 0;
	const size_t seq_bytes = n_pieces ? cuts.size() * sizeof(ntc::LongSeq) : 0, tab_bytes = seq_bytes + (size_t)n_slots * sizeof(ntc::LongSpan);
	if (!(sl.h_meta.reserve(tab_bytes, sl.h_meta.cap * 2) && sl.d_meta.reserve(tab_bytes, sl.d_meta.cap * 2)))
		return fail(NTC_ERR_MEMORY, "ntc_submit_long_device: cannot allocate %zu B of sequence and slot tables", tab_bytes);
	unsigned char* h_tab = reinterpret_cast<unsigned char*>(sl.h_meta.get());
	if (seq_bytes) std::memcpy(h_tab, cuts.data(), seq_bytes);
	ntc::LongSpan* h_spans = reinterpret_cast<ntc::LongSpan*>(h_tab + seq_bytes);
	uint64_t slot = 0;
	if (n_slots)
		(void)emit_rows(rp, items.size(), item_len, [&](uint64_t i, uint64_t start, uint64_t nbytes, uint64_t limit) {
			h_spans[slot++] = ntc::LongSpan{items[i].src + start, (uint32_t)nbytes, (uint32_t)limit};
			return 0;
		});
	if (slot != n_slots) return fail(NTC_ERR_STATE, "ntc_submit_long_device: internal plan mismatch");
	std::lock_guard<std::mutex> lk(e->mu);
	if ((h2d_bytes && hipMemcpyAsync(sl.d_stage, sl.h_stage, h2d_bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess) ||
	    hipMemcpyAsync(sl.d_meta, sl.h_meta, tab_bytes, hipMemcpyHostToDevice, e->stream) != hipSuccess)
		return stage_copy_failed(e);
	const unsigned char* d_tab = reinterpret_cast<const unsigned char*>(sl.d_meta.get());
	return end_stage_use(e, sl, run_long_rounds(e, d_src, reinterpret_cast<const ntc::LongSeq*>(d_tab), n_pieces, n_cut_seqs,
	                                            reinterpret_cast<const ntc::LongSpan*>(d_tab + seq_bytes), n_slots, rp, L));
}

// what submit_impl leaves to row slots.  On an engine that qualifies (long_fast) the sequences of at least two full pieces are copied raw and contiguous
// into the staging pair — one memcpy each, their bytes cross PCIe once — and cut on the device, once together they hold long_min full pieces
// (NTC_LONG_MIN: tuning runs, tools/long_time.py); everything else takes row slots as before
template <class LenFn, class PtrFn> int submit_rows_or_long(ntc_engine* e, uint64_t n_reads, const LenFn& len_of, const PtrFn& ptr_of)
{
	uint64_t long_min = kLongMinDefault;
	if (const char* ev = std::getenv("NTC_LONG_MIN")) {
		const long long v = std::strtoll(ev, nullptr, 10);
		long_min = v >= 1 ? (uint64_t)v : kLongMinNever;
	}
	if (long_min == kLongMinNever || !long_fast(e)) return submit_rows(e, n_reads, len_of, ptr_of);
	const uint32_t L = kLongPieceDefault;
	const uint64_t S = L - (long_kmax(e) - 1u);
	std::vector<uint64_t> sel, rest;
	uint64_t pieces = 0;
	size_t bytes = 0;
	for (uint64_t i = 0; i < n_reads; ++i) {
		const uint64_t n = len_of(i);
		if (n >= L + S) {
			pieces += (n - L) / S + 1u;
			bytes += n;
			sel.push_back(i);
		} else {
			rest.push_back(i);
		}
	}
	if (sel.empty() || pieces < long_min) return submit_rows(e, n_reads, len_of, ptr_of);
	{
		StageLease lease;
		if (int rc = lease_stage(e, bytes + 16, lease)) return rc;
		auto& sl = *lease.sl;
		std::vector<uint64_t> off(sel.size() + 1, 0);
		for (size_t j = 0; j < sel.size(); ++j) {
			std::memcpy(sl.h_stage + off[j], ptr_of(sel[j]), len_of(sel[j]));
			off[j + 1] = off[j] + len_of(sel[j]);
		}
		if (int rc = submit_long_leased(e, sl, sl.d_stage, bytes, sel.size(), [&](uint64_t j) { return off[j + 1] - off[j]; }, [&](uint64_t j) { return off[j]; }, L))
			return rc;
	}
	if (rest.empty()) return 0;
	return submit_rows(e, rest.size(), [&](uint64_t i) { return len_of(rest[i]); }, [&](uint64_t i) { return ptr_of(rest[i]); });
}

template <class LenFn, class PtrFn> int submit_impl(ntc_engine* e, uint64_t n_reads, const LenFn& len_of, const PtrFn& ptr_of)
{
	const uint32_t kmin = *std::min_element(e->klist.begin(), e->klist.end());
	if (e->ts_ok && n_reads >= 1024) {
		// Reads of ONE length (an untrimmed FASTQ file) are one tiled batch.  Otherwise the reads are binned by their number of 16-base pieces,
		// C = ceil(len / 16): every bin of at least 32 Ki reads becomes a RAGGED tiled batch — sorted longest first, K1h masks the windows
		// behind every read's end — all of them hashed by ONE launch per k that shares its workgroups among the bins (run_tiled_segs), and what is left
		// (thin bins, reads shorter than every k, sequences beyond 64 Ki bases) takes row slots and K1.  profiles/r05_ragged_host.txt: 8 M reads of which
		// 5 % are trimmed to 50 .. 149 bp: 0.483 ms with bins from 32 Ki reads, 0.527 from 512 Ki (the thin bins through K1), 0.728 through K1 alone;
		// lengths uniform in 100 .. 150: 0.385 against 0.647.  (With one launch PER BIN, the first form of this, thin bins lost to K1 and the bar was 512 Ki.)
		// NTC_FLAG_REQUIRE_TILED, the validation flag, lowers the bar to 1024 reads.
		uint32_t bin_min = e->ts_required ? 1024u : 32u * 1024u;
		if (const char* ev = std::getenv("NTC_BIN_MIN")) bin_min = (uint32_t)std::max(1024l, std::strtol(ev, nullptr, 10)); // tuning runs (tools/ragged_time.py)
		const uint64_t len0 = len_of(0);
		uint64_t same = 0;
		for (uint64_t i = 0; i < n_reads; ++i)
			same += len_of(i) == len0;
		if (same == n_reads) {
			if (len0 >= kmin && len0 <= 0xffffu && k1_fits_tiles(e, (uint32_t)len0)) { // (a mixed list with reads too long for K1's tiled staging: row slots, chunked)
				const HostBin one{nullptr, n_reads, (uint32_t)len0, false};
				return submit_tiled_host(e, &one, 1, len_of, ptr_of);
			}
		} else { // (also under a list of which a part is K1's — K1 gets a slot table derived from the tiles' prefix tables)
			constexpr uint32_t kMaxC = 0x10000u / 16u;
			std::vector<uint32_t> per_c(kMaxC + 1, 0u);
			for (uint64_t i = 0; i < n_reads; ++i) {
				const uint64_t l = len_of(i);
				if (l >= kmin && l <= 0xffffu) ++per_c[(l + 15u) / 16u];
			}
			std::vector<uint64_t> rest;
			std::vector<std::vector<uint64_t>> bins; // (only the bins that are taken)
			std::vector<int32_t> bin_of(kMaxC + 1, -1);
			for (uint32_t c = 1; c <= kMaxC; ++c)
				if (per_c[c] >= bin_min && k1_fits_tiles(e, 16u * c)) {
					bin_of[c] = (int32_t)bins.size();
					bins.emplace_back();
					bins.back().reserve(per_c[c]);
				}
			if (!bins.empty()) {
				for (uint64_t i = 0; i < n_reads; ++i) {
					const uint64_t l = len_of(i);
					const int32_t b = (l >= kmin && l <= 0xffffu) ? bin_of[(l + 15u) / 16u] : -1;
					if (b >= 0) bins[(size_t)b].push_back(i);
					else rest.push_back(i);
				}
				std::vector<HostBin> hbins;
				for (uint32_t c = kMaxC; c >= 1; --c) { // (longest bin first)
					if (bin_of[c] < 0) continue;
					std::vector<uint64_t>& idx = bins[(size_t)bin_of[c]];
					// longest first: a counting sort by the 16 possible tails (stable)
					std::vector<uint64_t> sorted(idx.size());
					size_t start[17] = { 0 };
					for (uint64_t i : idx)
						++start[16u - (uint32_t)(len_of(i) - 16u * (c - 1u))]; // tail 16 -> bucket 0
					size_t acc = 0;
					for (int t = 0; t < 17; ++t) {
						const size_t n = start[t];
						start[t] = acc;
						acc += n;
					}
					for (uint64_t i : idx)
						sorted[start[16u - (uint32_t)(len_of(i) - 16u * (c - 1u))]++] = i;
					idx.swap(sorted);
					hbins.push_back(HostBin{idx.data(), idx.size(), 16u * c, true});
				}
				// all the bins in one staging buffer and one launch per k (up to 8 bins: run_tiled_segs groups the rest)
				if (int rc = submit_tiled_host(e, hbins.data(), (uint32_t)hbins.size(), len_of, ptr_of)) return rc;
				if (rest.empty()) return 0;
				return submit_rows_or_long(e, rest.size(), [&](uint64_t i) { return len_of(rest[i]); }, [&](uint64_t i) { return ptr_of(rest[i]); });
			}
		}
	}
	return submit_rows_or_long(e, n_reads, len_of, ptr_of);
}

// ---- homopolymer compression (include/ntcard_hip.h: NTC_FLAG_HPC; DESIGN.md §4 "Homopolymer compression") ----
constexpr uint64_t kHpcRoundBytes = 1ull << 30; // source bytes of one round of ntc_submit_long_device's compaction (NTC_HPC_ROUND_BYTES)

int hpc_fixed_layout(const ntc_engine*, const char* who)
{
	return fail(NTC_ERR_ARG, "%s: a fixed-layout batch fixes every read's length, which homopolymer compression changes (NTC_FLAG_HPC): use ntc_submit, ntc_submit_spans or ntc_submit_long_device; nothing was counted", who);
}

// host reads: every read compressed into a temporary batch, which then takes submit_impl's routes — tiles, bins, rows, the path behind NTC_LONG_MIN
template <class LenFn, class PtrFn> int submit_hpc_host(ntc_engine* e, uint64_t n_reads, const LenFn& len_of, const PtrFn& ptr_of)
{
	uint64_t total = 0;
	for (uint64_t i = 0; i < n_reads; ++i)
		total += len_of(i);
	std::vector<char> buf(total ? total : 1);
	std::vector<uint64_t> off(n_reads + 1, 0);
	for (uint64_t i = 0; i < n_reads; ++i) {
		uint64_t m = 0;
		if (int rc = ntc_hpc_compress(ptr_of(i), len_of(i), buf.data() + off[i], &m)) return rc;
		off[i + 1] = off[i] + m;
	}
	if (int rc = submit_impl(e, n_reads, [&](uint64_t i) { return off[i + 1] - off[i]; }, [&](uint64_t i) { return buf.data() + off[i]; })) return rc;
	std::lock_guard<std::mutex> lk(e->mu);
	e->hpc_bytes_in += total;
	e->hpc_bytes_out += off[n_reads];
	return 0;
}

// ntc_submit_long_device on an engine with the flag: rounds of whole sequences — compact into d_hpc, bring the new offsets back (the ONE wait per round:
// the planner of the cut is host code), count (d_hpc, new offsets) exactly as the caller's buffer is counted without the flag.  The caller's source is
// only read by the compaction, which is in the stream when the call returns.
int submit_long_hpc(ntc_engine* e, const unsigned char* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint32_t L)
{
	uint64_t budget = kHpcRoundBytes;
	if (const char* ev = std::getenv("NTC_HPC_ROUND_BYTES")) budget = (uint64_t)std::max(1ll, std::strtoll(ev, nullptr, 10)); // tests: several rounds of a small input
	std::lock_guard<std::mutex> hk(e->hpc_mu);
	std::vector<uint64_t> noff;
	for (uint64_t s0 = 0, s1; s0 < n_seqs; s0 = s1) {
		for (s1 = s0 + 1; s1 < n_seqs && offsets[s1 + 1] - offsets[s0] <= budget;) // (a sequence beyond the budget is a round of its own)
			++s1;
		const uint64_t ns = s1 - s0, n = offsets[s1] - offsets[s0];
		noff.assign(ns + 1, 0);
		if (n != 0) {
			std::lock_guard<std::mutex> lk(e->mu);
			HIP_TRY(hipSetDevice(e->device));
			const size_t aux_bytes = ntc::hpc_aux_bytes(n, ns);
			if (n > e->d_hpc.cap || aux_bytes > e->d_hpc_aux.cap) {
				HIP_TRY(hipStreamSynchronize(e->stream)); // (the round before may still be counting from the scratch)
				if (!e->d_hpc.reserve(n) || !e->d_hpc_aux.reserve(aux_bytes))
					return fail(NTC_ERR_MEMORY, "ntc_submit_long_device: cannot allocate %zu B of scratch for homopolymer compression on device", (size_t)n + aux_bytes);
			}
			if (int rc = close_run(e)) return rc;
			Span sp;
			if (int rc = open_span(e, sp)) return rc;
			HIP_TRY(ntc::launch_hpc_compact(d_bases, offsets + s0, ns, e->d_hpc, e->d_hpc_aux.get(), e->stream));
			if (int rc = close_span(sp, e->stream, e->timers[T_HPC].spans)) return rc;
			HIP_TRY(hipMemcpyAsync(noff.data(), ntc::hpc_aux_offsets(e->d_hpc_aux.get(), ns), (ns + 1) * 8, hipMemcpyDeviceToHost, e->stream));
			HIP_TRY(hipStreamSynchronize(e->stream));
			e->hpc_bytes_in += n;
			e->hpc_bytes_out += noff[ns];
		}
		StageLease lease;
		if (int rc = lease_stage(e, 0, lease)) return rc; // (its meta buffers hold the round's tables)
		if (int rc = submit_long_leased(e, *lease.sl, e->d_hpc.get(), 0, ns, [&](uint64_t i) { return noff[i + 1] - noff[i]; }, [&](uint64_t i) { return noff[i]; }, L))
			return rc;
	}
	return 0;
}

} // namespace

extern "C" {

int ntc_submit(ntc_engine* e, const char* bases, const uint64_t* offsets, uint64_t n_reads)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit: null engine");
	if (n_reads == 0) return 0;
	if (!bases || !offsets) return fail(NTC_ERR_ARG, "ntc_submit: null buffer");
	for (uint64_t i = 0; i < n_reads; ++i)
		if (offsets[i + 1] < offsets[i]) return fail(NTC_ERR_ARG, "ntc_submit: offsets not monotone at read %llu", (unsigned long long)i);
	if (e->hpc) return submit_hpc_host(e, n_reads, [&](uint64_t i) { return offsets[i + 1] - offsets[i]; }, [&](uint64_t i) { return bases + offsets[i]; });
	return submit_impl(e, n_reads, [&](uint64_t i) { return offsets[i + 1] - offsets[i]; }, [&](uint64_t i) { return bases + offsets[i]; });
}

int ntc_submit_spans(ntc_engine* e, const char* buf, const uint64_t* starts, const uint32_t* lens, uint64_t n_reads)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_spans: null engine");
	if (n_reads == 0) return 0;
	if (!buf || !starts || !lens) return fail(NTC_ERR_ARG, "ntc_submit_spans: null buffer");
	if (e->hpc) return submit_hpc_host(e, n_reads, [&](uint64_t i) { return (uint64_t)lens[i]; }, [&](uint64_t i) { return buf + starts[i]; });
	return submit_impl(e, n_reads, [&](uint64_t i) { return (uint64_t)lens[i]; }, [&](uint64_t i) { return buf + starts[i]; });
}

int ntc_submit_device(ntc_engine* e, const void* d_slots, uint64_t n_reads, uint32_t read_len, uint32_t stride)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_device: null engine");
	if (e->hpc) return hpc_fixed_layout(e, "ntc_submit_device");
	if (n_reads == 0) return 0;
	if (!d_slots || (stride & 3u) || stride < read_len || ((uintptr_t)d_slots & 15u))
		return fail(NTC_ERR_ARG, "ntc_submit_device: need 16-byte aligned slots, stride %% 4 == 0, stride >= read_len");
	if (read_len > 0xffffu) return fail(NTC_ERR_ARG, "ntc_submit_device: read_len %u > 65535", read_len);
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return run_batch(e, (const unsigned char*)d_slots, nullptr, n_reads, read_len, stride);
}

int ntc_submit_long_device(ntc_engine* e, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint32_t piece_len)
{
	// (what needs no engine first, so that a bad call is told apart before a device is looked for)
	if (n_seqs && !offsets) return fail(NTC_ERR_ARG, "ntc_submit_long_device: null offsets");
	if ((piece_len & 15u) || piece_len > 65520u) return fail(NTC_ERR_ARG, "ntc_submit_long_device: piece_len %u is not 0 or a multiple of 16 up to 65520", piece_len);
	for (uint64_t i = 0; i < n_seqs; ++i)
		if (offsets[i + 1] < offsets[i]) return fail(NTC_ERR_ARG, "ntc_submit_long_device: offsets not monotone at sequence %llu", (unsigned long long)i);
	if (n_seqs && offsets[n_seqs] > offsets[0] && !d_bases) return fail(NTC_ERR_ARG, "ntc_submit_long_device: null buffer");
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_long_device: null engine");
	if (n_seqs == 0) return 0;
	const bool fast = long_fast(e);
	if (!fast && e->ts_required)
		return fail(NTC_ERR_ARG, "ntc_submit_long_device: the tiled kernels do not serve this configuration (NTC_FLAG_REQUIRE_TILED); nothing was counted");
	const uint32_t L = piece_len ? piece_len : kLongPieceDefault;
	if (fast && L < long_kmax(e) + 15u)
		return fail(NTC_ERR_ARG, "ntc_submit_long_device: piece_len %u below k + 15 = %u (k: the largest of the list)", L, long_kmax(e) + 15u);
	if (e->hpc) return submit_long_hpc(e, (const unsigned char*)d_bases, offsets, n_seqs, L);
	StageLease lease;
	if (int rc = lease_stage(e, 0, lease)) return rc; // (its meta buffers hold the call's tables)
	return submit_long_leased(e, *lease.sl, (const unsigned char*)d_bases, 0, n_seqs, [&](uint64_t i) { return offsets[i + 1] - offsets[i]; },
	                          [&](uint64_t i) { return offsets[i]; }, L);
}

int ntc_submit_tiled_device(ntc_engine* e, const void* d_tiles, uint64_t n_reads, uint32_t read_len)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_tiled_device: null engine");
	if (e->hpc) return hpc_fixed_layout(e, "ntc_submit_tiled_device");
	if (n_reads == 0) return 0;
	if (!d_tiles || ((uintptr_t)d_tiles & 15u)) return fail(NTC_ERR_ARG, "ntc_submit_tiled_device: need a 16-byte aligned buffer");
	if (read_len == 0 || read_len > 0xffffu) return fail(NTC_ERR_ARG, "ntc_submit_tiled_device: read_len %u outside 1..65535", read_len);
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return defer_or_run_tiled(e, TiledSeg{(const unsigned char*)d_tiles, n_reads, read_len, nullptr});
}

int ntc_submit_tiled_ragged_device(ntc_engine* e, const void* d_tiles, uint64_t n_reads, uint32_t n_chunks, const uint32_t* d_tails)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_tiled_ragged_device: null engine");
	if (e->hpc) return hpc_fixed_layout(e, "ntc_submit_tiled_ragged_device");
	if (n_reads == 0) return 0;
	if (!d_tiles || ((uintptr_t)d_tiles & 15u) || !d_tails || ((uintptr_t)d_tails & 3u)) return fail(NTC_ERR_ARG, "ntc_submit_tiled_ragged_device: need a 16-byte aligned tile buffer and a tails array");
	if (n_chunks == 0 || n_chunks > 0xffffu / 16u) return fail(NTC_ERR_ARG, "ntc_submit_tiled_ragged_device: n_chunks %u outside 1..4095", n_chunks);
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return defer_or_run_tiled(e, TiledSeg{(const unsigned char*)d_tiles, n_reads, 16u * n_chunks, d_tails});
}

int ntc_submit_tiled_bins_device(ntc_engine* e, uint32_t n_bins, const void* const* d_tiles, const uint64_t* n_reads, const uint32_t* read_len,
                                 const uint32_t* const* d_tails)
{
	if (!e) return fail(NTC_ERR_ARG, "ntc_submit_tiled_bins_device: null engine");
	if (e->hpc) return hpc_fixed_layout(e, "ntc_submit_tiled_bins_device");
	if (n_bins == 0) return 0;
	if (!d_tiles || !n_reads || !read_len) return fail(NTC_ERR_ARG, "ntc_submit_tiled_bins_device: null argument"); // (d_tails == NULL: every bin is equal-length)
	std::vector<TiledSeg> segs;
	for (uint32_t i = 0; i < n_bins; ++i) {
		if (n_reads[i] == 0) continue;
		const uint32_t* tails_i = d_tails ? d_tails[i] : nullptr;
		if (!d_tiles[i] || ((uintptr_t)d_tiles[i] & 15u) || ((uintptr_t)tails_i & 3u)) return fail(NTC_ERR_ARG, "ntc_submit_tiled_bins_device: bin %u: need a 16-byte aligned tile buffer", i);
		if (read_len[i] == 0 || read_len[i] > 0xffffu || (tails_i && (read_len[i] & 15u)))
			return fail(NTC_ERR_ARG, "ntc_submit_tiled_bins_device: bin %u: read_len %u (a ragged bin's is 16 x its chunks, at most 65520)", i, read_len[i]);
		segs.push_back(TiledSeg{(const unsigned char*)d_tiles[i], n_reads[i], read_len[i], tails_i});
	}
	if (segs.empty()) return 0;
	std::lock_guard<std::mutex> lk(e->mu);
	HIP_TRY(hipSetDevice(e->device));
	return run_tiled_segs(e, segs.data(), (uint32_t)segs.size());
}

} // extern "C"
