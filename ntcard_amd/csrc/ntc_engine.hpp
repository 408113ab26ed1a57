// ntc_engine.hpp — the engine behind the C ABI (include/ntcard_hip.h): its state, the owners of its device resources and the functions its
// translation units share.  ntc_plan.hip: launch geometry and policy (no HIP calls); ntc_launch.hip: everything that enters the engine's stream;
// ntc_submit.hip: host packing, length bins, the staging pool; ntc_lifecycle.hip: create .. finish and the queries; ntc_merge.hip: multi-GPU merge
// and log exchange; ntc_device_tools.hip: the entry points that need no engine.  Signatures: ntc_signature.hip: the container's kernels, the engine's
// glue and the entry points that take an engine; those that need none sit with their kernels — ntc_sig_sort.hip: sort; ntc_sig_lists.hip: SigLists (lists on the
// device, their ascent check), compare, matrix; ntc_sig_gather.hip: gather; ntc_sig_algebra.hip: union, select, hist; ntc_sig_device.hpp is what these five share; ntc_sig_file.cpp: the signature file
// format and the host compare, plain host C++ like ntc_estimator.cpp.
//
// Host-side mirror of the reference seam B2: ntc_create = the allocation/zeroing main() does (ntcard.cpp:433-439),
// ntc_submit = a batch of ntRead/stRead calls (ntcard.cpp:147-171), ntc_finish = the state compEst reads (ntcard.cpp:237-247) + F1
// (ntcard.cpp:464-466).  No CPU fallback exists: every entry point needs a live HIP device.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ntcard_hip.h"
#include "ntc_kernels.hpp"

// sets ntc_last_error() and returns `code`: for the translation units outside ntc_eng (ntc_estimator.cpp, ntc_sig_file.cpp)
int ntc_internal_fail(int code, const char* fmt, ...);

namespace ntc_eng {

int fail(int code, const char* fmt, ...); // the same, for the engine's own files

#define HIP_TRY(expr)                                                                               \
	do {                                                                                            \
		hipError_t e__ = (expr);                                                                    \
		if (e__ != hipSuccess)                                                                      \
			return ntc_eng::fail(NTC_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e__));  \
	} while (0)

constexpr uint32_t kMaxK = 600; // the closed-form table (k x 128 B) and one wave of host slots (64 x ~2k B) share the 160 KiB of LDS; 600 is tested, 640 no longer fits
constexpr uint32_t kSlotCapMin = 256; // host packing: slot capacity (bytes) for ragged batches
constexpr size_t kMaxDynLds = 160 * 1024 - 2048; // 160 KiB minus the largest static LDS of any kernel here

// kernel kinds: the simple validation kernel (K1s/K1d) and the production kernels (K1)
enum { KIND_SIMPLE = 0, KIND_HF = 2 };

// A device allocation (kPinned: pinned host memory) with one owner: grow-only, freed by its destructor, converts to its pointer.
// reserve() neither waits for the stream nor keeps the old contents: a caller whose buffer may be in flight synchronises first.
template <class T, bool kPinned = false> struct Buf {
	T* p = nullptr;
	size_t cap = 0; // bytes
	Buf() = default;
	Buf(const Buf&) = delete;
	Buf& operator=(const Buf&) = delete;
	Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
	Buf& operator=(Buf&& o) noexcept
	{
		std::swap(p, o.p);
		std::swap(cap, o.cap);
		return *this;
	}
	~Buf() { reset(); }
	void reset()
	{
		if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
		p = nullptr, cap = 0;
	}
	// true: at least `need` bytes are there.  A buffer that is too small is freed and max(need, at_least) bytes are allocated — the caller's growth
	// rule: nothing = exactly the need, 2 * cap = doubling, a constant = a floor; false: no memory (the buffer is then empty)
	bool reserve(size_t need, size_t at_least = 0)
	{
		if (need <= cap) return true;
		reset();
		const size_t n = std::max(need, at_least);
		if ((kPinned ? hipHostMalloc((void**)&p, n, hipHostMallocDefault) : hipMalloc((void**)&p, n)) != hipSuccess) {
			p = nullptr;
			return false;
		}
		cap = n;
		return true;
	}
	bool upload(const std::vector<uint32_t>& h) { return reserve(h.size() * 4) && hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice) == hipSuccess; }
	T* get() const { return p; }
	operator T*() const { return p; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// A timed span of the engine's stream: two events.  An event record is a stream bubble of its own, so where two spans touch — hash bracket | K1f |
// hash bracket, K1f | apply — the end event of the first IS the start event of the second: the second span borrows it (owns0 == false) and the first
// destroys it.  Spans that touch are drained together (drain_events), so a borrowed event outlives every reader.
struct Span {
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	bool owns0 = true;
	uint64_t submits = 1; // what the span adds to ntc_kernel_time's launch count (a bracket of tiled launches: the submits it covers)
	Span() = default;
	Span(const Span&) = delete;
	Span& operator=(const Span&) = delete;
	Span(Span&& o) noexcept : ev0(o.ev0), ev1(o.ev1), owns0(o.owns0), submits(o.submits) { o.ev0 = o.ev1 = nullptr; }
	Span& operator=(Span&& o) noexcept
	{
		std::swap(ev0, o.ev0), std::swap(ev1, o.ev1), std::swap(owns0, o.owns0), std::swap(submits, o.submits);
		return *this;
	}
	~Span()
	{
		if (ev0 && owns0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
	}
};

enum Timer { T_HASH, T_APPLY, T_K1F, T_LONG_CUT, T_LONG_GATHER, T_HPC, T_SIG_INSERT, T_SIG_GROW, T_SIG_SORT, kTimers }; // ntc_engine::timers (T_K1F: outside the hash spans)

// One device-resident tiled batch: equal-length reads (d_tails == nullptr) or one length bin of a ragged read set (read_len = 16 C)
struct TiledSeg {
	const unsigned char* d_tiles;
	uint64_t n_reads;
	uint32_t read_len;
	const uint32_t* d_tails;
	// != 0: the reads are pieces of long sequences, cut with the overlap of this k — the largest of the list (ntc_submit.hip).  A smaller k owns the
	// windows that start in the piece's first read_len - (cut_k - 1) bytes: those of a read of len_for(k) bases in the same chunks
	uint32_t cut_k = 0;
	uint32_t len_for(uint32_t k) const { return cut_k ? read_len - (cut_k - k) : read_len; }
};

// K1 (sketch_hf_kernel) launch shape.  Every wave parks its 64 slots in LDS and the block shares
// the closed-form tables, so the waves a CU can hold are bounded by its 160 KiB of LDS; pick the block size
// (1..16 waves) that packs the most waves per CU (a fixed 4-wave block loses a third of them at k = 64).
struct HfPlan {
	unsigned grid = 0, wpb = 0, waves_per_cu = 0;
	size_t smem = 0;
};

} // namespace ntc_eng

struct ntc_engine {
	template <class T> using DevBuf = ntc_eng::DevBuf<T>;
	int device = 0;
	hipStream_t stream = nullptr;
	std::vector<uint32_t> klist;
	uint32_t r_bits = 27, s_bits = 7;
	std::vector<ntc::HfK> hfk;    // per-k argument blocks of K1 (tables derived once at create)
	uint32_t* d_sketch = nullptr; // [nk][2][1<<r_bits]: the caller's (ntc_config::ext_sketch / ext_f1) or own_sketch / own_f1's
	unsigned long long* d_f1 = nullptr;
	DevBuf<uint32_t> own_sketch;  // (empty when the caller owns the memory)
	DevBuf<unsigned long long> own_f1;
	DevBuf<uint32_t> d_phist;     // [nk][2][65536]
	DevBuf<uint16_t> d_out16;     // [2][1<<r_bits] scratch for finish
	int kernel_kind = 2;          // KIND_HF unless NTC_FLAG_SIMPLE_KERNEL
	// Hit log (ntc_apply.hip): K1 appends the counter index of every sampled k-mer instead of incrementing; the
	// log is applied to d_sketch when it fills up and whenever the sketch itself is needed (finish, merge, ...).
	DevBuf<uint32_t> d_log;         // [log_regions][log_region_cap]
	DevBuf<uint32_t> d_logfill;     // [log_regions]
	uint32_t log_regions = 0, log_region_cap = 0;
	uint32_t klog_regions = 0;      // K1f's own regions BEHIND the hash kernels' log_regions (the suspects it counts are log entries too); the apply reads all of them
	uint64_t log_cap = 0;           // entries (of the hash kernels' regions)
	// Does the sketch still hold the zeros of the last reset?  Then the first apply writes its counts instead of adding them (count_kernel).  The
	// host knows about applies, merges and pointers it has handed out (sk_host_dirty); kernels that increment the sketch themselves — K1 in direct mode, any
	// wave out of log regions, K1f's slow path, a partition run that overflowed — set the device word.
	DevBuf<uint32_t> d_skdirty;
	bool sk_host_dirty = true;
	bool sk_exposed = false;        // ntc_device_state has handed the counters' address out: the caller may add to them whenever it likes
	uint32_t all_log_regions() const { return log_regions + klog_regions; }
	double log_est = 0.0;           // host-side upper estimate of the entries logged since the last apply
	bool log_pending = false;
	// log or direct atomics: decided ON THE DEVICE from a sample of what the first sizeable batch after a reset logged
	// (repeated keys -> the counters stay cached -> direct atomics are cheaper; ntc_apply.hip, log_probe_kernel)
	DevBuf<uint32_t> d_logmode;             // 0 = log, 1 = direct atomics
	bool partition_always = false;          // NTC_FLAG_PARTITION_ALWAYS
	DevBuf<unsigned long long> d_logstats;  // {keys sampled, repeats among them}
	DevBuf<uint32_t> d_probe;               // 2^20-slot hash table of the probe
	bool adaptive = true, probed = false;
	struct ApplyPlan {
		uint32_t key_bits = 0, slice_bits = 0, b1 = 0, b2 = 0; // key = [b1 | b2 | slice_bits]
		uint32_t g1 = 0, parts2 = 0, cap1 = 0, cap2 = 0, n_slices = 0;
		// bytes per key in the runs of partition pass 1 / 2: the LAST pass writes uint16 (the run implies the slice; A3 reads the low slice_bits <= 15 bits)
		size_t key_bytes(int pass) const { return (pass == 2 || b2 == 0) ? 2 : 4; }
	} ap;
	DevBuf<uint32_t> d_s1, d_c1, d_s2, d_c2; // partition scratch: runs and run counts of the two passes
	std::vector<DevBuf<void>> d_t4s;          // K1f: closed-form table, 4 bases per entry, per k of the list (empty: that k is not K1h's)
	std::vector<DevBuf<uint32_t>> d_k1h_tabs; // K1h: closed-form table (3 bases per entry) per k of the list
	// What K1h hands to K1f (two bit arrays, the suspect list, a little state): one set per K1h launch whose K1f is still to come.  K1f's kernels
	// wait on memory (a few dependent loads per dirty piece / suspect, ~45 us per kernel whatever the batch), so for a caller that promised to leave
	// its batches alone until ntc_sync (NTC_FLAG_DEFER_REDO) the engine collects up to kK1fBatch K1h launches and sends ONE K1f over all of them;
	// without the promise K1f follows its K1h launch at once (set 0).
	struct K1hSet {
		DevBuf<uint32_t> d_dirty, d_tie;
		DevBuf<uint4> d_sus; // the suspect lists of a launch's waves (16 B per entry)
		DevBuf<uint32_t> d_sus_count, d_fix_state;
	} k1h_set[ntc::kK1fBatch];
	ntc::K1fBatch k1f_batch;        // the launches waiting for K1f (k1f_batch.item[i] uses k1h_set[i])
	uint32_t k1f_n = 0;
	// With NTC_FLAG_DEFER_REDO the HASH launches wait as well — up to eight device-resident tiled batches are hashed by ONE K1h launch per k, as
	// segments that share its workgroups (K1hMulti, built for the length bins of a ragged read set).  A K1h wave that starts inside a tile walks two masked
	// blocks first to fill its window: 8 % of a 10 M-read launch (24 blocks per wave), 1 % of an 80 M-read one; and a launch's ramp and tail are paid once.
	// The caller's promise is the same as for K1f: the batches stay unchanged until ntc_sync.  Everything that reads counters or F1, or ends the promise,
	// goes through join_k1f, which launches what waits here first.
	std::vector<ntc_eng::TiledSeg> deferred;
	bool in_flush = false;
	// ntc_merge_devices: exchange buffers, copy streams and events, kept between merges (grow-only).  ntc_destroy synchronises the lanes first.
	struct MergeCache {
		DevBuf<uint16_t> narrow, recv;
		std::vector<hipStream_t> lanes;
		std::vector<hipEvent_t> arrived;
		hipEvent_t narrowed = nullptr, summed = nullptr;
		MergeCache() = default;
		MergeCache(const MergeCache&) = delete;
		MergeCache& operator=(const MergeCache&) = delete;
		void sync_lanes() const
		{
			for (hipStream_t st : lanes)
				if (st) (void)hipStreamSynchronize(st);
		}
		~MergeCache()
		{
			for (hipStream_t st : lanes)
				if (st) (void)hipStreamDestroy(st);
			for (hipEvent_t ev : arrived)
				if (ev) (void)hipEventDestroy(ev);
			if (narrowed) (void)hipEventDestroy(narrowed);
			if (summed) (void)hipEventDestroy(summed);
		}
	} mc;
	uint64_t merge_allocs = 0; // device allocations + streams + events ntc_merge_devices has created for this engine
	uint32_t k1h_launch_id = 0;
	// profiling (HIP events on the engine stream).  Of the tiled path: ONE span brackets a RUN of hash launches (a pair of events per launch costs
	// 10 - 20 us of stream bubbles per launch, measured); the run ends when anything else is about to enter the stream (K1f, an apply, another kind of
	// batch, a sync).  `run` is that bracket while it is open (ev0 only).
	bool profiling = false;
	ntc_eng::Span run;
	struct {
		std::vector<ntc_eng::Span> spans; // closed, not yet read: drain_events adds them to ms and count (the submits they covered) and drops them
		double ms = 0.0;
		uint64_t count = 0;
	} timers[ntc_eng::kTimers];
	uint64_t applies = 0; // (counted whether or not the engine is profiling)
	bool ts_ok = false;             // the tiled kernel pair K1h + K1f is built for SOME k of this configuration (k_tiled says which) ...
	bool ts_all = false;            // ... for every k (then nothing of a tiled batch is left to K1)
	std::vector<uint8_t> k_tiled;   // per k of the list: K1h + K1f take it from tiled batches (the others are K1's, which stages the same tiles)
	bool ts_required = false;       // NTC_FLAG_REQUIRE_TILED
	bool seeded = false;            // ntc_create_seeded (a ragged tiled batch of a list no plane of which is K1h's goes to row slots, instead of being refused)
	bool defer_redo = false;        // NTC_FLAG_DEFER_REDO
	uint32_t strand = 0;            // 0 canonical; 1 NTC_FLAG_STRAND_FORWARD, 2 NTC_FLAG_STRAND_REVERSE: every batch is K1's one-strand form (no k is K1h's) unless NTC_FLAG_STRAND_TILED
	                                // was given and every plane is one of the one-strand K1h kernels' (then ts_all, and the tiled routes are those of a canonical engine)
	DevBuf<unsigned char> d_untile; // row-major scratch for tiled batches of configurations K1h is not built for
	// ntc_submit_long_device (ntc_submit.hip): the scratch of one round — the tiles its pieces are cut into, or its row slots and their slot table — grown like
	// d_untile; what ntc_long_stats and ntc_long_time report
	DevBuf<unsigned char> d_long;
	uint64_t long_pieces = 0, long_seqs = 0;
	// NTC_FLAG_HPC (ntc_submit.hip, ntc_hpc.hip): homopolymer-compressed counting.  ntc_submit_long_device compacts a round of whole sequences into d_hpc —
	// an owner of its own: d_long is recycled by the rounds of the cut that then READ d_hpc — with d_hpc_aux as the kernels' scratch (offsets, keep bits,
	// prefix table); hpc_mu serialises such calls (a round leaves e->mu between its compaction and its count); what ntc_hpc_stats / ntc_hpc_time report
	bool hpc = false;
	DevBuf<unsigned char> d_hpc, d_hpc_aux;
	std::mutex hpc_mu;
	uint64_t hpc_bytes_in = 0, hpc_bytes_out = 0;
	// NTC_FLAG_SIGNATURE (ntc_signature.hip): per plane an open-addressing table of the sampled 64-bit values and their counts, fed from a u64 value log
	// that K1's signature instantiations append to.  d_sigstate: per plane {log cursor, live keys, values in the log} (device uint64), then one scratch cursor for the compaction.
	// sig_booked: the WINDOWS of the launches since the last insert pass plus one chunk per wave of them, per plane — a hard bound of the log's cursor (a
	// read set may sample every window; a wave books the log in chunks of sig_chunk entries and leaves at most one of them partly unused).
	// live_ub: the live keys at the last read-back plus everything injected since (the insert pass reads the exact figure before it decides on growth)
	struct SigPlane {
		DevBuf<unsigned long long> keys;
		DevBuf<uint32_t> counts;
		uint64_t slots = 0, live_ub = 0;
	};
	bool sig = false;
	std::vector<SigPlane> sig_planes;
	DevBuf<unsigned long long> d_siglog, d_sigstate, d_sigtmp_k; // [planes][sig_log_cap]; the state words; compaction / inject scratch (keys)
	DevBuf<uint32_t> d_sigtmp_c;                                  // ... (counts)
	// ntc_signature / ntc_signature_device sort the compaction on the device (ntc_sig_sort.hip): the second pair buffer the radix passes alternate with, and the
	// sort's histograms; grow-only like the compaction's scratch, untouched while a plane fits the one-launch sort
	DevBuf<unsigned long long> d_sigalt_k;
	DevBuf<uint32_t> d_sigalt_c;
	DevBuf<unsigned char> d_sigsort;
	uint64_t sig_log_cap = 0, sig_log_limit = 0, sig_booked = 0, sig_init_slots = 0, sig_grows = 0;
	uint32_t sig_chunk = 64;
	DevBuf<uint32_t> d_tmeta;       // K1's slot table (len | len << 16 per read) of a RAGGED tiled batch under a list of which a part is K1's
	uint32_t hll_bits = 0;          // != 0: nthll engine (d_sketch holds uint32 M[1<<hll_bits])
	DevBuf<uint32_t> d_hll_thr;
	uint64_t hll_reads_seen = 0;
	// Spaced seeds, per plane of the list (ntc_create with a gap: its one plane's -g mask; ntc_create_seeded: the caller's masks).  A plane with an
	// empty mask counts plain k-mers; kgap != 0 marks ntcard's symmetric seed 1^a 0^g 1^a (ntcard.cpp:407-413), which K1h is built for at (12, 2), (32, 8).
	std::vector<std::string> masks;
	std::vector<uint32_t> kgap;
	std::vector<ntc::SeedPlan> seeds;  // K1's tables of each spaced plane (k == 0: plain)
	std::vector<DevBuf<void>> d_seedt; // SeedPlan::blob on device, per plane (empty: plain)
	uint32_t max_seed_lds = 0;         // the largest seed_lds of the list (pick_stride)
	bool plain(size_t ki) const { return masks[ki].empty(); }
	std::vector<DevBuf<void>> d_t1;    // per k: closed-form table of the H-filter kernel's resolve stage
	// ntc_submit staging: a small pool of pinned host + device buffer pairs (grow-only).  A caller packs its reads into a free
	// pair WITHOUT holding the engine lock (the reference's per-file parser threads pack in parallel), then enqueues
	// copy + kernels under the lock; `done` marks the point on the stream after which the pair may be reused.
	struct StageSlot {
		ntc_eng::PinBuf<unsigned char> h_stage;
		ntc_eng::PinBuf<uint32_t> h_meta;
		DevBuf<unsigned char> d_stage;
		DevBuf<uint32_t> d_meta;
		hipEvent_t done = nullptr;
		bool busy = false, used = false;
		~StageSlot()
		{
			if (done) (void)hipEventDestroy(done);
		}
	};
	static constexpr int kStageSlots = 4;
	StageSlot stage[kStageSlots];
	std::mutex stage_mu;
	std::condition_variable stage_cv;
	std::mutex mu;

	uint64_t plane_elems() const { return 2ull << r_bits; }
};

namespace ntc_eng {

// ---- ntc_plan.hip: geometry and policy, no HIP calls ----
uint32_t ceil_log2(uint64_t x);
size_t smem_simple(uint32_t stride);
void hf_shape(uint32_t stride, const uint32_t* ks, uint32_t n_k, uint32_t seed_lds, HfPlan& p, size_t& shared_out);
uint32_t pick_stride(uint64_t maxlen, const std::vector<uint32_t>& klist, uint32_t seed_lds);
unsigned hash_blocks_per_cu(size_t smem);
uint32_t seed_lds(const ntc::SeedPlan& sp);
uint32_t symmetric_gap(const std::string& m);
bool plan_log(ntc_engine* e, uint64_t want_entries);
bool k1_fits_tiles(const ntc_engine* e, uint32_t read_len);
double sampled_per_read(int64_t len, uint32_t k, uint32_t s_bits);
uint64_t probe_head_reads(double per_read);
uint32_t k1h_suspects_per_wave(uint32_t blocks_per_wave, uint32_t s_bits, uint32_t max_waves);
void fill_hfk(ntc::HfK& o, uint32_t k, uint32_t* sketch, unsigned long long* f1, const void* t1, uint32_t key_base = 0, uint32_t strand = 0);
void set_seed_args(ntc::HfArgs& a, const ntc::SeedPlan& sp, const void* d_blob);

// ---- ntc_launch.hip: what enters the engine's stream (the caller holds e->mu) ----
int device_cus(int dev, unsigned& cus);
int ensure_kernel_attrs(int dev);
int ensure_strand_kernel_attrs(int dev);
int hf_plan(int dev, uint64_t n_slots, uint32_t stride, const uint32_t* ks, uint32_t n_k, uint32_t seed_lds, HfPlan& p);
int hash_grid(int dev, uint64_t n_slots, uint32_t stride, unsigned& grid, size_t& smem);
int open_span(ntc_engine* e, Span& s, hipEvent_t borrow = nullptr);
int close_span(Span& s, hipStream_t st, std::vector<Span>& into, hipEvent_t* recorded = nullptr);
int close_run(ntc_engine* e, hipEvent_t* recorded = nullptr);
int drain_events(ntc_engine* e);
int join_k1f(ntc_engine* e, hipEvent_t* last = nullptr);
int apply_log(ntc_engine* e);
// the hash->sample->count kernel for every k of the list over one device-resident batch.  tiled: d_slots is a TILED batch (stride = 16 x its chunks: K1
// stages the tiles itself); skip: the k of the list that are NOT this call's (K1h has taken them)
int run_batch(ntc_engine* e, const unsigned char* d_slots, const uint32_t* d_meta, uint64_t n_slots, uint32_t read_len, uint32_t stride, bool tiled = false,
              const std::vector<uint8_t>* skip = nullptr);
// n_submits: the caller's submits these batches came in (ntc_kernel_time's launch count); k1f_now: the caller recycles the batches' memory behind this
// call, so their K1f may not wait (whatever NTC_FLAG_DEFER_REDO promised for the caller's own buffers)
int run_tiled_segs(ntc_engine* e, const TiledSeg* segs_in, uint32_t n_in, uint64_t n_submits = 1, bool k1f_now = false);
int defer_or_run_tiled(ntc_engine* e, const TiledSeg& sg);

// ---- ntc_signature.hip: NTC_FLAG_SIGNATURE (the caller holds e->mu) ----
int sig_setup(ntc_engine* e);                       // create: the knobs, the state words (the tables come with the reset)
int sig_reset(ntc_engine* e);                       // empty tables of the initial size; the stream is idle
uint64_t sig_max_slots(ntc_engine* e, uint64_t windows_per_slot); // the row slots one K1 launch may take (a multiple of 4; the log grows to at least four slots' need)
uint64_t sig_need(const ntc_engine* e, uint64_t n_slots, uint64_t windows_per_slot); // log entries a launch over n_slots may book: its windows + a chunk per wave
int sig_book(ntc_engine* e, uint64_t entries);      // room for a launch's sig_need in every plane's log: an insert pass first if it would not fit
void sig_args(const ntc_engine* e, ntc::HfArgs& a, size_t first, size_t n); // the log of planes first .. first + n into a K1 launch
int sig_flush(ntc_engine* e);                       // the pending log into the tables (waits for the stream)
int sig_merge_from(ntc_engine* root, ntc_engine* other); // other's signatures added to root's (both flushed; the caller holds both locks)

} // namespace ntc_eng
