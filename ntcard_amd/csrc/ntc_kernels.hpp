// ntc_kernels.hpp — argument blocks and launch helpers shared by ntc_kernels.hip and the engine's host layer (ntc_engine.hpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ntcard_hip.h"
#include "nthash_tables.hpp"

namespace ntc {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kTableBytes = kSlots * 32; // A (20 x 16 B) + B (20 x 16 B)

struct HashArgs {
	const unsigned char* slots; // [n_slots][stride] raw read bytes, slot i at i*stride
	const uint32_t* meta;       // optional [n_slots]: len | (window-start limit << 16); NULL: uniform
	uint64_t n_slots;
	uint32_t stride;            // bytes per slot, multiple of 4
	uint32_t read_len;          // uniform read length when meta == NULL
	uint32_t k;
	uint32_t r_bits, s_bits;
	uint32_t max_win;           // dump mode: capacity per read
	uint32_t* sketch;           // MODE 0: uint32 [2][1<<r_bits] plane pair of this k
	unsigned long long* f1;     // MODE 0: F1 of this k
	uint64_t* dump;             // MODE 1: [n_slots][max_win]
	uint32_t* dump_count;       // MODE 1: [n_slots]
	const void* t1;             // H-filter kernel: [ceil(k/2)][16] x {fwd.lo, fwd.hi, rev.lo, rev.hi} pre-rotated seed pairs (device)
	const void* gapt;           // H-filter kernel, spaced seed: [ceil(gap/2)][16] x {f.Hd, r.Hd, 0, 0} terms to XOR out
	uint32_t gap, gap_first;    // number of don't-care positions and index of the first one (ntcard.cpp:407-413)
	uint32_t hll_bits;          // != 0: nthll mode — `sketch` is uint32 M[1<<hll_bits] (max leading-zero runs, nthll.cpp:92-97)
	const uint32_t* hll_thr;    // nthll mode: device word, only hashes whose top 32 bits are < *hll_thr can raise a register
	uint32_t init[6];           // fast kernel: strand registers of the k x 'A' window {flo,fB,fHd,rlo,rB,rHd}
	uint32_t strand;            // 0: canonical min(fh, rh); 1: fh; 2: rh (NTC_FLAG_STRAND_*)
	HashTables tab;
};

// K1 (sketch_hf_kernel): one launch hashes a resident batch for up to kMaxFusedK values of k (the reference's
// ntRead loops over its k list per read, ntcard.cpp:147-158): the batch is staged and decoded once.
constexpr int kMaxFusedK = 4;
struct HfK {
	uint32_t k;
	uint32_t init_f, init_r;    // H halves ((H << 1) | H[30]) of the hash of k x 'A', forward / reverse
	uint32_t strand;            // 0: canonical; 1 forward / 2 reverse (the same for every k of a launch): the one-strand instantiations, which read the FIRST
	                            // half of every table entry — tabh[][0], init_f, HfArgs::tabg[][0], the first 8 (t1) / 4 (gapt) bytes — where the host has put the
	                            // wanted strand's words (nthash_tables.hpp: strand_t2, strand_seed_plan); the value only picks the rotate of the rolling update
	uint32_t* sketch;           // uint32 [2][1<<r_bits] plane pair of this k (nthll: uint32 M[1<<hll_bits])
	unsigned long long* f1;     // F1 of this k
	const void* t1;             // [ceil(k/2)][16] x {fwd.lo, fwd.hi, rev.lo, rev.hi} pre-rotated seed pairs (device)
	uint32_t key_base;          // index of this k's first counter in the engine's sketch array (hit-log keys are global indices)
	uint32_t pad2_;
	uint32_t tabh[kMainSlots][2]; // per (in,out) base pair: {Tf.Hd, Tr.Hd} step terms of the H halves
};
struct HfArgs {
	const unsigned char* slots; // as HashArgs
	const uint32_t* meta;
	uint64_t n_slots;
	uint32_t stride, read_len;
	uint32_t r_bits, s_bits;
	uint32_t n_k;               // 1..kMaxFusedK
	uint32_t gap;               // spaced seed (single k only): number of don't-care positions of the mask (SeedPlan::n_dc)
	uint32_t hll_bits;          // nthll mode: single k only
	uint32_t log_regions, log_region_cap; // hit log geometry (0 regions: ntComp's increment is a direct device atomic)
	uint32_t* log;              // [log_regions][log_region_cap] counter indices of sampled k-mers, relative to sketch0
	uint32_t* log_fill;         // [log_regions] entries used per region (persists across launches until the log is applied)
	uint32_t* sketch0;          // the engine's whole sketch array (overflow fallback of the log)
	const uint32_t* log_mode;   // device word: 0 = append to the log, 1 = direct atomics (set by the apply pass, see ntc_apply.hip)
	uint32_t* sk_dirty;         // the engine's "direct atomics happened" word (NULL: none), as K1hArgs::sk_dirty
	uint64_t* dump;             // validation build of K1 (kDump): [n_slots][dump_win] canonical hash of the window starting at each position
	uint32_t* dump_valid;       //   [n_slots][ceil(dump_win / 32)] bit set where a hash was written (window without a non-ACGTU byte)
	uint32_t dump_win;
	uint32_t tiled;             // the batch is in the TILED layout below (stride = 16 n_chunks is the LDS slot size): the wave's 64 reads are one lane group of a tile
	const void* gapt;           // spaced seed: SeedPlan::blob (XOR-out tables, further toggle tables, position words), staged in LDS
	const uint32_t* hll_thr;
	uint32_t tabg[kMainSlots][2]; // spaced seed, rolling form: toggle pair 0 (SeedPlan::tabg)
	HfK ks[kMaxFusedK];
	uint32_t seed_nroll;        // spaced seed: toggle pairs of the rolling form (0: every wave takes the closed-form XOR-out)
	uint32_t seed_extra;        // spaced seed: bytes of the blob behind its XOR-out tables (SeedPlan::extra_bytes)
	uint32_t roll_t[kMaxRollPairs]; // spaced seed: toggle pair p = t_a | t_b << 16 (bytes q - k + t of step q)
	// NTC_FLAG_SIGNATURE (ntc_signature.hip; the kSig instantiations only, behind everything the others read): per fused plane the u64 value log of the
	// sampled k-mers and its cursor (entries booked so far, all launches since the last insert round).  A wave books sig_chunk entries at a time (one
	// atomic), fills them round by round — a round may end one chunk and begin the next — and zeroes the rest of its last one.  sig_cap entries per log — the host books a launch's WINDOWS plus one chunk
	// per wave, so the cursor cannot pass it; a write behind it is dropped and shows as cursor > sig_cap at the next read-back
	unsigned long long* sig_log[kMaxFusedK];
	unsigned long long* sig_cursor[kMaxFusedK]; // [0] the cursor, [2] the VALUES logged (without the zeroed rests: what the table must make room for)
	uint64_t sig_cap;           // != 0 selects the signature instantiations (row slots; plain k lists and spaced seeds, canonical or one strand)
	uint32_t sig_chunk;         // >= 64 (a resolve round holds up to 64 values)
};

// TILED slot layout (ntc_submit_tiled_device): tile t = reads [2048 t, 2048 t + 2048); the 16 raw bytes of bases [16 c, 16 c + 16) of read r
// of tile t sit at ((t * n_chunks + c) * 2048 + r) * 16.
constexpr uint32_t kTileReads = 2048;
// K1h + K1f (ntc_sketch_k1h.hip; kernel body generated by gen_k1h.py): one wave per tile.  The generated code reads the first 88 bytes
// with scalar loads at the offsets of gen_k1h.KARG — keep the two in step (static_asserts in ntc_sketch_k1h.hip).
struct K1hArgs {
	const unsigned char* tiles;   // tiled slots
	uint32_t* log;                // hit log, [log_regions][log_region_cap] (log_regions == 0: direct atomics on sketch0)
	uint32_t* log_fill;
	uint32_t* sketch0;
	unsigned long long* f1;
	uint32_t* dirty;              // [n_tiles][n_chunks][64]: bit m of word (t, c, lane) = the 16-byte piece of read 64 m + lane holds a non-ACGTU byte
	uint32_t* tie;                // [n_tiles][blocks][64]: bit m = some window of that block of that read has both strands flagged
	uint32_t n_tiles, n_chunks;
	uint32_t read_len, nv_last;   // nv_last: reads in the last tile (1 .. 2048)
	uint32_t key_base, rmask2;    // rmask2 = (2 << r_bits) - 1: the counter index and the sample bit of a table word
	uint32_t log_regions, log_region_cap;
	const uint32_t* table;        // build_k1h_table
	uint32_t s_bits, r_bits;
	uint32_t blocks_per_wave;     // ceil(n_tiles * blocks / waves of the launch): wave w walks that many consecutive blocks from w * blocks_per_wave
	uint32_t nb_magic;            // floor(2^32 / blocks)
	uint4* sus;                   // suspect list: [waves][sus_cap] x {counter index, tile, read | window << 11, 0}: candidates K1h resolved but whose
	                              // window lies near a dirty piece — K1f counts them iff their bytes are all bases
	uint32_t* sus_count;          // [waves]: entries written (0xffffffff: the wave ran out of room — K1f then walks every dirty-affected block itself)
	uint32_t sus_cap, launch_id;
	uint32_t* fix_state;          // K1f scratch: [0] = launch_id of the last launch that must take the slow path, [2..3] = F1 correction (uint64)
	const uint32_t* tails;        // ragged batch (NULL: every read is read_len long): [n_tiles][16], tails[t][d] = reads of tile t with more than d bases in
	                              // their last 16-base piece; read_len = 16 n_chunks, every tile sorted longest read first (ntc_submit_tiled_ragged_device)
	uint32_t first_wg, n_wg;      // the workgroups of the launch that walk THIS batch (K1hMulti: several batches share one launch)
	uint32_t* sk_dirty;           // the engine's "direct atomics happened" word (NULL: none): set to 1 by every wave that increments the sketch itself instead of logging (round 6)
};
// One K1h launch over up to kK1hSegs batches of different geometry (the length bins of a ragged read set: round 5).  Every batch ("segment") has its own
// arguments — tiles, read length, bit arrays, suspect list — and a contiguous range of the launch's workgroups, in proportion to its blocks; the waves of a
// workgroup share out their segment's blocks exactly as in a launch of their own.  Why: a wave that starts inside a tile first walks two masked blocks to
// fill its window, which is 8 % of a 10 M-read launch and 40 % of four 2.5 M-read launches one after the other (profiles/r05_batch_size_sweep.txt).
constexpr uint32_t kK1hSegs = 8;
struct K1hMulti {
	K1hArgs seg[kK1hSegs];
	uint32_t n_segs;
};
// strand: 0 the canonical kernels; 1 forward / 2 reverse: the one-strand kernels (gen_k1h.STRAND_VARIANTS: the same k, gaps and sBits classes)
bool sketch_k1h_supports(uint32_t k, uint32_t gap, uint32_t s_bits, uint32_t r_bits, uint32_t strand = 0);
uint32_t sketch_k1h_blocks(uint32_t k, uint32_t read_len);
uint32_t sketch_k1h_waves();
uint32_t sketch_k1h_min_blocks(); // blocks per wave below which launch_sketch_k1h uses fewer workgroups
void build_k1h_table(uint32_t k, uint32_t gap, uint32_t r_bits, uint32_t s_bits, uint32_t* out /* 2 * ceil(k / 3) * 64 dwords */);
hipError_t set_sketch_k1h_smem_limit();        // the canonical kernels
hipError_t set_sketch_k1h_strand_smem_limit(); // the one-strand kernels (before the first launch of one on a device)
hipError_t launch_sketch_k1h(const K1hArgs& a, uint32_t k, uint32_t gap, unsigned cus, hipStream_t st, K1hArgs* args_out, uint32_t* n_waves, uint32_t strand = 0);
// the workgroups and block shares launch_sketch_k1h_multi gives n batches (read_len / n_tiles of a[i] set): fills first_wg, n_wg, blocks_per_wave, nb_magic of
// out[i]; -> the grid.  The engine sizes the suspect lists from it before the launch.
unsigned plan_sketch_k1h(const K1hArgs* a, uint32_t n, uint32_t k, unsigned cus, K1hArgs* out);
// ONE launch over n <= kK1hSegs batches (same k, gap, sBits, table); args_out[i] = the arguments of batch i as launched; *n_waves = the waves of the
// whole launch.  Every batch's suspect list is indexed by the wave's number in the LAUNCH: batch i's suspects sit in the regions first_wg * 8 .. of ITS list,
// the other regions of that list are not written (K1f visits n_wg * 8 regions from first_wg * 8: K1fItem::n_waves)
hipError_t launch_sketch_k1h_multi(const K1hArgs* a, uint32_t n, uint32_t k, uint32_t gap, unsigned cus, hipStream_t st, K1hArgs* args_out, uint32_t* n_waves,
                                   uint32_t strand = 0);
// K1f takes up to kK1fBatch K1h launches at a time (blockIdx.y = the launch): its kernels wait on memory, not on issue slots, so the launches of
// several batches cost little more than those of one (an engine whose caller keeps the batches unchanged until ntc_sync defers them)
constexpr uint32_t kK1fBatch = 8;
struct K1fItem {
	K1hArgs a;                    // as launched (launch_sketch_k1h's args_out)
	const void* t4;               // build_t4 of this k, with the engine's gap
	uint32_t k, n_waves;          // n_waves: the K1h waves that walked this batch (a.n_wg x 8) = its suspect regions, from region a.first_wg x 8
	// round 6: the suspects K1f counts go to the hit log like every other sampled k-mer (regions of their own behind the hash kernels', shared by all K1f
	// blocks through one cursor atomic per wave) instead of to the sketch as scattered device atomics; klog_n == 0: no log, atomics
	uint32_t* klog;               // [klog_n][klog_cap]
	uint32_t* klog_fill;          // [klog_n]
	uint32_t klog_n, klog_cap;
	uint32_t strand;              // 0: a canonical K1h launch; 1 forward / 2 reverse: a one-strand launch — the slow path takes fh / rh, the tie rows are not visited
};
struct K1fBatch {
	K1fItem item[kK1fBatch];
};
hipError_t launch_k1h_fixup(const K1fBatch& b, uint32_t n_items, unsigned cus, hipStream_t st);
// tiled layout -> row-major slots: device-side re-layout for the configurations the tiled kernels are not built for
hipError_t launch_gen_tiled(unsigned char* out, uint64_t seed, uint64_t first, uint64_t n, uint32_t len, uint32_t dist, uint64_t glen, hipStream_t st);
hipError_t launch_untile(const unsigned char* tiles, unsigned char* slots, uint64_t n_reads, uint32_t read_len, uint32_t stride, hipStream_t st);
// a ragged tiled batch for K1 (round 6): meta[i] = len | len << 16 of read i from tails[tile][16] (the reads of a tile are sorted longest first)
hipError_t launch_tails_to_meta(const uint32_t* tails, uint64_t n_reads, uint32_t n_chunks, uint32_t* meta, hipStream_t st);
// ---- long sequences (ntc_long.hip; ntc_submit_long_device) ----
// pieces -> tiles: the call's sequences that hold a full piece are seqs[0 .. n_seqs), in piece order, and seqs[n_seqs] = {0, the call's pieces} closes the
// table; piece p of the call = the piece_len (= 16 x chunks) source bytes from src + seqs[s].src + (p - seqs[s].first) * step, of any alignment, for the s
// with seqs[s].first <= p < seqs[s + 1].first.  Pieces first_piece .. first_piece + n_pieces become "reads" 0 .. n_pieces of an equal-length tiled batch
// (ntc_tiled_bytes(n_pieces, piece_len) bytes at `tiles`; the slots behind the last piece stay unwritten)
struct LongSeq {
	uint64_t src, first;
};
hipError_t launch_cut_tiles(const unsigned char* src, const LongSeq* seqs, uint32_t n_seqs, uint64_t first_piece, uint64_t n_pieces, uint32_t step,
                            uint32_t piece_len, unsigned char* tiles, hipStream_t st);
// spans -> row slots: slot i = `bytes` source bytes from src + spans[i].src, then 'A' up to the stride (a multiple of 4; slots 4-byte aligned);
// meta[i] = bytes | limit << 16 (HashArgs::meta)
struct LongSpan {
	uint64_t src;
	uint32_t bytes, limit;
};
hipError_t launch_gather_slots(const unsigned char* src, const LongSpan* spans, uint64_t n_slots, uint32_t stride, unsigned char* slots, uint32_t* meta, hipStream_t st);
// ---- homopolymer compression (ntc_hpc.hip; NTC_FLAG_HPC, ntc_hpc_compress_device) ----
// One compaction: the n_seqs sequences [h_off[i], h_off[i + 1]) of src (host offsets, non-decreasing; source bytes of any alignment) lose every byte that
// repeats the base class of the byte in front of it inside its sequence; the kept bytes go to out (any alignment; room for h_off[n_seqs] - h_off[0] bytes)
// behind one another, and the new offsets — from 0 — to hpc_aux_offsets(aux, n_seqs): n_seqs + 1 device uint64.  aux: hpc_aux_bytes() bytes of device
// scratch, 8-byte aligned.  Everything is queued on st, the copy of h_off included: the caller waits for the stream before h_off goes away.
size_t hpc_aux_bytes(uint64_t n_bytes, uint64_t n_seqs);
const uint64_t* hpc_aux_offsets(const void* aux, uint64_t n_seqs);
hipError_t launch_hpc_compact(const unsigned char* src, const uint64_t* h_off, uint64_t n_seqs, unsigned char* out, void* aux, hipStream_t st);

// ---- deferred sketch update (ntc_apply.hip) ----
// A1/A2: radix partition of key runs.  Input run `seg` = in[seg * in_cap, +min(in_cnt[seg], in_cap)).
//   mode 0: workgroup w reads runs w, w + grid, ...                      (first pass over the raw log regions)
//   mode 1: workgroup w = b * parts + p reads runs (p + t * parts) * nb_in + b, t = 0, 1, ...   (bucket b of pass 1)
// Output run (w, digit) = out[(w * 2^bits + digit) * out_cap, +out_cnt[w * 2^bits + digit]).
struct SplitArgs {
	const uint32_t* in;
	const uint32_t* in_cnt;
	uint32_t in_cap, n_in;
	uint32_t mode, parts, nb_in;
	uint32_t shift, bits;
	uint32_t out_cap;
	uint32_t* out;    // narrow != 0: uint16_t runs (the LAST pass before A3: the slice index is implied by the run, the low 16 bits are all A3 reads)
	uint32_t* out_cnt;
	uint32_t* sketch; // uint32 [2][1 << r_bits] of this k: overflow fallback
	uint32_t narrow;
	uint32_t* sk_dirty; // set to 1 when the overflow fallback increments the sketch directly
	// round 6: packed runs between two passes (ntc_apply.hip): pack_out — the runs are written three keys to a 64-bit word (out_cap counts words; only when
	// the keys' bits below the digit number <= 21); pack_in — the input runs are such words (in_cap, in_cnt count words), hi_shift: where the digit of the
	// pass that wrote them goes back into the key
	uint32_t pack_out, pack_in, hi_shift;
};
// A3: slice s = keys [s << slice_bits, (s + 1) << slice_bits).  mode 0: raw regions (one slice), 1: after one
// split pass (runs (w1, s), w1 < nwg1), 2: after two (runs ((b, p), d2), s = b * nb2 + d2, p < parts).
struct CountArgs {
	const uint32_t* in;
	const uint32_t* in_cnt;
	uint32_t in_cap, n_in;
	uint32_t mode, nb1, nwg1, parts, nb2;
	uint32_t slice_bits, n_slices;
	uint32_t* sketch;
	uint32_t in16; // the runs hold uint16_t keys (SplitArgs::narrow)
	// round 6: the FIRST apply behind a reset finds a sketch of zeros unless some kernel incremented it directly (*sk_dirty != 0): it then WRITES its counts
	// instead of adding them — the sweep reads nothing (1 GiB less per apply at rBits = 27)
	uint32_t first;
	const uint32_t* sk_dirty;
	// round 6: the log's fill words, cleared by this kernel when the partition passes in front of it were their readers (mode != 0): one memset launch and
	// its stream bubble less per apply
	uint32_t* clear_fill;
	uint32_t n_clear;
};
hipError_t launch_log_atomics(const uint32_t* log, uint32_t* fill, uint32_t region_cap, uint32_t n_regions, uint32_t* total16, uint32_t* sketch, uint32_t* sk_dirty,
                              hipStream_t st);
// sample of the first batch's log -> *mode (0 keep logging, 1 direct atomics: the sampled keys repeat); ntc_apply.hip
hipError_t launch_log_probe(const uint32_t* log, const uint32_t* fill, uint32_t region_cap, uint32_t n_regions, uint32_t per_region, uint32_t* table,
                            uint32_t table_slots, unsigned long long* stats, uint32_t* mode, hipStream_t st);
// the pending log split by counter-range owner (ntc_log_export_device): cursor[p] += keys of owner p = key / keys_per_part; out != NULL: written to out[part_off[p] + ...]
hipError_t launch_log_export(const uint32_t* log, const uint32_t* fill, uint32_t region_cap, uint32_t n_regions, uint32_t n_parts, uint32_t keys_per_part,
                             uint32_t* out, const unsigned long long* part_off, unsigned long long* cursor, hipStream_t st);
// fill[r] = the part of n keys that falls into region r of a log loaded contiguously (ntc_log_replace_device)
hipError_t launch_log_set_fill(uint32_t* fill, uint32_t n_regions, uint32_t region_cap, unsigned long long n_keys, hipStream_t st);
hipError_t launch_split(const SplitArgs& a, unsigned grid, hipStream_t st);
hipError_t launch_count(const CountArgs& a, unsigned grid, hipStream_t st);
hipError_t set_apply_smem_limit();

// ---- signatures (ntc_signature.hip; NTC_FLAG_SIGNATURE) ----
// One plane's container: an open-addressing table, keys[slots] (0 = empty) + counts[slots], slots a power of two, linear probing from a multiplicative
// home slot; *live = the keys it holds.  The HOST keeps it at most half full (ntc_signature.hip: sig_room), so a probe always ends.
struct SigTable {
	unsigned long long* keys;
	uint32_t* counts;
	uint64_t slots;
	unsigned long long* live;
};
// adds n pairs (in_keys[i], in_counts ? in_counts[i] : 1), zeros skipped, duplicates summed, counts saturating at 2^32 - 1 (in_counts == nullptr: n < 2^31)
hipError_t launch_sig_insert(const SigTable& t, const unsigned long long* in_keys, const uint32_t* in_counts, uint64_t n, hipStream_t st);
// the live pairs of a table, in slot order of arrival, to out_keys / out_counts (room for *live entries); *cursor (zeroed by the caller) counts them
hipError_t launch_sig_compact(const SigTable& t, unsigned long long* out_keys, uint32_t* out_counts, unsigned long long* cursor, hipStream_t st);
// ---- sort of (u64 key, u32 value) pairs (ntc_sig_sort.hip) ----
// A stable LSD radix sort, ascending by key, n < 2^32; vals (and alt_vals) may be nullptr.  n <= sig_sort_one_launch(): one launch, in place, alt_* and aux
// unused.  Otherwise the passes alternate between (keys, vals) and (alt_keys, alt_vals) — room for n each — with sig_sort_aux_bytes(n) bytes of aux, and
// *in_alt says where the sorted pairs lie; the call waits for the stream once (it reads the digit histograms to skip the digits that do not tell any keys
// apart) and returns with the passes enqueued
uint64_t sig_sort_one_launch();
size_t sig_sort_aux_bytes(uint64_t n);
hipError_t sig_sort(unsigned long long* keys, uint32_t* vals, unsigned long long* alt_keys, uint32_t* alt_vals, uint64_t n, void* aux, hipStream_t st, bool* in_alt);

hipError_t launch_hash(int mode, const HashArgs& a, unsigned grid, size_t smem, hipStream_t st);
hipError_t set_hash_smem_limit(size_t smem);
hipError_t launch_sketch_hf(const HfArgs& a, unsigned grid, unsigned waves_per_block, size_t smem, hipStream_t st);
hipError_t launch_compact_dump(const uint64_t* full, const uint32_t* valid, uint64_t n_reads, uint32_t n_win, uint32_t max_win, uint64_t* out, uint32_t* count, hipStream_t st);
hipError_t set_sketch_hf_smem_limit(size_t smem);
// what launch_sketch_hf has dispatched for row `row` of K1's variant table (ntc_k1_variant_stats); false: the table has no such row
constexpr int kK1Regimes = 8;
static_assert(sizeof(ntc_k1_variant_info::regime) == kK1Regimes * sizeof(uint64_t), "ntc_k1_variant_info::regime");
bool k1_variant_stats(uint32_t row, ntc_k1_variant_info& out);
bool sketch_hf_deep_prefetch(uint32_t stride);
hipError_t launch_hll_threshold(const uint32_t* regs, uint32_t n_regs, uint32_t* thr, hipStream_t st);
hipError_t launch_finalize(const uint32_t* sketch, uint64_t n_per_sample, uint32_t* p_hist,
                           uint16_t* out16, hipStream_t st);
hipError_t launch_value_hist(const uint32_t* counters, uint64_t n, uint32_t* p_hist, hipStream_t st);
// dst[i] = dst[i] + src[i] (or max for nthll registers): the full-width part of ntc_merge_devices (F1, nthll register files)
hipError_t launch_fold_u32(uint32_t* dst, const uint32_t* src, uint64_t n, bool take_max, hipStream_t st);
hipError_t launch_fold_u64(unsigned long long* dst, const unsigned long long* src, uint64_t n, hipStream_t st);
hipError_t launch_add_counters(uint32_t* sketch, const uint16_t* add16, uint64_t n, hipStream_t st);
hipError_t launch_narrow_u16(const uint32_t* src, uint16_t* dst, uint64_t n, hipStream_t st);
hipError_t launch_value_hist_u16(const uint16_t* counters, uint64_t n, uint32_t* p_hist, hipStream_t st);
hipError_t launch_sum_slices_u16(uint16_t* slices, uint64_t stride, uint32_t n_slices, uint64_t len, hipStream_t st);
hipError_t launch_widen_u16(const uint16_t* src, uint32_t* dst, uint64_t n, hipStream_t st);
hipError_t launch_gen(unsigned char* out, uint64_t seed, uint64_t first, uint64_t n, uint32_t len,
                      uint32_t stride, uint32_t dist, uint64_t glen, hipStream_t st);

} // namespace ntc
