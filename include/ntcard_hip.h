/*
 * ntcard_hip.h — C ABI of the MI355X (gfx950) ntHash -> sample -> count engine.
 *
 * Drop-in boundary (seam B2).  The reference has no FFI; the seam this library
 * replaces is the in-process call the record parsers make for every sequence,
 *     ntRead / stRead(const std::string& seq, const std::vector<unsigned>& kList,
 *                     uint16_t* t_Counter, size_t totKmer[])      ntcard.cpp:147-171
 * (call sites ntcard.cpp:182,185,203,205,230,232), together with the state that call mutates,
 *     uint16_t t_Counter[nK][nSamp=2][1<<rBits]                  ntcard.cpp:437-439
 *     size_t   totalKmers[nK]  (F1)                              ntcard.cpp:433-435,464-466
 * its configuration globals opt::{rBits,sBits,sMask,rBuck,nSamp,gap,seedSet} (ntcard.cpp:52-67),
 * and the consumer of that state, compEst (ntcard.cpp:237-275) + outDefault/outCompact
 * (ntcard.cpp:277-315).  INTEGRATION.md shows the patch a reference maintainer would apply.
 *
 * Conventions: plain C, plain pointers and sizes, no torch/HIP types in signatures (a HIP stream is
 * passed as void*).  Every function returns 0 on success and a negative ntc_status on failure;
 * ntc_last_error() returns a thread-local message.  There is NO CPU fallback: if no gfx950 device
 * or kernel image is available, ntc_create fails with NTC_ERR_DEVICE.
 */
#ifndef NTCARD_HIP_H
#define NTCARD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTC_ABI_VERSION 6
#define NTC_MAX_K_LIST 32

typedef enum {
    NTC_OK = 0,
    NTC_ERR_ARG = -1,      /* bad argument / unsupported configuration              */
    NTC_ERR_DEVICE = -2,   /* no usable HIP device, or a HIP runtime call failed    */
    NTC_ERR_MEMORY = -3,   /* host or device allocation failed                      */
    NTC_ERR_STATE = -4     /* call not valid in the engine's current state          */
} ntc_status;

typedef struct ntc_engine ntc_engine; /* opaque: owns the device sketch, F1 and staging buffers */

/* Replaces opt::{kList(-k), gap(-g), rBits(-r), sBits(-s)} (ntcard.cpp:52-67,325-363).  The CALLER
 * applies the "total input < 50 GB => sBits = 7" rule (ntcard.cpp:427-431) before ntc_create.   */
typedef struct {
    uint32_t n_k;              /* number of k values (order defines sketch plane order)          */
    const uint32_t *k;         /* k list; every k >= 1 and <= NTC_MAX_K (see ntc_max_k())        */
    uint32_t gap;              /* 0, or g: seed = 1^((k-g)/2) 0^g 1^((k-g)/2); needs n_k == 1    */
    uint32_t r_bits;           /* log2 buckets per sample (reference default 27); 8..30          */
    uint32_t s_bits;           /* sampling bits (reference: 7 or 11); 2..24                      */
    int32_t device;            /* HIP device ordinal                                             */
    void *stream;              /* hipStream_t to run on, or NULL for the device's null stream    */
    void *ext_sketch;          /* optional caller-owned DEVICE memory for the sketch:
                                  uint32_t [n_k][2][1<<r_bits]; NULL -> engine allocates.
                                  (lets a host framework own/merge the buffer, e.g. RCCL reduce)
                                  Its CONTENTS are the engine's from ntc_create / ntc_reset (which zero
                                  it) on: the caller may read it behind ntc_flush / ntc_finish, and may
                                  WRITE to it (an in-place reduce, a merge) only after a call of
                                  ntc_device_state — which is what tells the engine that the counters
                                  can change behind its back (the first sketch update after a reset
                                  otherwise writes its counts into the zeroed buffer without reading) */
    void *ext_f1;              /* optional caller-owned DEVICE uint64_t [n_k]; NULL -> engine    */
    uint32_t flags;            /* NTC_FLAG_*                                                      */
    uint64_t log_entries;      /* capacity of the hit log in 4-byte entries, 0 = default (four per
                                  counter, at most 2^30: 4 GiB at rBits = 27 and one k).  ntComp's `++t_Counter[...]` (ntcard.cpp:142-143) is
                                  deferred: the kernels log the counter index of every sampled k-mer
                                  and the log is applied to the sketch when it fills up and whenever
                                  the counters are needed (ntc_finish, ntc_flush, ...)              */
} ntc_config;

#define NTC_FLAG_NONE 0u
#define NTC_FLAG_SIMPLE_KERNEL 1u  /* run the simple validation kernel instead of the production ones */
#define NTC_FLAG_LANE_KERNEL 32u    /* the lane-per-read kernel K1 takes every batch, tiled ones too (re-laid out as row slots): cross-check, A/B runs.
                                      (Flag value 4, round 2-4's NTC_FLAG_BITSLICE_KERNEL, is unused since ABI 5: the bit-sliced row-slot kernel K1b is gone.) */
#define NTC_FLAG_ALWAYS_LOG 8u      /* keep logging whatever the data looks like (by default the engine switches to direct
                                      atomics when an apply finds few distinct counters per increment: repeats)       */
#define NTC_FLAG_PARTITION_ALWAYS 16u /* validation: apply even a small hit log through the partition + histogram passes
                                         (by default fewer than 4 M pending entries are applied with plain atomics)   */
#define NTC_FLAG_DEFER_REDO 128u    /* device-resident batches (ntc_submit_device, ntc_submit_tiled_device): the caller promises to keep every
                                      submitted buffer valid AND UNCHANGED until ntc_sync / ntc_finish returns.  The second passes over a batch's
                                      reads with non-ACGTU bytes are then shared by several batches instead of run per batch: the fix-up
                                      kernels K1f behind up to 8 launches of the one-wave-per-tile kernel K1h.  Since ABI 6 the HASH launches wait as
                                      well: up to 8 tiled batches (ntc_submit_tiled_device / _ragged_device) are hashed by one launch per k, started
                                      when the eighth arrives or when ntc_flush / ntc_sync / ntc_finish / ntc_reset / ntc_merge_devices / ntc_device_state /
                                      the log calls need the counters — work submitted under this flag is only guaranteed to have been ENQUEUED after one of
                                      those calls (a small batch then costs its share of a large launch instead of a launch of its own).  ntc_merge_counters
                                      does NOT start them: it adds its image into the counters, the waiting batches are added behind it in stream order, and
                                      the sums commute (tests/test_engine_seq_gpu.py pins the launch count across it and the result after it).  Without the flag a
                                      buffer may be reused as soon as the stream has passed the submit call. */
#define NTC_FLAG_REQUIRE_TILED 64u  /* validation: a tiled batch must be served by the tiled kernels for EVERY k of the list, else ntc_submit_tiled_device fails */
/* ONE STRAND instead of the canonical k-mer (additive to ABI 6: two flag bits and ntc_hash_dump_strand_device; ntc_config and NTC_ABI_VERSION are unchanged).
 * An engine has a strand: canonical (no flag, what ntcard counts), forward, or reverse.
 *   - Which windows count is unchanged: a window of k bytes counts (F1, sketch) only when all k bytes are bases, those under a mask's '0' included,
 *     so F1 of a read set is the same for all three strands.
 *   - The value that goes into ntComp (ntcard.cpp:132-145) is
 *       canonical:  rh < fh ? rh : fh                                    (nthash.hpp:275-279)
 *       forward:    fh = XOR_i srol^(k-1-i)(seedTab[b_i])                (nthash.hpp:220-228, what NTF64 rolls)
 *       reverse:    rh = XOR_i srol^i(seedTab[b_i & cpOff])              (nthash.hpp:231-239, NTR64): the forward value of the window's reverse complement.
 *     For a plane that is a spaced seed (ntc_create_seeded, ntc_create with gap) fs / rs as defined there — the don't-care terms XORed out of fh / rh —
 *     take the place of fh / rh.
 *   - Everything behind the value is unchanged: sampling, bucket, hit log, sketch update, estimator, output.
 * Valid with ntc_create (k lists, gap) and ntc_create_seeded; both flags together are NTC_ERR_ARG (checked before a device is looked for).  WITHOUT
 * NTC_FLAG_STRAND_TILED a strand engine is the general kernel's (K1, in its one-strand form: one rolling update and one table half per base instead of two)
 * and the simple validation kernel's: no k of it is the tiled pair's — tiled batches, ragged ones and bins included, are re-laid out on the device and
 * counted by K1, NTC_FLAG_REQUIRE_TILED makes the tiled submit fail with nothing counted, host batches take row slots.  It then counts at K1's rate, not at
 * K1h's (DESIGN.md §4 "One strand").  ntc_merge_devices refuses engines whose strands differ.  nthll engines take the same two flags through
 * ntc_hll_create_ex (ntc_hll_create: canonical). */
#define NTC_FLAG_STRAND_FORWARD 512u
#define NTC_FLAG_STRAND_REVERSE 1024u
/* A ONE-STRAND engine on the TILED kernels (additive to ABI 6: one flag bit).  Valid only beside exactly one of NTC_FLAG_STRAND_FORWARD / _REVERSE: alone,
 * or beside both, it is NTC_ERR_ARG, checked before a device is looked for; ntc_hll_create_ex refuses it.  The library holds a one-strand form of K1h for
 * every (k, gap) of the canonical one — it walks, tests and queues that strand alone; K1f re-derives with fh or rh where it re-derives at all and has no
 * ties to settle.  A strand engine's plane is the tiled kernels' when it is plain k = 12 .. 32 or one of the two tiled -g seeds, with sBits >= 7.
 *   - EVERY plane of the engine is one of those: every tiled route works as for a canonical engine — ntc_submit_tiled_device, _ragged_device,
 *     _bins_device, the tile packing of host batches, NTC_FLAG_DEFER_REDO's shared launches and deferred K1f — NTC_FLAG_REQUIRE_TILED is satisfied on
 *     them, and the engine qualifies for the long-sequence cut under the rules given at ntc_submit_long_device.
 *   - Only PART of the list qualifies (k = 32,64): the flag changes nothing, for any k of the list — re-layout, then K1, and NTC_FLAG_REQUIRE_TILED
 *     refuses tiled batches as above.  (K1 has no one-strand form that stages tiles, so a strand list cannot be split between the kernels the way a
 *     canonical one is.)
 * Without the flag a strand engine behaves bit for bit as before it existed; results are identical either way, and ntc_merge_devices does not compare the
 * flag (strand, k list, masks, rBits and sBits still have to match).  Rates: DESIGN.md §4 "One strand", profiles/strand_k1h.txt.
 * (Bit 2048 stays refused as an unknown flag.) */
#define NTC_FLAG_STRAND_TILED 4096u
/* HOMOPOLYMER-COMPRESSED counting (additive to ABI 6: one flag bit, ntc_hpc_compress, ntc_hpc_compress_device, ntc_hpc_stats, ntc_hpc_time; ntc_config and
 * NTC_ABI_VERSION are unchanged).  Every run of one base is collapsed to its first byte before the windows are taken — the space HiFi / ONT assemblers and
 * their QC count k-mers in, since long-read errors are mostly errors of a run's length.  class(b): A a -> 0, C c -> 1, G g -> 2, T t U u -> 3; every other
 * byte has none (N, IUPAC letters, CR, the control bytes 1, 3, 4, 5, 7 the seed table takes for bases).  Within ONE sequence byte j is DROPPED iff j > 0 and
 * class(b[j]) exists and equals class(b[j - 1]); kept bytes keep value and order (of `aAAa` the leading `a` survives).  So bytes without a class are never
 * dropped (`NNN` stays three bytes), a run never continues across a sequence boundary, an empty sequence stays empty.  The compressed sequence is what
 * ntRead (ntcard.cpp:147-158) then sees: which windows count, strands, masks, k lists, sampling, F1, the estimator and the outputs are unchanged.
 *   - Valid in ntc_create and ntc_create_seeded beside every other flag, and in ntc_hll_config.flags alone or beside one strand flag.
 *   - ntc_submit / ntc_submit_spans compress every read on the host (ntc_hpc_compress) into a temporary batch and go on as without the flag.
 *   - ntc_submit_long_device compacts ON THE DEVICE into scratch of the engine's own, in rounds of whole sequences of at most NTC_HPC_ROUND_BYTES source
 *     bytes (environment, read per call; default 1 GiB; a longer sequence is a round of its own, the scratch grows to it), and hands the scratch and the new
 *     offsets to the path the call takes without the flag: piece_len, the cut, ntc_long_stats and NTC_FLAG_REQUIRE_TILED speak of the COMPRESSED sequences.
 *     Every round WAITS for the stream once: the new offsets (8 B per sequence) come back to the host, whose planner cuts the sequences.  The source
 *     may be reused as soon as the stream has passed the call, under NTC_FLAG_DEFER_REDO too.
 *   - The fixed-layout device batches (ntc_submit_device, ntc_submit_tiled_device, _ragged_device, _bins_device) fix a read's length: on an engine with
 *     the flag they fail with NTC_ERR_ARG and count nothing.
 *   - ntc_merge_devices refuses engines that differ in the flag.  ntc_merge_counters CANNOT know how a dumped image was counted: merging an image
 *     counted without the flag into an engine with it (or the other way round) is the caller's mistake to avoid.  The dump and generator tools ignore it.
 * (Bits 4, 256, 2048 and 1 << 20 stay refused as unknown flags.) */
#define NTC_FLAG_HPC 8192u
/* SIGNATURES (additive to ABI 6: one flag bit, the ntc_signature* calls — the device sort, compare and matrix among them — and ntc_sig_header; ntc_config and NTC_ABI_VERSION are unchanged).  The engine keeps,
 * per plane (a k of the list, or a mask), every value h it hands to ntComp (ntcard.cpp:132-145) that ntComp SAMPLES —
 *     sample 0: (h >> (63 - s)) == 1          sample 1: (h >> (64 - s)) == (1 << (s - 1)) - 1           s = s_bits
 * — with its exact multiplicity: a FracMinHash signature of the read set at rate ~ 2 * 2^-s.  h is whatever the engine counts: the canonical, forward or reverse
 * value, plain or under a mask, of a homopolymer-compressed sequence or not.  Two read sets counted with the same planes, strand, hpc and s_bits sample the same
 * k-mers, so the intersection of their signatures estimates Jaccard similarity and containment (ntc_signature_compare), and the multiplicities are a
 * collision-free cross-check of the estimator.  Everything else is unchanged: t_Counter, F1 and the outputs of a signature engine are bit-identical to those of
 * the same engine without the flag.  A signature plane is a list of pairs (uint64 hash, uint32 count), strictly ascending by hash, counts saturating at
 * 2^32 - 1; h == 0 cannot be sampled (both patterns hold a 1 bit) and marks an empty slot.
 *   - Valid in ntc_create and ntc_create_seeded beside the strand flags, NTC_FLAG_HPC, NTC_FLAG_DIRECT_ATOMICS, _ALWAYS_LOG, _PARTITION_ALWAYS, _LANE_KERNEL
 *     and _DEFER_REDO; beside NTC_FLAG_SIMPLE_KERNEL it is NTC_ERR_ARG; ntc_hll_create_ex refuses it.  Checked before a device is looked for.
 *   - Every plane of a signature engine is the general kernel's (K1), exactly as for a strand engine without NTC_FLAG_STRAND_TILED: tiled, ragged and binned
 *     batches are re-laid out on the device, NTC_FLAG_REQUIRE_TILED makes those submits fail with nothing counted, host batches take row slots,
 *     ntc_submit_long_device gathers every sequence whole (ntc_long_stats stays (0, 0)); NTC_FLAG_STRAND_TILED is accepted and has no effect.
 *   - K1 appends the sampled values to a per-plane log on the device; an insert pass moves the log into an open-addressing table per plane (12 B per slot,
 *     at most half full: 24 .. 48 B per distinct value), which doubles as it fills.  The engine books a launch's WINDOWS in the log (a read set may sample
 *     every window; plus one chunk of 1024 entries per wave), so a batch with more windows than the log holds is counted in several launches; every insert
 *     pass waits for the stream once (it reads the log's fill and the tables' live counts back): once per 2^27 booked windows, not once per submit.  A table that cannot grow makes the submit or sync fail with NTC_ERR_MEMORY; nothing is dropped
 *     silently.  Environment, read per engine: NTC_SIG_SLOTS (initial slots per plane, a power of two >= 64; default 2^16), NTC_SIG_LOG_ENTRIES (the value
 *     log's capacity per plane in entries; default 2^27 = 1 GiB, allocated as far as the batches need it).
 *   - ntc_reset empties the signatures, ntc_destroy frees them; ntc_merge_devices refuses a mix of engines with and without the flag and unions the
 *     signatures of engines 1 .. into engine 0's (counts added); ntc_merge_counters moves no signature.
 * (Bits 4, 256, 2048 and 1 << 20 stay refused as unknown flags.)  DESIGN.md §4 "Signatures". */
#define NTC_FLAG_SIGNATURE 16384u
#define NTC_FLAG_DIRECT_ATOMICS 2u /* no hit log: every sampled k-mer is one device atomic on the sketch
                                      (the literal form of ntcard.cpp:142-143; cross-check and A/B runs) */

uint32_t ntc_abi_version(void);
uint32_t ntc_max_k(void);
const char *ntc_last_error(void);

/* ntcard.cpp:437-439 (allocate + zero t_Counter), :433-435 (zero F1) */
int ntc_create(const ntc_config *cfg, ntc_engine **out);

/* An engine whose planes are SPACED SEEDS given as masks: seeds[i] is a string of k_i characters '0' / '1'
 * (1 <= k_i <= ntc_max_k(), at least one '1'); offset 0 is the leftmost base of the window.  This is the seed
 * syntax of the reference's hash library (stHashIterator::parseSeed, stHashIterator.hpp:23-33; NTMSM64,
 * nthash.hpp:620-678), which ntcard itself only uses for the one shape 1^a 0^g 1^a of -g (ntcard.cpp:407-413).
 * For every window of k_i bases of a read:
 *   - the window counts (F1 of the plane, t_Counter) only when ALL k_i bytes are bases, those under a '0' included
 *     (the -g path's rule: stHashIterator::next, NTMSM64);
 *   - its value starts from the plain ntHash fh / rh of the window (nthash.hpp:220-239); for every i with mask[i] == '0'
 *       fs ^= srol^(k-1-i)(seed[b_i]),   rs ^= srol^i(seed[b_i & cpOff])
 *     and the canonical value is rs < fs ? rs : fs (NTMSM64 with m = m2 = 1);
 *   - ntComp (ntcard.cpp:132-145) counts it into the plane of that mask.
 * Planes follow the order of `seeds` like a k list: t_counter[n_seeds][2][1 << r_bits], f1[n_seeds]; the engine's k list
 * is the masks' lengths, so ntc_finish, ntc_merge_counters, the log calls and ntc_merge_devices (which refuses engines
 * whose seed lists differ) work unchanged.  A mask of '1's only is a plain k-mer plane, 1^a 0^g 1^a is ntcard's -g g
 * seed (bit-identical results to ntc_create with gap = g); one list may mix masks of any length and shape.
 * cfg->n_k == 0, cfg->k == NULL, cfg->gap == 0; everything else of cfg as for ntc_create.  1 <= n_seeds <= NTC_MAX_K_LIST.
 * NTC_FLAG_SIMPLE_KERNEL with a mask that has a '0' is an argument error.  Every argument is checked before a device
 * is looked for.  Tiled batches: the tiled kernels take the plain planes and ntcard's two tiled -g seeds (k 12 / g 2,
 * k 32 / g 8); every other spaced plane is counted from a row-slot copy of the batch (NTC_FLAG_REQUIRE_TILED: an error,
 * before anything is counted). */
int ntc_create_seeded(const ntc_config *cfg, uint32_t n_seeds, const char *const *seeds, ntc_engine **out);
void ntc_destroy(ntc_engine *e);                 /* ntcard.cpp:474 */
int ntc_reset(ntc_engine *e);                    /* re-zero sketch and F1 */

/* ntRead/stRead for a batch of sequences (ntcard.cpp:147-171).  HOST buffers:
 * bases = concatenated raw sequence bytes exactly as the parsers produced them (any case, any
 * IUPAC/N byte), offsets[n_reads+1] delimits read i = bases[offsets[i], offsets[i+1]).
 * The engine copies what it needs before returning (caller keeps ownership): reads are packed
 * into one of a few pinned staging buffers, then copy + kernels are queued on the engine's
 * stream; device-side errors surface at ntc_sync/ntc_finish.  Thread-safe: may be called
 * concurrently from several parser threads like the reference's seam (packing runs in parallel,
 * only the enqueue is serialised).                                                             */
int ntc_submit(ntc_engine *e, const char *bases, const uint64_t *offsets, uint64_t n_reads);

/* The same for reads that are SPANS of one host buffer: read i = buf[starts[i], starts[i] + lens[i]).  This is what a
 * block-based record splitter produces (the sequence lines of a FASTQ block, field 10 of SAM lines): the bytes are
 * copied exactly once, from the file block into the pinned staging buffer.  Same threading and ownership rules.  */
int ntc_submit_spans(ntc_engine *e, const char *buf, const uint64_t *starts, const uint32_t *lens, uint64_t n_reads);

/* Same for a batch that is already DEVICE-resident in the engine's slot layout: read i occupies
 * d_slots[i*stride, i*stride+read_len), stride % 4 == 0, d_slots 16-byte aligned.  Padding bytes
 * (read_len..stride) are never hashed; filling them with a base letter ('A') keeps the kernel on
 * its fast path (a non-ACGTU byte anywhere in a wave's 64 slots selects the dirty-window path).
 * Asynchronous on the engine's stream: the buffer may be reused as soon as the stream has passed the call (stream-ordered,
 * like a kernel launch) — unless the engine was created with NTC_FLAG_DEFER_REDO, see there.
 * A wave parks its 64 slots in LDS, so stride is limited to about 2.4 KB (64 * stride + tables <= 160 KiB);
 * longer sequences go through ntc_submit, which splits them into overlapping chunks, or — device-resident — through
 * ntc_submit_long_device.                                                                       */
int ntc_submit_device(ntc_engine *e, const void *d_slots, uint64_t n_reads, uint32_t read_len,
                      uint32_t stride);

/* The same for a DEVICE-resident batch in the engine's TILED slot layout — the layout the hot kernel pair (K1h + K1f) streams:
 *     tile t   = reads [2048 t, 2048 t + 2048) of the batch,       n_chunks = ceil(read_len / 16)
 *     piece    = the 16 raw bytes of bases [16 c, 16 c + 16) of read i, at byte offset
 *                ((i / 2048 * n_chunks + c) * 2048 + i % 2048) * 16          (ntc_tiled_bytes() bytes in all)
 * i.e. the pieces of one base range of a tile's 2048 reads are contiguous (32 KiB): one coalesced load hands every lane
 * the next 16 bases of "its" read, in the position-major order the bit-sliced hash walk consumes.  Bytes are raw sequence
 * bytes as the parsers produce them (any case, N / IUPAC); bytes behind a read's end (inside its last piece) must hold a base
 * letter ('A'); the slots behind the batch's last read (the rest of the last tile) are ignored whatever they hold, so any
 * prefix of a tiled buffer is a valid batch.  All reads of a batch have the same length.  Asynchronous on the engine's
 * stream; the buffer may be reused as soon as the stream has passed the call — unless the engine was created with
 * NTC_FLAG_DEFER_REDO, see there.  A list of k is served by one launch per k.  The tiled kernels are built for k = 12 .. 32
 * (spaced seeds: ntcard's -g seed at k = 12 / gap 2 and k = 32 / gap 8) and sBits >= 7; a list of which only a part lies in 12 .. 32
 * is served by both kernels from the same tiles (the general kernel stages the tiles for its k: no re-layout); a configuration in
 * which NO k is theirs (every k outside 12 .. 32, other spaced seeds, nthll, sBits < 7) is re-laid out on the device and takes the
 * general kernel: same results, not the fast path.  Host batches reach the same kernels: ntc_submit / ntc_submit_spans pack them
 * into tiles in pinned staging (reads of one length as one batch, mixed lengths as the length bins of ntc_submit_tiled_bins_device). */
int ntc_submit_tiled_device(ntc_engine *e, const void *d_tiles, uint64_t n_reads, uint32_t read_len);
uint64_t ntc_tiled_bytes(uint64_t n_reads, uint32_t read_len);

/* The same for reads of UNEQUAL length (ntRead takes any sequence, ntcard.cpp:173-189; adapter-trimmed FASTQ) — ABI 5.  A ragged tiled batch holds
 * reads of 16 * n_chunks - 15 .. 16 * n_chunks bases (one bin of ceil(len / 16)) in the tiled layout of ntc_submit_tiled_device with
 * read_len = 16 * n_chunks; bytes behind a read's end hold a base letter ('A').  EVERY TILE IS SORTED LONGEST READ FIRST (counting is
 * order-independent, so a producer may reorder), and d_tails[tile * 16 + d], d = 0 .. 15, is the number of reads of that tile with more than d
 * bases in their last 16-base piece (d_tails[tile * 16] = the reads of the tile; non-increasing in d).  The kernel masks every window that ends
 * behind a read's end with the prefix of the tile that is long enough: no per-read length array, 64 bytes per tile.  d_tails follows the rules of
 * d_tiles (device memory, valid until the stream has passed the call — until ntc_sync with NTC_FLAG_DEFER_REDO).  Fails with NTC_ERR_ARG on an
 * engine in whose configuration NO k is the tiled kernels' (ABI 6: a list of which only a part is theirs is fine — the general kernel stages the same
 * tiles for its k and takes every read's length from a table the engine derives from d_tails).  ntc_submit / ntc_submit_spans build such batches themselves: a host batch of
 * mixed lengths is binned by ceil(len / 16), bins of >= 1024 reads go this way, the rest takes row slots.                                      */
int ntc_submit_tiled_ragged_device(ntc_engine *e, const void *d_tiles, uint64_t n_reads, uint32_t n_chunks, const uint32_t *d_tails);

/* Several tiled batches of different geometry in ONE call — the length bins of a ragged read set (ABI 5).  Bin i is d_tiles[i] with n_reads[i] reads of
 * read_len[i] bases; d_tails[i] == NULL (or d_tails == NULL: all of them): an equal-length batch as for ntc_submit_tiled_device, otherwise a ragged one as for
 * ntc_submit_tiled_ragged_device (read_len[i] = 16 * n_chunks).  Counts exactly what n_bins separate calls count; the difference is speed: the
 * hash kernel takes up to 8 bins per launch and shares its workgroups among them in proportion to their work, where separate calls are separate,
 * small launches (four 2.5 M-read bins: 0.55 ms one by one, 0.39 ms together).  Empty bins are skipped.  NTC_ERR_ARG as for the single calls.    */
int ntc_submit_tiled_bins_device(ntc_engine *e, uint32_t n_bins, const void *const *d_tiles, const uint64_t *n_reads, const uint32_t *read_len,
                                 const uint32_t *const *d_tails);

/* LONG sequences that are already DEVICE-resident — a chromosome or contig, HiFi / ONT reads, an assembler's or a decompressor's output: what the reference's
 * FASTA / SAM parsers hand to ntRead one sequence at a time (ntcard.cpp:147-158,173-208) — additive to ABI 6.  d_bases is device memory holding the
 * concatenated raw bytes (any byte: N, IUPAC, lower case; any alignment), sequence i = d_bases[offsets[i], offsets[i + 1]), offsets a HOST array of
 * n_seqs + 1 non-decreasing entries.  Stream-ordered: d_bases may be reused as soon as the stream has passed the call, under NTC_FLAG_DEFER_REDO too (the
 * engine counts from scratch of its own, so this call never defers); offsets is free on return.  The kernels read d_bases in aligned 4-byte words, and only
 * words that hold at least one byte of a sequence.
 * An engine QUALIFIES when every plane is the tiled kernels' (plain k = 12 .. 32 or the two tiled -g seeds, sBits >= 7; canonical, or one strand with
 * NTC_FLAG_STRAND_TILED) and it has either one
 * plane or a list of plain k with kmax - kmin <= 15.  Every sequence of n >= piece_len bytes is then cut on the device into the full pieces
 * [j S, j S + piece_len) of ntc_long_plan(kmax, ..), S = piece_len - (kmax - 1): ONE cut, with the overlap of the largest k, for the whole list — an
 * equal-length tiled batch counted by K1h + K1f at their rate, once per k.  A k of the list owns the windows that start in a piece's first S bytes: the
 * windows of a read of piece_len - (kmax - k) bases, which is how the tiled kernels are launched for it over the same tiles (the limit of 15 keeps that
 * length inside the piece's last 16-byte chunk).  So each window of each k lies in exactly one piece or in the remainder [m S, n).  The remainder is gathered
 * into row slots for the general kernel iff it holds a window of kmin (n - m S >= kmin), like every sequence shorter than piece_len.  piece_len: 0 = the
 * engine's choice (1008), or a multiple of 16 with kmax + 15 <= piece_len <= 65520.  The work goes in rounds of at most 1 GiB of engine scratch, whatever the
 * input's size.  The host builds and sends 16 B per sequence that holds a full piece (its offset and the index of its first piece) and 16 B per row slot:
 * the pieces' offsets are derived on the device.
 * On every other engine (a list wider than 15 or with a k outside 12 .. 32, k > 32, other seeds, a strand without NTC_FLAG_STRAND_TILED, nthll, sBits < 7, NTC_FLAG_LANE_KERNEL,
 * NTC_FLAG_SIMPLE_KERNEL) every sequence is gathered whole: exactly ntc_submit's results, ntc_long_stats stays (0, 0) — with NTC_FLAG_REQUIRE_TILED the call
 * fails with NTC_ERR_ARG instead and counts nothing.
 * NTC_ERR_ARG for null pointers, a bad piece_len or offsets that decrease, checked before a device is looked for.
 * ntc_submit / ntc_submit_spans take the same path for the long sequences of a host batch on such an engine: the sequences of two or more full pieces
 * (piece_len 1008) are copied raw into staging and cut on the device once together they hold 32768 full pieces (about 32 MB; below that row slots are as fast
 * or faster, profiles/long_seq.txt); the environment variable NTC_LONG_MIN, read per call, sets another number (0: never).  Same counts either way. */
int ntc_submit_long_device(ntc_engine *e, const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t piece_len);

/* The cut ntc_submit_long_device makes of ONE sequence of len bytes (a pure host function; ntRead's window loop, ntcard.cpp:147-158,173-208, split
 * into ranges); k: the engine's k, for a list its LARGEST.  *pieces = m full pieces [j S, j S + piece_len), j < m, S = piece_len - (k - 1); *rem_start = m S:
 * the remainder [m S, len) — the whole sequence when len < piece_len (m = 0), else k - 1 .. piece_len - 1 bytes — holds a window of a k' <= k iff
 * len - m S >= k' (the engine counts it iff that holds for the smallest k of its list).  For every k' of a list within k - 15 .. k, the windows that start in
 * the first S bytes of the pieces and the windows of the remainder are the sequence's windows of k' bases, each once.  NTC_ERR_ARG unless piece_len is a
 * multiple of 16 with k + 15 <= piece_len <= 65520. */
int ntc_long_plan(uint32_t k, uint32_t piece_len, uint64_t len, uint64_t *pieces, uint64_t *rem_start);

/* cumulative since create / reset: the full pieces ntc_submit_long_device (and the host path behind NTC_LONG_MIN) has cut for the tiled kernels and the
 * sequences that contributed one (ntcard.cpp:147-158,173-208: the ntRead calls that went that way) — a diagnostic, like ntc_merge_allocations */
int ntc_long_stats(ntc_engine *e, uint64_t *pieces, uint64_t *sequences);
/* milliseconds of the cut and of the gather kernels while profiling (ntc_set_profiling), outside ntc_kernel_time's spans; either pointer may be NULL */
int ntc_long_time(ntc_engine *e, double *cut_ms, double *gather_ms);

/* Homopolymer compression of ONE sequence of n bytes (NTC_FLAG_HPC has the definition) — a pure host function, what ntc_submit / ntc_submit_spans run per
 * read on an engine with the flag.  out has room for n bytes; out == in is allowed (any other overlap is not); *n_out = the bytes kept.  NTC_ERR_ARG for a
 * null n_out, or a null in / out with n != 0. */
int ntc_hpc_compress(const char *in, uint64_t n, char *out, uint64_t *n_out);
/* The same for DEVICE-resident sequences, by the kernels an engine with NTC_FLAG_HPC runs in ntc_submit_long_device (a stand-alone tool, like
 * ntc_hash_dump_device): d_in and offsets as for ntc_submit_long_device (any alignment; a HOST array of n_seqs + 1 non-decreasing entries), d_out device
 * memory of any alignment with room for offsets[n_seqs] - offsets[0] bytes, not overlapping d_in; offsets_out a HOST array of n_seqs + 1 entries:
 * offsets_out[0] = 0, sequence i of the result = d_out[offsets_out[i], offsets_out[i + 1]).  Synchronous.  NTC_ERR_ARG for null pointers and offsets that
 * decrease, checked before the device is touched.  The call allocates its scratch (an eighth of the input and 12 B per 4 KiB) and frees it. */
int ntc_hpc_compress_device(int32_t device, void *stream, const void *d_in, const uint64_t *offsets, uint64_t n_seqs, void *d_out, uint64_t *offsets_out);
/* cumulative since create / reset: the sequence bytes an engine with NTC_FLAG_HPC was given and the bytes it kept, over the host and the device paths
 * alike; (0, 0) for ever on an engine without the flag */
int ntc_hpc_stats(ntc_engine *e, uint64_t *bytes_in, uint64_t *bytes_out);
/* milliseconds of the compaction kernels of ntc_submit_long_device while profiling (ntc_set_profiling), outside ntc_kernel_time's spans, like ntc_long_time */
int ntc_hpc_time(ntc_engine *e, double *ms);

/* ---- signatures (NTC_FLAG_SIGNATURE); plane: index into the k list / seed list.  NTC_ERR_STATE on an engine without the flag, NTC_ERR_ARG for a bad plane ---- */
/* brings pending work in (the value log is inserted; waits for the stream) and returns the number of distinct sampled values of the plane */
int ntc_signature_size(ntc_engine *e, uint32_t plane, uint64_t *n);
/* the plane's pairs, strictly ascending by hash: hashes[cap], counts[cap] (HOST; counts may be NULL), *n = the pairs written.  cap smaller than the
 * plane's size: NTC_ERR_ARG and nothing is written, *n included (ask ntc_signature_size).  The pairs are gathered AND sorted on the device (ntc_signature_sort_device's kernels, with scratch the engine keeps: a
 * second pair buffer and the sort's histograms, 12 B per pair); when that scratch cannot be had: NTC_ERR_MEMORY and nothing is written.
 * ntc_signature_device: the same with the sorted pairs left in caller-owned DEVICE arrays on the engine's device (d_counts_u32 may be NULL); the same
 * checks, the same refusal of a short cap; the arrays are complete when the call returns. */
int ntc_signature(ntc_engine *e, uint32_t plane, uint64_t *hashes, uint32_t *counts, uint64_t cap, uint64_t *n);
int ntc_signature_device(ntc_engine *e, uint32_t plane, void *d_hashes_u64, void *d_counts_u32, uint64_t cap, uint64_t *n);
/* adds n pairs to the plane's signature: the merge-in for checkpoints and peers (and how tests drive the container on chosen keys).  counts == NULL: 1
 * each; duplicates inside a call are legal and add up; zeros are skipped; counts saturate at 2^32 - 1.  ntc_signature_inject: HOST arrays (copied before
 * the call returns).  ntc_signature_inject_device: DEVICE arrays, read stream-ordered on the engine's stream (they may be reused once the stream has
 * passed the call; the call itself waits for the stream only when a table has to grow).  Neither touches t_Counter or F1. */
int ntc_signature_inject(ntc_engine *e, uint32_t plane, const uint64_t *hashes, const uint32_t *counts, uint64_t n);
int ntc_signature_inject_device(ntc_engine *e, uint32_t plane, const void *d_hashes_u64, const void *d_counts_u32, uint64_t n);
/* |A n B| of two hash lists (a pure host function): both strictly ascending, else NTC_ERR_ARG.  Jaccard = c / (na + nb - c), containment of A in B = c / na. */
int ntc_signature_compare(const uint64_t *a, uint64_t na, const uint64_t *b, uint64_t nb, uint64_t *n_common);
/* diagnostics: the table slots of all planes together and the doublings of a table since create / reset (a table that grows 64 -> 65536 slots in one
 * rehash counts 10); ntc_signature_time: milliseconds of the insert passes and of the rehashes while profiling (ntc_set_profiling), outside ntc_kernel_time */
int ntc_signature_stats(ntc_engine *e, uint64_t *slots, uint64_t *grows);
int ntc_signature_time(ntc_engine *e, double *insert_ms, double *grow_ms);
/* milliseconds of the device sorts of ntc_signature / ntc_signature_device while profiling (their one wait for the digit histograms included) */
int ntc_signature_sort_time(ntc_engine *e, double *ms);
/* Engine-less device tools (like ntc_hpc_compress_device: `device`, `stream` a hipStream_t or NULL; all three are synchronous and free their scratch).
 *   ntc_signature_sort_device    sorts n pairs (uint64 key, uint32 value) in place, ascending by unsigned key and STABLE (equal keys keep their order);
 *       d_vals_u32 may be NULL (keys only).  An LSD radix sort of 8-bit digits that skips every digit in which all keys agree; up to 4096 pairs are sorted by
 *       one launch in LDS.  NTC_ERR_ARG for a NULL key array with n != 0 or n >= 2^32 (before the device is touched); NTC_ERR_MEMORY when the scratch — a
 *       second key and value array plus histograms — cannot be had, with nothing changed; n == 0 touches nothing.
 *   ntc_signature_compare_device *n_common = |A n B| of two strictly ascending DEVICE lists; when both count arrays and min_sum are non-NULL, *min_sum = the
 *       sum of min(count_a, count_b) over the common hashes (uint64: the numerator of the abundance-weighted Jaccard), else min_sum is left alone.  Ascent
 *       is checked on the device: NTC_ERR_ARG names the list and an offending entry, as ntc_signature_compare does.  NULL n_common, or a NULL list with a
 *       length: NTC_ERR_ARG before the device is touched.  Empty lists are legal.
 *   ntc_signature_matrix_device  all pairs at once: d_hashes_u64 is a HOST array of n_sigs DEVICE lists (1 <= n_sigs <= 1024; list i has n[i] strictly
 *       ascending hashes, NULL allowed where n[i] == 0), common_out a HOST array [n_sigs][n_sigs]: common_out[i][j] = |S_i n S_j|, symmetric, the diagonal
 *       n[i].  Every list's ascent is checked once; NTC_ERR_ARG names the index of an unsorted list.  The pairs are cut into work items (a pair and 4096
 *       entries of its shorter list) that run 2^18 per launch.  On any error common_out is left alone. */
int ntc_signature_sort_device(int32_t device, void *stream, void *d_keys_u64, void *d_vals_u32, uint64_t n);
int ntc_signature_compare_device(int32_t device, void *stream, const void *d_a_u64, const void *d_ca_u32, uint64_t na, const void *d_b_u64,
                                 const void *d_cb_u32, uint64_t nb, uint64_t *n_common, uint64_t *min_sum);
int ntc_signature_matrix_device(int32_t device, void *stream, uint32_t n_sigs, const void *const *d_hashes_u64, const uint64_t *n, uint64_t *common_out);
/* Gather, another engine-less device tool (synchronous, frees its scratch): which references are in a query, and how much of it does each explain on its
 * own — the greedy minimum-set-cover decomposition of FracMinHash tools.  The query: nq strictly ascending DEVICE hashes with optional uint32 counts
 * (NULL: 1 each); d_refs_u64: a HOST array of n_refs DEVICE lists (1 <= n_refs <= 1024; list i has n[i] strictly ascending hashes, NULL allowed where
 * n[i] == 0).  Every query entry starts live.  A round counts, for every reference, the live query entries it holds (unique); the reference with the most
 * wins, the lowest index among equals; the run stops, with nothing more reported, when that count is below `threshold` (a number of hashes; 0 is taken as
 * 1), when rows_cap rows are written or after n_refs rounds; else the round writes rows[r] = {ref, common = |Q n R_ref| on the whole query, unique,
 * unique_weight = the sum of the query's counts over those live entries} and the entries stop being live.  *n_rows = the rows written, *unassigned = the
 * query entries still live after the last reported row, *unassigned_weight = the sum of their counts (both may be NULL).  So a reference given twice is
 * reported once, one inside an earlier pick never, the rows' unique values do not increase and they add up, with *unassigned, to nq.  All results are
 * integer sums: exact and the same on every run.
 * NTC_ERR_ARG before the device is touched: n_refs outside 1 .. 1024, nq or an n[i] >= 2^32, NULL n_rows, NULL rows with rows_cap != 0, a NULL list with a
 * length.  Ascent of the query and of every reference is checked once on the device: NTC_ERR_ARG names the list ("the query", or the reference's index)
 * and an offending entry.  NTC_ERR_MEMORY when the scratch cannot be had (a byte per query entry, 4 B per common hash of every reference with the
 * query).  On any error every output is left alone.  rows_cap == 0 is legal: *n_rows = 0 and the whole query is unassigned. */
typedef struct {
    uint32_t ref, reserved;     /* index into d_refs_u64; 0 */
    uint64_t common, unique, unique_weight;
} ntc_gather_row;
int ntc_signature_gather_device(int32_t device, void *stream, const void *d_query_u64, const void *d_query_counts_u32, uint64_t nq, uint32_t n_refs,
                                const void *const *d_refs_u64, const uint64_t *n, uint64_t threshold, ntc_gather_row *rows, uint32_t rows_cap,
                                uint32_t *n_rows, uint64_t *unassigned, uint64_t *unassigned_weight);
/* SET ALGEBRA AND SPECTRUM (additive to ABI 6: three calls and three constants; NTC_ABI_VERSION and every other declaration are unchanged).  Engine-less
 * device tools like the ones above: synchronous, on the caller's `stream`, and they free their scratch.  New signatures out of existing ones, and the
 * abundance spectrum of one, without an engine.  Every result is an exact integer.
 *   ntc_signature_union_device   1 <= n_lists <= 1024; d_hashes_u64 and n are HOST arrays, list i has n[i] strictly ascending DEVICE hashes (NULL allowed
 *       where n[i] == 0); d_counts_u32 is NULL, or a HOST array whose entry i is NULL or a DEVICE array of n[i] counts — NULL means 1 each.  The result: the
 *       distinct hashes of all lists, strictly ascending, each with min(the sum of its counts over the lists, 2^32 - 1).  A hash of 0 is a value like any
 *       other here, as for compare.  The sum of the n[i] is below 2^32 (the sort's limit).  The lists are gathered into one pair buffer, sorted
 *       (ntc_signature_sort_device's kernels), and every head of a run of equal hashes — at most n_lists long — adds up its run; n_lists == 1 is a checked
 *       copy.  Scratch: 25 B per entry of the input (two pair buffers of 12 B — one up to 4096 entries —, a byte of flag), the sort's histograms and 4 B
 *       per 2048 entries.  The host waits three times: for the sort's digit histograms (above 4096 entries), in front of the scatter, and at the end.
 *   ntc_signature_select_device  an entry (h, c) of A (na strictly ascending DEVICE hashes; c = 1 when d_ca_u32 == NULL) is kept iff it passes the count
 *       test — min_count <= c, and c <= max_count unless max_count == 0 (no upper bound) — and the membership test: the rule of `mode` over the n_refs
 *       reference lists (0 <= n_refs <= 1024; d_refs_u64 and n as above, both may be NULL with 0 references; na and every n[i] below 2^32).  Kept entries
 *       keep A's order, hashes and counts.  An empty reference holds nothing: under NTC_SIG_IN_ALL nothing is kept, under NTC_SIG_IN_NONE it excludes
 *       nothing.  So intersect is IN_ALL, subtract IN_NONE, and the abundance filter is n_refs == 0 with bounds.  NTC_ERR_ARG for min_count > max_count != 0
 *       or a mode above 2.  A lane per entry of A searches reference after reference and leaves at the first that decides.  Scratch: a byte per entry of A
 *       and 4 B per 2048 entries.  The host waits twice: in front of the scatter, and at the end.
 *   Output of both: d_out_u64 has room for cap hashes, d_out_counts_u32 (may be NULL: hashes only) for cap counts, *n_out = the size of the result.
 *       d_out_u64 == NULL asks for the size alone and is legal only with cap == 0 and d_out_counts_u32 == NULL: NTC_OK, *n_out is set, nothing else is
 *       written.  A cap smaller than the result: NTC_ERR_ARG, the message names the needed size, nothing is written; the sum of the n[i] (union) and na
 *       (select) are always enough.  An output array that overlaps an input array: NTC_ERR_ARG, decided from the pointer ranges.  NTC_ERR_ARG before the
 *       device is touched also for a NULL n_out, a NULL table or n with lists to read, a NULL list with a length, a length or a sum >= 2^32, n_lists
 *       outside 1 .. 1024, n_refs > 1024.  Ascent of every input list is checked once on the device: NTC_ERR_ARG names the list ("A", "list i",
 *       "reference i") and an offending entry.  NTC_ERR_MEMORY when the scratch cannot be had.  On ANY error every output is left alone: both arrays and
 *       *n_out.
 *   ntc_signature_hist_device    the abundance spectrum of a signature's n DEVICE counts (any n): hist_out, a HOST array [cov_max + 2], gets
 *       hist_out[v] = the entries with count v for 0 <= v <= cov_max and hist_out[cov_max + 1] = the entries with a larger count; *weight_out (may be
 *       NULL) = the sum of the counts.  The spectrum of the SAMPLED distinct k-mers, exact and free of collisions: what the estimator's f[] estimates,
 *       scaled by the sampling rate.  1 <= cov_max <= 65535.  NTC_ERR_ARG for a NULL hist_out, a cov_max outside that range or a NULL d_counts_u32 with
 *       n != 0, all before the device is touched; n == 0 touches no device.  One launch, one wait; scratch (cov_max + 3) x 8 B. */
#define NTC_SIG_IN_ALL  0u   /* keep an entry of A iff every reference holds it (no references: every entry) */
#define NTC_SIG_IN_NONE 1u   /* ... iff no reference holds it                                               */
#define NTC_SIG_IN_ANY  2u   /* ... iff at least one reference holds it (no references: none)               */
int ntc_signature_union_device(int32_t device, void *stream, uint32_t n_lists, const void *const *d_hashes_u64, const void *const *d_counts_u32,
                               const uint64_t *n, void *d_out_u64, void *d_out_counts_u32, uint64_t cap, uint64_t *n_out);
int ntc_signature_select_device(int32_t device, void *stream, const void *d_a_u64, const void *d_ca_u32, uint64_t na, uint32_t n_refs,
                                const void *const *d_refs_u64, const uint64_t *n, uint32_t mode, uint32_t min_count, uint32_t max_count, void *d_out_u64,
                                void *d_out_counts_u32, uint64_t cap, uint64_t *n_out);
int ntc_signature_hist_device(int32_t device, void *stream, const void *d_counts_u32, uint64_t n, uint32_t cov_max, uint64_t *hist_out,
                              uint64_t *weight_out);
/* A signature FILE (`ntcard --signature`, bin/ntsig): little-endian; the 8 bytes "NTCSIG1\0", uint32 k, gap, strand, hpc, s_bits, mask_len, uint64 n, the mask
 * (mask_len bytes '0' / '1', all '1' for plain k; zero-padded to a multiple of 8), uint64 hashes[n], uint32 counts[n].  The header says how the file was
 * counted: two files compare only when they agree in everything but n.  Pure host functions.
 *   ntc_signature_write  h->mask: k characters; NTC_ERR_ARG for a bad header, hashes that are not strictly ascending or a file that cannot be written
 *   ntc_signature_read   fills *h; hashes / counts (either may be NULL: skipped) have room for cap pairs — cap < n with a non-NULL array: NTC_ERR_ARG after
 *                        *h is filled, so a first call with cap = 0 and NULL arrays learns n; NTC_ERR_ARG for a file that is not a signature or is cut short */
#define NTC_SIG_MASK_MAX 608
typedef struct {
    uint32_t k, gap;            /* window length; -g of the run (0: none, or a mask given with --seed) */
    uint32_t strand, hpc;       /* 0 canonical, 1 forward, 2 reverse; 1: homopolymer-compressed */
    uint32_t s_bits, reserved;
    uint64_t n;                 /* pairs */
    char mask[NTC_SIG_MASK_MAX]; /* NUL-terminated */
} ntc_sig_header;
int ntc_signature_write(const char *path, const ntc_sig_header *h, const uint64_t *hashes, const uint32_t *counts);
int ntc_signature_read(const char *path, ntc_sig_header *h, uint64_t *hashes, uint32_t *counts, uint64_t cap);
/* the header of plane `plane` of a signature engine (k, gap, mask, strand, hpc, s_bits; n = 0): what ntc_signature_write needs beside the pairs */
int ntc_signature_header(ntc_engine *e, uint32_t plane, ntc_sig_header *h);

/* BLOOM FILTERS of EVERY k-mer (additive to ABI 6: nine calls, one constant, one struct; NTC_ABI_VERSION and every other declaration are unchanged).
 * What ntCard's F0 is for: the filter a downstream tool sizes from the `.hist` file, built and queried by the same ntHash walk.  The layout is the
 * reference's vendor/ntHash/lib/BloomFilter.hpp: position loc_i = h_i % m_bits, bit 7 - loc % 8 of byte loc / 8, h_0 the window's value and
 * h_i = (t ^ t >> 27), t = h_0 * (i ^ k * multiSeed) for 1 <= i < n_hash (nthash.hpp:381-390).  Engine-less device tools like the signature tools above:
 * synchronous, on the caller's `stream`, and they free their scratch.
 *   The filter    caller-owned DEVICE memory: (m_bits + 7) / 8 bytes rounded up to a multiple of 4, 4-byte aligned, zeroed by the caller before the
 *       first insert.  The bits from m_bits on (the padding) stay zero.  1 <= m_bits < 2^40, 1 <= n_hash <= 32, 1 <= k <= ntc_max_k().
 *   The input     as for ntc_hpc_compress_device: d_bases DEVICE bytes of any alignment, offsets a HOST array of n_seqs + 1 non-decreasing values,
 *       sequence i = d_bases[offsets[i], offsets[i + 1]); offsets[0] need not be 0, empty sequences are legal, n_seqs and the byte range need not fit
 *       32 bits (at most 2^43 bytes in one call).  A window [p, p + k) counts iff it lies inside one sequence and every byte is one of A C G T U, either
 *       case — the windows ntHashIterator yields on text (the control bytes 1, 3, 4, 5, 7 that the reference's seed table also maps are NOT bases
 *       here).  A sequence shorter than k contributes nothing.  strand: 0 canonical min(fh, rh), 1 forward fh, 2 reverse rh (the numbers of
 *       NTC_FLAG_STRAND_*).  Homopolymer compression is not a flag here: a caller who wants it runs ntc_hpc_compress_device first and passes its output.
 *   ntc_bloom_size           pure host: m = ceil(-n_distinct * n_hash / ln(1 - fpr^(1 / n_hash))) rounded up to a multiple of 64.  NTC_ERR_ARG for
 *       n_distinct == 0, n_hash outside 1 .. 32, fpr outside (0, 1), a NULL m_bits or a result of 2^40 or more.  It serves both kinds of filter: the
 *       positions it returns are bits for a plain filter and counters for a counting one (below).
 *   ntc_bloom_insert_device  sets the n_hash bits of every window; *n_windows = the windows inserted (may be NULL).  The byte range is cut into blocks
 *       of NTC_BLOOM_BLOCK window starts, counted from offsets[0]; a workgroup stages its block's bytes in LDS and a lane rolls over 16 consecutive
 *       windows.  A bit that a plain load already finds set costs no atomic.  Scratch: the offsets (8 B per sequence) and 8 B.
 *   ntc_bloom_query_device   d_windows_u32[i] = the windows of sequence i, d_hits_u32[i] = those whose n_hash bits are all set; both DEVICE arrays of
 *       n_seqs uint32, zeroed by the call (a sequence of 2^32 windows or more wraps).  Exact integers: the same on every run.
 *   ntc_bloom_insert_hashes_device / ntc_bloom_query_hashes_device  the same bit arithmetic on n GIVEN h_0 values (DEVICE uint64), without hashing:
 *       a signature's hashes go in this way.  d_flags_u8[i] = 1 iff all n_hash bits of d_h0_u64[i] are set, else 0.  k enters h_i only.
 *   ntc_bloom_popcount_device  *pop = the set bits among the first m_bits; NTC_ERR_STATE when a padding bit is set (then it is no filter of m_bits).
 *   ntc_bloom_or_device      d_dst |= d_src, two filters of the same m_bits (shards of one input, peers' filters); the padding is OR-ed too.
 * Before the device is touched, NTC_ERR_ARG for: a NULL pointer that is needed (the filter; offsets; d_bases with bytes to read; the outputs of a query;
 * d_h0_u64 with n != 0; pop), a filter that is not 4-byte aligned, offsets that decrease, k, n_hash, m_bits or strand out of range.  NTC_ERR_MEMORY when
 * the scratch cannot be had.  On any error nothing is written.
 * A filter FILE (bin/ntbloom): the 8 bytes "NTCBF1\0\0", the header below little-endian, then the reference's byte image — (m_bits + 7) / 8 bytes, as
 * BloomFilter::storeFilter writes them.  Pure host functions.
 *   ntc_bloom_write  writes path + ".part" and renames it when it is whole, so a failure leaves nothing behind; NTC_ERR_ARG for a bad header
 *                    (the ranges above, reserved == 0) or a file that cannot be written
 *   ntc_bloom_read   fills *h; filter_bytes has room for cap_bytes — cap_bytes smaller than the image with a non-NULL array: NTC_ERR_ARG after *h is
 *                    filled, so a first call with cap_bytes == 0 and a NULL array learns the header; NTC_ERR_ARG for a file that is no filter file, has a
 *                    bad header, is cut short or holds more than its header says */
#define NTC_BLOOM_BLOCK 4096u   /* window starts per workgroup: block b holds the starts [b * NTC_BLOOM_BLOCK, (b + 1) * NTC_BLOOM_BLOCK) behind offsets[0] */
int ntc_bloom_size(uint64_t n_distinct, uint32_t n_hash, double fpr, uint64_t *m_bits);
int ntc_bloom_insert_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand,
                            const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, uint64_t *n_windows);
int ntc_bloom_query_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand,
                           const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, void *d_windows_u32, void *d_hits_u32);
int ntc_bloom_insert_hashes_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void *d_h0_u64,
                                   uint64_t n);
int ntc_bloom_query_hashes_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k,
                                  const void *d_h0_u64, uint64_t n, void *d_flags_u8);
int ntc_bloom_popcount_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint64_t *pop);
int ntc_bloom_or_device(int32_t device, void *stream, void *d_dst, const void *d_src, uint64_t m_bits);
typedef struct {
    uint32_t k, n_hash, strand, reserved;   /* strand: 0 canonical, 1 forward, 2 reverse; reserved: 0 (a blocked filter's file: 512) */
    uint64_t m_bits, n_inserted;            /* n_inserted: the windows inserted so far (a count of insertions, not of distinct k-mers) */
} ntc_bloom_header;
int ntc_bloom_write(const char *path, const ntc_bloom_header *h, const void *filter_bytes);
int ntc_bloom_read(const char *path, ntc_bloom_header *h, void *filter_bytes, uint64_t cap_bytes);

/* COUNTING BLOOM FILTERS and SOLID k-mers (additive to ABI 6: eleven calls; NTC_ABI_VERSION and every other declaration are unchanged).  The other half
 * of ntCard's output: f1 and the f_i lines say how many distinct k-mers occur once, twice, ...; a downstream tool keeps the SOLID ones, seen at least c
 * times, in a filter it sizes from F0 - sum_{i<c} f_i.  Engine-less device tools like the Bloom calls above, with their input, their limits, their
 * errors and their walk (ntc_bloom_size serves both kinds: the positions it returns are counters here and bits there).
 *   The counters  caller-owned DEVICE memory: m unsigned 8-bit counters, counter loc = byte loc, m bytes rounded up to a multiple of 4, 4-byte aligned,
 *       zeroed by the caller before the first insert.  The bytes from m on (the padding) stay zero.  1 <= m < 2^40.  A k-mer's n_hash positions are the
 *       plain filter's: loc_i = h_i % m.
 *   Insert        every one of the n_hash counters += 1, saturating at 255; two positions of one k-mer that coincide (small m) give that counter two
 *       increments.  After any inserts, in any order, on any number of workgroups: counter[loc] = min(255, the increments aimed at loc).  There is NO
 *       conservative update (incrementing only the minimal counters): its result depends on the order of concurrent inserts.
 *   Count         of a k-mer: the minimum of its n_hash counters — never below its true number of occurrences capped at 255, above it only by collisions.
 *   ntc_cbloom_insert_device   increments for every window; *n_windows = the windows inserted (may be NULL).  A counter that a plain load finds at 255
 *       costs nothing; otherwise one 32-bit compare-and-swap loop on the containing dword, which adds 1 << 8 (loc % 4) and leaves at 255.
 *   ntc_cbloom_query_device    d_windows_u32[i] = the windows of sequence i, d_hits_u32[i] = those whose count is >= min_count (1 .. 255); DEVICE arrays of
 *       n_seqs uint32, zeroed by the call.
 *   ntc_cbloom_profile_device  the coverage profile: for n = offsets[n_seqs] - offsets[0], d_counts_u8[p] = the count of the window that STARTS at
 *       position p (byte offsets[0] + p of d_bases), 0 where none starts: the last k - 1 positions of a sequence, windows with a non-base, sequences
 *       shorter than k.  All n bytes are written (a DEVICE array of n bytes, any alignment, not zeroed by the caller).
 *   ntc_cbloom_insert_hashes_device / ntc_cbloom_query_hashes_device  the same arithmetic on n GIVEN h_0 values (DEVICE uint64); d_counts_u8[i] = the count.
 *   ntc_cbloom_threshold_device  writes the plain filter of m_bits = m in the reference's layout: the bit of position loc is set iff
 *       counter[loc] >= min_count, the padding behind m is zero.  Every k-mer seen >= min_count times has all its bits set; with min_count = 1 the image
 *       is what ntc_bloom_insert_device builds from the same input with the same n_hash.  d_filter: (m + 7) / 8 bytes rounded up to 4, every byte written.
 *   ntc_bloom_insert_solid_device  the second stage: walks the input again and sets, in a plain filter of its OWN m_bits and n_hash, every window whose
 *       count in a finished counting filter (d_counters, m, c_n_hash) is >= min_count; *n_windows = the windows that passed (may be NULL).
 *   ntc_cbloom_add_device      d_dst = min(255, d_dst + d_src) per counter: shards of one input, peers' filters.  The two arrays are distinct.
 *   ntc_cbloom_hist_device     hist_u64[v] = how many of the first m counters hold v (HOST array of 256).  NTC_ERR_STATE when a padding byte is not 0.
 *       (sum_{v>=c} hist[v] / m)^n_hash is the expected rate of a false "count >= c"; hist[255] the saturated counters.
 * A counting filter FILE: the 8 bytes "NTCCB1\0\0", ntc_bloom_header with m_bits = the number of counters, then the m counter bytes.
 * ntc_cbloom_write / ntc_cbloom_read behave as ntc_bloom_write / ntc_bloom_read do (".part" and rename; the size query with a NULL array). */
int ntc_cbloom_insert_device(int32_t device, void *stream, void *d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand,
                             const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, uint64_t *n_windows);
int ntc_cbloom_query_device(int32_t device, void *stream, const void *d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand,
                            const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t min_count, void *d_windows_u32, void *d_hits_u32);
int ntc_cbloom_profile_device(int32_t device, void *stream, const void *d_counters, uint64_t m, uint32_t n_hash, uint32_t k, uint32_t strand,
                              const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, void *d_counts_u8);
int ntc_cbloom_insert_hashes_device(int32_t device, void *stream, void *d_counters, uint64_t m, uint32_t n_hash, uint32_t k, const void *d_h0_u64,
                                    uint64_t n);
int ntc_cbloom_query_hashes_device(int32_t device, void *stream, const void *d_counters, uint64_t m, uint32_t n_hash, uint32_t k,
                                   const void *d_h0_u64, uint64_t n, void *d_counts_u8);
int ntc_cbloom_threshold_device(int32_t device, void *stream, const void *d_counters, uint64_t m, uint32_t min_count, void *d_filter);
int ntc_bloom_insert_solid_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, const void *d_counters, uint64_t m,
                                  uint32_t c_n_hash, uint32_t min_count, uint32_t k, uint32_t strand, const void *d_bases, const uint64_t *offsets,
                                  uint64_t n_seqs, uint64_t *n_windows);
int ntc_cbloom_add_device(int32_t device, void *stream, void *d_dst, const void *d_src, uint64_t m);
int ntc_cbloom_hist_device(int32_t device, void *stream, const void *d_counters, uint64_t m, uint64_t *hist_u64);
int ntc_cbloom_write(const char *path, const ntc_bloom_header *h, const void *counter_bytes);
int ntc_cbloom_read(const char *path, ntc_bloom_header *h, void *counter_bytes, uint64_t cap_bytes);

/* BLOCKED BLOOM FILTERS (additive to ABI 6: ten calls, one constant; NTC_ABI_VERSION and every other declaration are unchanged).  A second kind of filter
 * beside the plain one, not a change to it: all n_hash bits of a k-mer lie in ONE aligned block of NTC_BBLOOM_BLOCK_BITS = 512 bits, a 64-byte line
 * (Putze, Sanders, Singler 2007), so a build or a query fetches one random line per k-mer where the plain filter fetches n_hash.  The price is a somewhat
 * larger filter for the same false positive rate (about 2 % more bits at three hashes and 1 %) and a file the reference's tools do not read.  Input,
 * strands, streams, scratch and the walk are the plain calls'.
 *   The format    m_bits bits, a multiple of 512 with 512 <= m_bits < 2^40; n_blocks = m_bits / 512.  For a window value h_0:
 *       block     b = h_0 mod n_blocks (exact for every 64-bit h_0)
 *       position  p_i = (g >> (55 - 9 * (i mod 4))) & 511 for i = 0 .. n_hash - 1, g = the multi-hash of nthash.hpp:381-390 with index 1 + i / 4
 *                 (g = t ^ t >> 27, t = h_0 * ((1 + i / 4) ^ k * multiSeed)): four 9-bit fields from the TOP 36 bits of each multi-hash value, highest
 *                 first.  The top bits, because the low bits of g depend only on the low bits of h_0 — which chose the block when n_blocks is a power of two.
 *       bit       loc_i = 512 * b + p_i by the plain filter's rule, bit 7 - loc % 8 of byte loc / 8.  Positions of one k-mer that coincide set one bit.
 *       The image is therefore an ORDINARY BIT IMAGE of m_bits bits: ntc_bloom_popcount_device and ntc_bloom_or_device serve a blocked filter unchanged,
 *       and the filter's memory is the plain filter's (m_bits / 8 bytes, 4-byte aligned, zeroed by the caller; there is no padding).
 *       For n_hash > 8 the reference's multi-hash values are linearly related (their multipliers differ in four low bits) and the realised false positive
 *       rate can lie above the formula's — up to 14 % in single runs at n_hash = 32.  A property of the multi-hash, not repaired here.
 *   ntc_bbloom_fpr   pure host: *fpr = sum_j Poisson(j; l) * (1 - (1 - 1/512)^(j * n_hash))^n_hash, l = 512 * n_distinct / m_bits — the load of a block is
 *       Poisson, and a block with j k-mers answers a foreign k-mer like a 512-bit filter.  Summed until the tail left is below 1e-15 of the sum.
 *       n_distinct may be 0 (*fpr = 0).  NTC_ERR_ARG for an m_bits that is no legal blocked size, n_hash outside 1 .. 32, a NULL fpr.
 *   ntc_bbloom_size  pure host: the smallest multiple of 512 whose ntc_bbloom_fpr is <= fpr, by bisection over n_blocks.  NTC_ERR_ARG where ntc_bloom_size
 *       is: n_distinct == 0, n_hash outside 1 .. 32, fpr outside (0, 1), a NULL m_bits or a result of 2^40 bits or more.
 *   ntc_bbloom_insert_device / ntc_bbloom_query_device / ntc_bbloom_insert_hashes_device / ntc_bbloom_query_hashes_device
 *       the plain calls' signatures and results on a blocked filter.  An insert loads the dword first and issues one atomic OR per dword that still
 *       lacks a bit: bits of one k-mer that share a dword go in one atomic.  A query leaves at the first clear bit.
 *   ntc_bbloom_hist_device  hist_u64[v] = the blocks that hold v set bits, v = 0 .. 512 (HOST array of 513), exact integers.
 *       sum_v hist[v] * (v / 512)^n_hash / n_blocks is the realised false positive rate: the chance that a k-mer never inserted finds its bits set.
 *   ntc_bbloom_insert_solid_device  ntc_bloom_insert_solid_device with a blocked destination: sets every window whose count in a finished counting
 *       filter (d_counters, m, c_n_hash) is >= min_count; *n_windows = the windows that passed (may be NULL).
 * Before the device is touched, NTC_ERR_ARG for what the plain calls refuse, and for an m_bits that is no multiple of 512 or outside 512 .. 2^40 - 512.
 * A blocked filter FILE: the 8 bytes "NTCBB1\0\0", ntc_bloom_header with reserved = the block size in bits (512 is the only accepted value), then the
 * m_bits / 8 bytes.  ntc_bbloom_write / ntc_bbloom_read behave as ntc_bloom_write / ntc_bloom_read do (".part" and rename; the size query with a NULL
 * array; the length checked against the header). */
#define NTC_BBLOOM_BLOCK_BITS 512u
int ntc_bbloom_fpr(uint64_t n_distinct, uint64_t m_bits, uint32_t n_hash, double *fpr);
int ntc_bbloom_size(uint64_t n_distinct, uint32_t n_hash, double fpr, uint64_t *m_bits);
int ntc_bbloom_insert_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand,
                             const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, uint64_t *n_windows);
int ntc_bbloom_query_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, uint32_t strand,
                            const void *d_bases, const uint64_t *offsets, uint64_t n_seqs, void *d_windows_u32, void *d_hits_u32);
int ntc_bbloom_insert_hashes_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k, const void *d_h0_u64,
                                    uint64_t n);
int ntc_bbloom_query_hashes_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint32_t n_hash, uint32_t k,
                                   const void *d_h0_u64, uint64_t n, void *d_flags_u8);
int ntc_bbloom_hist_device(int32_t device, void *stream, const void *d_filter, uint64_t m_bits, uint64_t *hist_u64);
int ntc_bbloom_insert_solid_device(int32_t device, void *stream, void *d_filter, uint64_t m_bits, uint32_t n_hash, const void *d_counters, uint64_t m,
                                   uint32_t c_n_hash, uint32_t min_count, uint32_t k, uint32_t strand, const void *d_bases, const uint64_t *offsets,
                                   uint64_t n_seqs, uint64_t *n_windows);
int ntc_bbloom_write(const char *path, const ntc_bloom_header *h, const void *filter_bytes);
int ntc_bbloom_read(const char *path, ntc_bloom_header *h, void *filter_bytes, uint64_t cap_bytes);

int ntc_sync(ntc_engine *e); /* wait for all submitted work */

/* Apply the pending hit log to the device sketch (asynchronous on the engine's stream).  After it the
 * device counters are the reference's t_Counter state for everything submitted so far (ntcard.cpp:142-143). */
int ntc_flush(ntc_engine *e);

/* End of stream: the state compEst/outDefault consume.
 * t_counter_out: HOST uint16_t [n_k][2][1<<r_bits] (== the reference's t_Counter) or NULL
 * p_hist_out:    HOST uint32_t [n_k][2][65536], p[s][v] = #buckets of sample s whose counter == v
 *                (ntcard.cpp:240-247) or NULL
 * f1_out:        HOST uint64_t [n_k] (totalKmers, ntcard.cpp:464-466) or NULL
 * May be called repeatedly; does not clear the sketch.                                          */
int ntc_finish(ntc_engine *e, uint16_t *t_counter_out, uint32_t *p_hist_out, uint64_t *f1_out);

/* compEst's first loop (ntcard.cpp:240-247) over an arbitrary run of DEVICE counters: for each of the n uint32
 * counters, ++d_hist_u32[counter & 0xffff] (the histogram is accumulated, not zeroed).  Asynchronous on `stream`.
 * Used by the multi-GPU merge: after a reduce-scatter every rank histograms its own slice of the summed sketch and
 * only the 256 KiB histograms travel to rank 0 (ntcard_amd/parallel.py).                                      */
int ntc_value_hist_device(int32_t device, void *stream, const void *d_counters_u32, uint64_t n, void *d_hist_u32);

/* The device steps of the multi-GPU merge for a caller that moves the counter slices itself — one process per GPU, the slices travel in one RCCL
 * all-to-all (ntcard_amd/parallel.py) — the same kernels ntc_merge_devices runs between its peer copies.  t_Counter wraps at 16 bits
 * (ntcard.cpp:142-143,439), so only the low halves travel:
 *   ntc_narrow_u16_device      d_out_u16[i] = d_counters_u32[i] mod 2^16, i < n
 *   ntc_sum_slices_u16_device  slice 0 += slices 1 .. n_slices - 1 (wrapping 16-bit adds); slice r = d_slices_u16[r * stride, r * stride + len)
 *   ntc_value_hist_u16_device  ++d_hist_u32[d_counters_u16[i]], i < n (compEst's first loop, ntcard.cpp:240-247, over a summed slice)
 * All asynchronous on `stream`; buffers 16-byte aligned, stride a multiple of 8 elements.                                              */
int ntc_narrow_u16_device(int32_t device, void *stream, const void *d_counters_u32, uint64_t n, void *d_out_u16);
int ntc_sum_slices_u16_device(int32_t device, void *stream, void *d_slices_u16, uint64_t stride, uint32_t n_slices, uint64_t len);
int ntc_value_hist_u16_device(int32_t device, void *stream, const void *d_counters_u16, uint64_t n, void *d_hist_u32);

/* The multi-GPU merge that ships HITS instead of counters (ABI 6) — for runs whose sampled k-mers are fewer than their counters' bytes, i.e. the reference's
 * sBits = 11 branch (inputs >= 50 GB, ntcard.cpp:427-431; BASELINE config 3: 125 M reads per GPU log 14.5 M keys = 58 MB where the 16-bit slice exchange
 * moves 448 MiB per rank).  Counter range p of n_parts ("owner" p) = the counters [p * C / n_parts, (p + 1) * C / n_parts), C = n_k * 2 * 2^r_bits.
 *   ntc_log_export_device   the PENDING hit log (everything counted since the last sketch update: the operands of ntComp's `++t_Counter[...]`,
 *                           ntcard.cpp:142-143) split by owner.  counts_out[p] (host) = the keys of owner p; with d_keys_u32 != NULL they are written, 32-bit
 *                           counter indices in arbitrary order, to d_keys_u32[part_offset[p] .. part_offset[p] + counts_out[p]) (part_offset: host, n_parts
 *                           entries; call once with d_keys_u32 == NULL to learn the counts).  Synchronises the engine's stream.  The log stays pending.
 *                           NTC_ERR_STATE when the sketch already holds counts (an update ran since the last reset, or a kernel incremented it directly) or
 *                           the engine has no hit log: the caller then merges counters (ntc_narrow_u16_device ...), which is always possible.
 *   ntc_log_replace_device  drops the pending log and makes the n_keys counter indices at d_keys_u32 (device) the pending log instead: the next
 *                           ntc_flush / ntc_finish counts exactly them.  An owner calls it with the keys it received for its range (its own included):
 *                           its sketch then holds the SUMMED counters of its range (and zeros elsewhere), to be histogrammed with ntc_value_hist_device.
 * ntcard_amd/parallel.py (merge_owner) runs the exchange between the two calls with one RCCL all-to-all.                                              */
int ntc_log_export_device(ntc_engine *e, uint32_t n_parts, void *d_keys_u32, const uint64_t *part_offset, uint64_t *counts_out);
int ntc_log_replace_device(ntc_engine *e, const void *d_keys_u32, uint64_t n_keys);

/* Sketch load / merge: adds a t_Counter image dumped by ntc_finish (same k list, r_bits;
 * uint16 [n_k][2][1<<r_bits]) and its F1 values (may be NULL) into this engine.  Counting is a commutative sum
 * mod 2^16 (ntcard.cpp:142-143), so runs split across processes, nodes or days merge exactly.               */
int ntc_merge_counters(ntc_engine *e, const uint16_t *t_counter, const uint64_t *f1);

/* Multi-GPU merge inside ONE host process: engines[0..n) are engines with the same configuration,
 * normally one per GPU of the node, each fed with its own share of the reads.  After the call engine 0 holds the
 * element-wise SUM of all sketches and F1 values (MAX of the registers for nthll engines) — the state the
 * reference's threads build in their one shared t_Counter / totalKmers (ntcard.cpp:142-143,464-466; nthll.cpp:
 * 238-243) — and the other engines are reset to zero.  t_Counter wraps at 16 bits (ntcard.cpp:439), so the counters travel
 * as their low halves: every engine narrows its sketch to uint16, slice j of every engine is copied to engine j's device (all
 * N x (N-1) peer copies in flight together, one per point-to-point xGMI link; hipMemcpyPeerAsync, staged by the runtime when two
 * devices have no peer access), engine j adds its N slices with wrapping 16-bit adds, the summed slices are gathered on engine
 * 0's device and widened into its sketch — the same exchange bench.py runs between processes with RCCL's all-to-all.  Engine 0's
 * counters afterwards hold their value mod 2^16 (all t_Counter ever held) and it may keep counting; F1 and nthll registers are
 * merged at full width.  No communicator, no library beyond HIP.                                                        */
int ntc_merge_devices(ntc_engine *const *engines, int32_t n_engines);

/* Device pointers of the live sketch / F1 (for a host framework's collective); flushes the hit log first */
int ntc_device_state(ntc_engine *e, void **d_sketch_u32, uint64_t *n_counters, void **d_f1_u64);

/* Validation kernel (K1d): canonical hash of every window of ONE k for a device-resident slot
 * batch.  d_hash_out: DEVICE uint64_t [n_reads][max_win], d_count_out: DEVICE uint32_t [n_reads].
 * The hashes of read i are written compacted, in window order, and d_count_out[i] says how many
 * there are (== that read's F1 share; may exceed max_win, then only max_win are stored), mirroring ntHashIterator
 * (ntHashIterator.hpp:59-86) / stHashIterator when gap != 0.                                     */
int ntc_hash_dump_device(int32_t device, void *stream, const void *d_slots, uint64_t n_reads,
                         uint32_t read_len, uint32_t stride, uint32_t k, uint32_t gap,
                         uint32_t max_win, void *d_hash_out, void *d_count_out);
/* The same dump produced by a validation build of the PRODUCTION kernel K1 (its filter lets every window through, so
 * every 64-bit value comes out of K1's closed-form resolve stage; spaced seeds included: ntcard.cpp:160-171,
 * stHashIterator.hpp:60-87, nthash.hpp:641-646).  ntc_hash_dump_device forwards here when gap != 0.  Synchronous. */
int ntc_hash_dump_k1_device(int32_t device, void *stream, const void *d_slots, uint64_t n_reads,
                            uint32_t read_len, uint32_t stride, uint32_t k, uint32_t gap,
                            uint32_t max_win, void *d_hash_out, void *d_count_out);
/* The same for a spaced seed given as a mask (ntc_create_seeded: k = strlen(seed)); a mask of '1's only dumps plain k-mers.
 * The arguments are checked before the device is touched. */
int ntc_hash_dump_seed_device(int32_t device, void *stream, const void *d_slots, uint64_t n_reads, uint32_t read_len,
                              uint32_t stride, const char *seed, uint32_t max_win, void *d_hash_out, void *d_count_out);

/* The same with a strand: 0 the canonical value (bit for bit ntc_hash_dump_seed_device), 1 the forward value fh / fs, 2 the reverse value rh / rs of every
 * window (NTC_FLAG_STRAND_*); anything else is NTC_ERR_ARG before the device is touched.  Strands 1 and 2 come out of the resolve stage of K1's one-strand form. */
int ntc_hash_dump_strand_device(int32_t device, void *stream, const void *d_slots, uint64_t n_reads, uint32_t read_len,
                                uint32_t stride, const char *seed, uint32_t strand, uint32_t max_win, void *d_hash_out,
                                void *d_count_out);

/* Synthetic workload generator (K0), bit-identical to oracle/orc_gen_reads; DESIGN.md
 * "Synthetic workloads".  Fills d_slots[n_reads*stride].                                         */
int ntc_gen_reads_device(int32_t device, void *stream, void *d_slots, uint64_t seed,
                         uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint32_t stride,
                         uint32_t dist, uint64_t genome_len);

/* the same reads (bit-identical bases) in the tiled layout of ntc_submit_tiled_device; fills ntc_tiled_bytes() bytes */
int ntc_gen_reads_tiled_device(int32_t device, void *stream, void *d_tiles, uint64_t seed, uint64_t first_read,
                               uint64_t n_reads, uint32_t read_len, uint32_t dist, uint64_t genome_len);

/* compEst (ntcard.cpp:249-274) from the value histogram of ONE k.  f_out has cov_max+1 doubles
 * (f_out[0] unused); only i <= cov_max is evaluated (identical values).          */
int ntc_estimate(const uint32_t *p_hist /* [2][65536] */, uint32_t r_bits, uint32_t s_bits,
                 uint32_t cov_max, double *F0_out, double *f_out);

/* outDefault body for one k (ntcard.cpp:283,291-294): writes "<prefix>_k<k>.hist" when path is
 * given verbatim.  Returns 0 or NTC_ERR_ARG if the file cannot be written.                      */
int ntc_write_hist(const char *path, uint64_t f1, double F0, const double *f, uint32_t cov_max);

/* ---- nthll: HyperLogLog-style F0 of the same ntHash stream ---------------------------
 * Replaces nthll.cpp's per-thread `uint8_t mVec[nBuck]`, its ntRead/ntComp (nthll.cpp:92-105: bucket = low
 * n_bits of the hash, value = leading zeros of the remaining bits, keep the max), the max-merge under
 * `omp critical` (nthll.cpp:238-243) and the estimate (nthll.cpp:247-254).  Reads are fed with
 * ntc_submit / ntc_submit_device exactly as for an ntcard engine.
 * ntc_hll_create: one plain k, canonical — what nthll counts; the one-k, flag-less case of ntc_hll_create_ex. */
int ntc_hll_create(uint32_t k, uint32_t n_bits /* nthll -b, default 16 */, int32_t device, void *stream,
                   ntc_engine **out);
/* An nthll engine with several planes, spaced seeds and a strand (additive to ABI 6).  Plane i — the i-th k or the i-th mask, in list order — is a
 * register file M_i[1 << n_bits] of its own.  The value of a window is the one an ntcard plane of that mask and strand counts (NTC_FLAG_STRAND_* and
 * ntc_create_seeded above): canonical rs < fs ? rs : fs, forward fs, reverse rs; a window counts (F1, registers) only when all k bytes are bases, those
 * under a '0' included.  Behind the value nthll.cpp:92-97 applies unchanged: bucket = the low n_bits bits, value = the leading zeros of the remaining
 * bits, skipped when those are all zero, keep the max.
 * Every argument is checked before a device is looked for; NTC_ERR_ARG with a message for: both strand flags, any other flag, both lists or neither, a
 * bad mask (the rules of ntc_create_seeded), more than NTC_MAX_K_LIST planes, a k outside 1 .. ntc_max_k(), n_bits outside 4 .. 24.
 * Every submit call works on such an engine: ntc_submit*, ntc_submit_device, the tiled submits (re-laid out on the device as row slots) and
 * ntc_submit_long_device (every sequence gathered whole); the general kernel K1 hashes a batch once per plane.  A mask whose tables leave no room in LDS
 * for a batch's slots makes the submit fail with a message, nothing counted, as for an ntcard engine.  ntc_reset zeroes every plane; ntc_merge_devices
 * folds every plane's registers by max and F1 by sum and refuses engines whose planes, masks, strand or n_bits differ. */
typedef struct {
    uint32_t n_k; const uint32_t *k;              /* a k list (plain k-mers), 1 .. NTC_MAX_K_LIST entries, each 1 .. ntc_max_k() — or */
    uint32_t n_seeds; const char *const *seeds;   /* masks with the syntax and rules of ntc_create_seeded; exactly one of the two is non-empty */
    uint32_t n_bits;                              /* nthll -b, 4 .. 24 */
    int32_t device; void *stream;
    uint32_t flags;                               /* 0 or NTC_FLAG_STRAND_FORWARD or NTC_FLAG_STRAND_REVERSE, each with or without NTC_FLAG_HPC; anything else: NTC_ERR_ARG */
} ntc_hll_config;
int ntc_hll_create_ex(const ntc_hll_config *cfg, ntc_engine **out);
/* regs_out: HOST uint8_t [n_planes][1<<n_bits] (a plane == tVec of nthll.cpp:212-243), or NULL; f1_out: uint64_t [n_planes], the k-mers hashed per
 * plane, or NULL.  One plane (ntc_hll_create): uint8_t [1<<n_bits] and one uint64_t. */
int ntc_hll_finish(ntc_engine *e, uint8_t *regs_out, uint64_t *f1_out);
/* nthll.cpp:247-254 on one plane's registers, alpha halved as the reference does for canonical hashes (nthll.cpp:248-249) */
int ntc_hll_estimate(const uint8_t *regs, uint32_t n_bits, double *est_out);
/* the same for an engine's strand: 0 canonical — bit for bit ntc_hll_estimate; 1 forward, 2 reverse — the alpha is NOT halved (the halving answers for the
 * canonical value being the minimum of two; a one-strand value is uniform), every other operation and its order as in nthll.cpp:247-254, no FMA
 * contraction; any other strand: NTC_ERR_ARG */
int ntc_hll_estimate_strand(const uint8_t *regs, uint32_t n_bits, uint32_t strand, double *est_out);

/* Timing of the hot kernel as measured with HIP events on the engine's stream (for bench.py's
 * roofline leg): accumulated milliseconds and launch count since create/reset.                  */
int ntc_kernel_time(ntc_engine *e, double *ms_total, uint64_t *launches);
/* same for the deferred sketch update (partition + count passes): milliseconds and number of applies */
int ntc_apply_time(ntc_engine *e, double *ms_total, uint64_t *applies);
/* same for the fix-up kernels K1f of the one-wave-per-tile kernel: a span of their own behind the hash kernels' — one per K1h launch, or with
 * NTC_FLAG_DEFER_REDO one over up to 8 batches — so this time is NOT part of ntc_kernel_time, with or without the flag */
int ntc_fixup_time(ntc_engine *e, double *ms_total);
/* device buffers, copy streams and events ntc_merge_devices has created for this engine so far: they are kept between merges, so the count
 * stops growing after the first merge of a given group of engines (diagnostic) */
int ntc_merge_allocations(ntc_engine *e, uint64_t *n);
int ntc_set_profiling(ntc_engine *e, int enable);
/* how ntComp's increment is currently carried out on the device: 0 = hit log + partitioned apply, 1 = direct atomics
 * (NTC_FLAG_DIRECT_ATOMICS, or chosen by the engine after an apply found mostly repeated counters); waits for the stream */
int ntc_update_mode(ntc_engine *e, uint32_t *mode_out);
/* K1 (the general kernel) is one template with many instantiations; this says which of them the library has launched and in which regimes (additive to
 * ABI 6; a diagnostic for the tests, like ntc_merge_allocations).  Process-wide, host only: it touches no device and needs none.  Row `row` of the table
 * of instantiations: its template arguments, the launches since the library was loaded, how many of them were in regime i —
 *   0 PREFETCH     ceil(64 stride / 1024) <= pref: the next wave-batch is prefetched into registers
 *   1 BLOCKING     ceil(64 stride / 1024) >  pref: blocking loads
 *   2 PARTIAL      n_slots % 64 != 0: the last wave-batch is staged by the byte loop
 *   3 META         a slot table (reads of unequal length)
 *   4 SMALL_BLOCK  waves per block % 4 != 0: the equal split of a workgroup's wave-batches
 *   5 IDLE         fewer wave-batches than waves: ceil(n_slots / 64) < grid x waves per block
 *   6 MULTI        at least two wave-batches per wave on average: ceil(n_slots / 64) >= 2 x grid x waves per block
 *   7 LOG          the launch had hit-log regions
 * — and the shape of the last launch.  Counts are exact under concurrent launches; the last_* words are each those of some recent launch.
 * NTC_ERR_ARG for a NULL out or row >= the table's rows: that is how a caller counts them. */
typedef struct {
    uint8_t multi, mode, pref, dump, tiled, one, sig, reserved;
    uint64_t launches;
    uint64_t regime[8];
    uint32_t last_grid, last_wpb, last_stride, reserved2;
    uint64_t last_n_slots;
} ntc_k1_variant_info;
int ntc_k1_variant_stats(uint32_t row, ntc_k1_variant_info *out);

#ifdef __cplusplus
}
#endif
#endif
