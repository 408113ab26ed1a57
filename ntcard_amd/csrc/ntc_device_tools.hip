// ntc_device_tools.hip — the entry points that need no engine: read generators, hash dumps of the validation builds, and the kernels of the
// multi-GPU merge for a caller that moves the slices itself (ntc_engine.hpp)
#include "ntc_engine.hpp"

using namespace ntc_eng;

namespace {
// K1's validation build over a batch: mask empty = plain k-mers (the arguments are checked)
int dump_k1(int32_t device, void* stream, const void* d_slots, uint64_t n_reads, uint32_t read_len, uint32_t stride, uint32_t k, const std::string& mask,
            uint32_t max_win, void* d_hash_out, void* d_count_out, uint32_t strand = 0)
{
	if (n_reads == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	if (int rc = ensure_kernel_attrs(device)) return rc;
	hipStream_t st = (hipStream_t)stream;
	const uint32_t n_win = read_len >= k ? read_len - k + 1 : 1;
	std::vector<uint32_t> t1((size_t)ntc::t2_pairs(k) * 64);
	ntc::build_t2(k, t1.data(), mask.empty() ? nullptr : mask.c_str());
	ntc::strand_t2(k, t1.data(), strand);
	ntc::SeedPlan sp;
	if (!mask.empty()) ntc::build_seed_plan(mask, sp);
	ntc::strand_seed_plan(sp, strand);
	const std::vector<uint32_t>& gt = sp.blob;
	const bool gap = !mask.empty();
	const size_t vbytes = (size_t)n_reads * ((n_win + 31) / 32) * 4;
	DevBuf<void> d_t1, d_gt; // (scratch of this call: freed on every way out)
	DevBuf<uint64_t> d_full;
	DevBuf<uint32_t> d_valid;
	DevBuf<unsigned long long> d_f1;
	if (!d_t1.reserve(t1.size() * 4) || (gap && !d_gt.reserve(gt.size() * 4)) || !d_full.reserve((size_t)n_reads * n_win * 8) || !d_valid.reserve(vbytes) || !d_f1.reserve(8))
		return fail(NTC_ERR_MEMORY, "ntc_hash_dump_k1_device: device allocation failed");
	HIP_TRY(hipMemcpyAsync(d_t1, t1.data(), t1.size() * 4, hipMemcpyHostToDevice, st));
	if (gap) HIP_TRY(hipMemcpyAsync(d_gt, gt.data(), gt.size() * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_valid, 0, vbytes, st));
	HIP_TRY(hipMemsetAsync(d_f1, 0, 8, st));
	ntc::HfArgs a;
	std::memset(&a, 0, sizeof a);
	a.slots = (const unsigned char*)d_slots;
	a.n_slots = n_reads;
	a.stride = stride;
	a.read_len = read_len;
	a.r_bits = 27;
	a.s_bits = 7;
	a.n_k = 1;
	if (gap) set_seed_args(a, sp, d_gt);
	fill_hfk(a.ks[0], k, nullptr, d_f1, d_t1, 0, strand);
	a.dump = d_full;
	a.dump_valid = d_valid;
	a.dump_win = n_win;
	HfPlan hp;
	if (int rc = hf_plan(device, n_reads, stride, &k, 1, seed_lds(sp), hp)) return rc;
	HIP_TRY(ntc::launch_sketch_hf(a, hp.grid, hp.wpb, hp.smem, st));
	HIP_TRY(ntc::launch_compact_dump(d_full, d_valid, n_reads, n_win, max_win, (uint64_t*)d_hash_out, (uint32_t*)d_count_out, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

} // namespace

extern "C" {

uint64_t ntc_tiled_bytes(uint64_t n_reads, uint32_t read_len)
{
	const uint64_t n_tiles = (n_reads + ntc::kTileReads - 1) / ntc::kTileReads;
	return n_tiles * ((read_len + 15u) / 16u) * (uint64_t)ntc::kTileReads * 16u;
}

int ntc_gen_reads_tiled_device(int32_t device, void* stream, void* d_tiles, uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                               uint32_t dist, uint64_t genome_len)
{
	if (!d_tiles || ((uintptr_t)d_tiles & 15u) || read_len == 0) return fail(NTC_ERR_ARG, "ntc_gen_reads_tiled_device: bad layout");
	if (dist > 1) return fail(NTC_ERR_ARG, "ntc_gen_reads_tiled_device: dist must be 0 (uniform) or 1 (genome)");
	if (dist == 1 && genome_len < read_len) return fail(NTC_ERR_ARG, "ntc_gen_reads_tiled_device: genome shorter than a read");
	if (n_reads == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_gen_tiled((unsigned char*)d_tiles, seed, first_read, n_reads, read_len, dist, genome_len, (hipStream_t)stream));
	return 0;
}

int ntc_gen_reads_device(int32_t device, void* stream, void* d_slots, uint64_t seed, uint64_t first_read,
                         uint64_t n_reads, uint32_t read_len, uint32_t stride, uint32_t dist, uint64_t genome_len)
{
	if (!d_slots || (stride & 3u) || stride < read_len) return fail(NTC_ERR_ARG, "ntc_gen_reads_device: bad layout");
	if (dist > 1) return fail(NTC_ERR_ARG, "ntc_gen_reads_device: dist must be 0 (uniform) or 1 (genome)");
	if (dist == 1 && genome_len < read_len) return fail(NTC_ERR_ARG, "ntc_gen_reads_device: genome shorter than a read");
	if (n_reads == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_gen((unsigned char*)d_slots, seed, first_read, n_reads, read_len, stride, dist, genome_len,
	                        (hipStream_t)stream));
	return 0;
}

int ntc_value_hist_device(int32_t device, void* stream, const void* d_counters_u32, uint64_t n, void* d_hist_u32)
{
	if (!d_counters_u32 || !d_hist_u32) return fail(NTC_ERR_ARG, "ntc_value_hist_device: null buffer");
	if ((n & 3u) || ((uintptr_t)d_counters_u32 & 15u)) return fail(NTC_ERR_ARG, "ntc_value_hist_device: need n %% 4 == 0 and 16-byte aligned counters");
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_value_hist((const uint32_t*)d_counters_u32, n, (uint32_t*)d_hist_u32, (hipStream_t)stream));
	return 0;
}

// The three device steps of the multi-GPU merge for a caller that moves the slices itself (one process per GPU: RCCL all-to-all under
// torch.distributed, ntcard_amd/parallel.py) — the kernels ntc_merge_devices runs between its peer copies
int ntc_narrow_u16_device(int32_t device, void* stream, const void* d_counters_u32, uint64_t n, void* d_out_u16)
{
	if (!d_counters_u32 || !d_out_u16) return fail(NTC_ERR_ARG, "ntc_narrow_u16_device: null buffer");
	if (((uintptr_t)d_counters_u32 & 15u) || ((uintptr_t)d_out_u16 & 15u)) return fail(NTC_ERR_ARG, "ntc_narrow_u16_device: need 16-byte aligned buffers");
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_narrow_u16((const uint32_t*)d_counters_u32, (uint16_t*)d_out_u16, n, (hipStream_t)stream));
	return 0;
}

int ntc_sum_slices_u16_device(int32_t device, void* stream, void* d_slices_u16, uint64_t stride, uint32_t n_slices, uint64_t len)
{
	if (!d_slices_u16) return fail(NTC_ERR_ARG, "ntc_sum_slices_u16_device: null buffer");
	if (((uintptr_t)d_slices_u16 & 15u) || (stride & 7u) || len > stride) return fail(NTC_ERR_ARG, "ntc_sum_slices_u16_device: need 16-byte aligned slices, stride %% 8 == 0, len <= stride");
	if (n_slices <= 1 || len == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_sum_slices_u16((uint16_t*)d_slices_u16, stride, n_slices, len, (hipStream_t)stream));
	return 0;
}

int ntc_value_hist_u16_device(int32_t device, void* stream, const void* d_counters_u16, uint64_t n, void* d_hist_u32)
{
	if (!d_counters_u16 || !d_hist_u32) return fail(NTC_ERR_ARG, "ntc_value_hist_u16_device: null buffer");
	if ((uintptr_t)d_counters_u16 & 15u) return fail(NTC_ERR_ARG, "ntc_value_hist_u16_device: need 16-byte aligned counters");
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	HIP_TRY(ntc::launch_value_hist_u16((const uint16_t*)d_counters_u16, n, (uint32_t*)d_hist_u32, (hipStream_t)stream));
	return 0;
}

// homopolymer compression of one sequence (include/ntcard_hip.h: NTC_FLAG_HPC); in place when out == in: byte j is read before byte m <= j is written
int ntc_hpc_compress(const char* in, uint64_t n, char* out, uint64_t* n_out)
{
	if (!n_out || (n && (!in || !out))) return fail(NTC_ERR_ARG, "ntc_hpc_compress: null argument");
	const auto cls = [](unsigned char b) -> uint32_t {
		switch (b | 0x20u) {
		case 'a': return 0u;
		case 'c': return 1u;
		case 'g': return 2u;
		case 't':
		case 'u': return 3u;
		default: return 0xffu; // N, IUPAC, CR, control bytes: no class, never dropped
		}
	};
	uint64_t m = 0;
	uint32_t pc = 0xffu;
	for (uint64_t j = 0; j < n; ++j) {
		const char b = in[j];
		const uint32_t c = cls((unsigned char)b);
		if (!(c != 0xffu && c == pc)) out[m++] = b;
		pc = c;
	}
	*n_out = m;
	return 0;
}

int ntc_hpc_compress_device(int32_t device, void* stream, const void* d_in, const uint64_t* offsets, uint64_t n_seqs, void* d_out, uint64_t* offsets_out)
{
	if (!offsets || !offsets_out) return fail(NTC_ERR_ARG, "ntc_hpc_compress_device: null offsets");
	for (uint64_t i = 0; i < n_seqs; ++i)
		if (offsets[i + 1] < offsets[i]) return fail(NTC_ERR_ARG, "ntc_hpc_compress_device: offsets not monotone at sequence %llu", (unsigned long long)i);
	const uint64_t n = offsets[n_seqs] - offsets[0];
	if (n && (!d_in || !d_out)) return fail(NTC_ERR_ARG, "ntc_hpc_compress_device: null buffer");
	std::fill(offsets_out, offsets_out + n_seqs + 1, (uint64_t)0);
	if (n == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	hipStream_t st = (hipStream_t)stream;
	DevBuf<unsigned char> aux; // (scratch of this call: freed on every way out)
	if (!aux.reserve(ntc::hpc_aux_bytes(n, n_seqs))) return fail(NTC_ERR_MEMORY, "ntc_hpc_compress_device: cannot allocate %zu B of scratch on device", ntc::hpc_aux_bytes(n, n_seqs));
	HIP_TRY(ntc::launch_hpc_compact((const unsigned char*)d_in, offsets, n_seqs, (unsigned char*)d_out, aux.get(), st));
	HIP_TRY(hipMemcpyAsync(offsets_out, ntc::hpc_aux_offsets(aux.get(), n_seqs), (n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

int ntc_hash_dump_device(int32_t device, void* stream, const void* d_slots, uint64_t n_reads, uint32_t read_len,
                         uint32_t stride, uint32_t k, uint32_t gap, uint32_t max_win, void* d_hash_out,
                         void* d_count_out)
{
	if (!d_slots || !d_hash_out || !d_count_out) return fail(NTC_ERR_ARG, "ntc_hash_dump_device: null buffer");
	if (k < 1 || k > kMaxK) return fail(NTC_ERR_ARG, "ntc_hash_dump_device: k=%u outside 1..%u", k, kMaxK);
	if (gap != 0) // the simple kernel has no spaced-seed form: the production kernel's validation build does it
		return ntc_hash_dump_k1_device(device, stream, d_slots, n_reads, read_len, stride, k, gap, max_win, d_hash_out, d_count_out);
	if ((stride & 3u) || stride < read_len || ((uintptr_t)d_slots & 15u))
		return fail(NTC_ERR_ARG, "ntc_hash_dump_device: need 16-byte aligned slots, stride %% 4 == 0, stride >= read_len");
	if (n_reads == 0) return 0;
	HIP_TRY(hipSetDevice(device));
	unsigned grid = 0;
	size_t smem = 0;
	if (int rc = ensure_kernel_attrs(device)) return rc;
	if (int rc = hash_grid(device, n_reads, stride, grid, smem)) return rc;
	ntc::HashArgs a;
	std::memset(&a, 0, sizeof a);
	a.slots = (const unsigned char*)d_slots;
	a.n_slots = n_reads;
	a.stride = stride;
	a.read_len = read_len;
	a.k = k;
	a.r_bits = 27;
	a.s_bits = 7;
	a.max_win = max_win;
	a.dump = (uint64_t*)d_hash_out;
	a.dump_count = (uint32_t*)d_count_out;
	ntc::build_tables(k, a.tab);
	HIP_TRY(ntc::launch_hash(1, a, grid, smem, (hipStream_t)stream));
	return 0;
}

int ntc_hash_dump_k1_device(int32_t device, void* stream, const void* d_slots, uint64_t n_reads, uint32_t read_len,
                            uint32_t stride, uint32_t k, uint32_t gap, uint32_t max_win, void* d_hash_out, void* d_count_out)
{
	if (!d_slots || !d_hash_out || !d_count_out) return fail(NTC_ERR_ARG, "ntc_hash_dump_k1_device: null buffer");
	if (k < 1 || k > kMaxK) return fail(NTC_ERR_ARG, "ntc_hash_dump_k1_device: k=%u outside 1..%u", k, kMaxK);
	if (gap != 0 && (gap % 2 != k % 2 || gap >= k)) return fail(NTC_ERR_ARG, "ntc_hash_dump_k1_device: gap size and kmer must have the same modulus");
	if ((stride & 3u) || stride < read_len || ((uintptr_t)d_slots & 15u))
		return fail(NTC_ERR_ARG, "ntc_hash_dump_k1_device: need 16-byte aligned slots, stride %% 4 == 0, stride >= read_len");
	return dump_k1(device, stream, d_slots, n_reads, read_len, stride, k, gap ? ntc::gap_mask(k, gap) : std::string(), max_win, d_hash_out, d_count_out);
}

int ntc_hash_dump_seed_device(int32_t device, void* stream, const void* d_slots, uint64_t n_reads, uint32_t read_len,
                              uint32_t stride, const char* seed, uint32_t max_win, void* d_hash_out, void* d_count_out)
{
	if (!d_slots || !d_hash_out || !d_count_out || !seed) return fail(NTC_ERR_ARG, "ntc_hash_dump_seed_device: null argument");
	const size_t k = strnlen(seed, (size_t)kMaxK + 1);
	if (k < 1 || k > kMaxK) return fail(NTC_ERR_ARG, "ntc_hash_dump_seed_device: seed length outside 1..%u", kMaxK);
	for (size_t j = 0; j < k; ++j)
		if (seed[j] != '0' && seed[j] != '1') return fail(NTC_ERR_ARG, "ntc_hash_dump_seed_device: character %zu of the seed is neither '0' nor '1'", j + 1);
	const std::string mask(seed, k);
	if (mask.find('1') == std::string::npos) return fail(NTC_ERR_ARG, "ntc_hash_dump_seed_device: the seed has no '1'");
	if ((stride & 3u) || stride < read_len || ((uintptr_t)d_slots & 15u))
		return fail(NTC_ERR_ARG, "ntc_hash_dump_seed_device: need 16-byte aligned slots, stride %% 4 == 0, stride >= read_len");
	return dump_k1(device, stream, d_slots, n_reads, read_len, stride, (uint32_t)k, mask.find('0') == std::string::npos ? std::string() : mask, max_win,
	               d_hash_out, d_count_out);
}

int ntc_hash_dump_strand_device(int32_t device, void* stream, const void* d_slots, uint64_t n_reads, uint32_t read_len, uint32_t stride, const char* seed,
                                uint32_t strand, uint32_t max_win, void* d_hash_out, void* d_count_out)
{
	if (!d_slots || !d_hash_out || !d_count_out || !seed) return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: null argument");
	if (strand > 2) return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: strand %u is none of 0 (canonical), 1 (forward), 2 (reverse)", strand);
	const size_t k = strnlen(seed, (size_t)kMaxK + 1);
	if (k < 1 || k > kMaxK) return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: seed length outside 1..%u", kMaxK);
	for (size_t j = 0; j < k; ++j)
		if (seed[j] != '0' && seed[j] != '1') return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: character %zu of the seed is neither '0' nor '1'", j + 1);
	const std::string mask(seed, k);
	if (mask.find('1') == std::string::npos) return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: the seed has no '1'");
	if ((stride & 3u) || stride < read_len || ((uintptr_t)d_slots & 15u))
		return fail(NTC_ERR_ARG, "ntc_hash_dump_strand_device: need 16-byte aligned slots, stride %% 4 == 0, stride >= read_len");
	return dump_k1(device, stream, d_slots, n_reads, read_len, stride, (uint32_t)k, mask.find('0') == std::string::npos ? std::string() : mask, max_win,
	               d_hash_out, d_count_out, strand);
}

} // extern "C"
