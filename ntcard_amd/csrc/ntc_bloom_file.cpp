// ntc_bloom_file.cpp — the host side of the Bloom filters (include/ntcard_hip.h: ntc_bloom_size, ntc_bloom_write, ntc_bloom_read, ntc_cbloom_write,
// ntc_cbloom_read): the sizing formula and the two filter files — a plain filter's bits and a counting filter's counters behind the same header.  Plain host C++ over the C ABI's types, like ntc_sig_file.cpp: it reads files from outside the program, and builds — and can be checked —
// without the device compiler or the engine (DESIGN.md §4 "Bloom filters").
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/ntcard_hip.h"

int ntc_internal_fail(int code, const char* fmt, ...); // ntc_lifecycle.hip: sets ntc_last_error()

namespace {
const char kBloomMagic[8] = {'N', 'T', 'C', 'B', 'F', '1', '\0', '\0'};
const char kCountingMagic[8] = {'N', 'T', 'C', 'C', 'B', '1', '\0', '\0'};
constexpr uint64_t kMaxBits = 1ull << 40;
struct FileCloser {
	FILE* f;
	~FileCloser()
	{
		if (f) std::fclose(f);
	}
};
bool good_header(const ntc_bloom_header& h)
{
	return h.k >= 1 && h.k <= ntc_max_k() && h.n_hash >= 1 && h.n_hash <= 32 && h.strand <= 2 && h.reserved == 0 && h.m_bits >= 1 && h.m_bits < kMaxBits;
}
// the two kinds of file: the magic, the bytes behind the header for a header's m_bits, and the names the messages use
struct Kind {
	const char* magic; // 8 bytes
	bool counters;     // m_bits counts bytes, not bits
	const char* write_name;
	const char* read_name;
	const char* what;  // "filter" / "counting filter"
	uint64_t body(uint64_t m) const { return counters ? m : (m + 7) / 8; }
};
const Kind kBits{kBloomMagic, false, "ntc_bloom_write", "ntc_bloom_read", "filter"};
const Kind kCounters{kCountingMagic, true, "ntc_cbloom_write", "ntc_cbloom_read", "counting filter"};

int write_file(const Kind& kd, const char* path, const ntc_bloom_header* h, const void* filter_bytes)
{
	if (!path || !h || !filter_bytes) return ntc_internal_fail(NTC_ERR_ARG, "%s: null argument", kd.write_name);
	if (!good_header(*h))
		return ntc_internal_fail(NTC_ERR_ARG, "%s: bad header (k 1..%u, n_hash 1..32, strand 0..2, reserved 0, m_bits 1..2^40-1)", kd.write_name, ntc_max_k());
	const uint64_t bytes = kd.body(h->m_bits);
	const std::string part = std::string(path) + ".part";
	FileCloser fc{std::fopen(part.c_str(), "wb")};
	if (!fc.f) return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot write %s", kd.write_name, path);
	const uint32_t head[4] = {h->k, h->n_hash, h->strand, 0};
	const uint64_t tail[2] = {h->m_bits, h->n_inserted};
	const bool ok = std::fwrite(kd.magic, 1, 8, fc.f) == 8 && std::fwrite(head, 4, 4, fc.f) == 4 && std::fwrite(tail, 8, 2, fc.f) == 2 &&
	                std::fwrite(filter_bytes, 1, bytes, fc.f) == bytes;
	FILE* f = fc.f;
	fc.f = nullptr;
	if (std::fclose(f) != 0 || !ok || std::rename(part.c_str(), path) != 0) {
		(void)std::remove(part.c_str());
		return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot write %s", kd.write_name, path);
	}
	return 0;
}

int read_file(const Kind& kd, const char* path, ntc_bloom_header* h, void* filter_bytes, uint64_t cap_bytes)
{
	const char* who = kd.read_name;
	if (!path || !h) return ntc_internal_fail(NTC_ERR_ARG, "%s: null argument", who);
	FileCloser fc{std::fopen(path, "rb")};
	if (!fc.f) return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot read %s", who, path);
	if (std::fseek(fc.f, 0, SEEK_END) != 0) return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot read %s", who, path);
	const long long file_len = (long long)ftello(fc.f);
	if (file_len < 0 || std::fseek(fc.f, 0, SEEK_SET) != 0) return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot read %s", who, path);
	char magic[8];
	uint32_t head[4];
	uint64_t tail[2];
	if (std::fread(magic, 1, 8, fc.f) != 8 || std::memcmp(magic, kd.magic, 8) != 0) return ntc_internal_fail(NTC_ERR_ARG, "%s: %s is not a %s file", who, path, kd.what);
	if (std::fread(head, 4, 4, fc.f) != 4 || std::fread(tail, 8, 2, fc.f) != 2) return ntc_internal_fail(NTC_ERR_ARG, "%s: %s is cut short", who, path);
	ntc_bloom_header x;
	x.k = head[0], x.n_hash = head[1], x.strand = head[2], x.reserved = head[3], x.m_bits = tail[0], x.n_inserted = tail[1];
	if (!good_header(x)) return ntc_internal_fail(NTC_ERR_ARG, "%s: %s: bad header", who, path);
	const uint64_t bytes = kd.body(x.m_bits), body = (uint64_t)file_len - 40u; // (m_bits comes from the file: checked against the file's length before anything is read by it)
	if (body != bytes)
		return ntc_internal_fail(NTC_ERR_ARG, "%s: %s is cut short or holds more than its header says (%llu bytes of %s, %llu bytes behind the header)", who, path,
		                         (unsigned long long)bytes, kd.what, (unsigned long long)body);
	*h = x;
	if (!filter_bytes) return 0;
	if (cap_bytes < bytes)
		return ntc_internal_fail(NTC_ERR_ARG, "%s: %s holds %llu bytes of %s, the array has room for %llu", who, path, (unsigned long long)bytes, kd.what, (unsigned long long)cap_bytes);
	if (std::fread(filter_bytes, 1, bytes, fc.f) != bytes) return ntc_internal_fail(NTC_ERR_ARG, "%s: %s is cut short", who, path);
	return 0;
}
} // namespace

extern "C" {

int ntc_bloom_size(uint64_t n_distinct, uint32_t n_hash, double fpr, uint64_t* m_bits)
{
	if (!m_bits) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: null m_bits");
	if (n_distinct == 0) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: n_distinct is 0");
	if (n_hash < 1 || n_hash > 32) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: n_hash=%u outside 1..32", n_hash);
	if (!(fpr > 0.0 && fpr < 1.0)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: fpr=%g outside (0, 1)", fpr);
	// m = ceil(-n h / ln(1 - fpr^(1 / h))): the m at which (1 - e^(-h n / m))^h = fpr
	const double m = std::ceil(-(double)n_distinct * (double)n_hash / std::log(1.0 - std::pow(fpr, 1.0 / (double)n_hash)));
	if (!(m < (double)kMaxBits)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: %llu distinct k-mers at fpr %g need 2^40 bits or more", (unsigned long long)n_distinct, fpr);
	const uint64_t r = ((uint64_t)(m < 1.0 ? 1.0 : m) + 63u) & ~(uint64_t)63;
	if (r >= kMaxBits) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bloom_size: %llu distinct k-mers at fpr %g need 2^40 bits or more", (unsigned long long)n_distinct, fpr);
	*m_bits = r;
	return 0;
}

int ntc_bloom_write(const char* path, const ntc_bloom_header* h, const void* filter_bytes) { return write_file(kBits, path, h, filter_bytes); }
int ntc_bloom_read(const char* path, ntc_bloom_header* h, void* filter_bytes, uint64_t cap_bytes) { return read_file(kBits, path, h, filter_bytes, cap_bytes); }
int ntc_cbloom_write(const char* path, const ntc_bloom_header* h, const void* counter_bytes) { return write_file(kCounters, path, h, counter_bytes); }
int ntc_cbloom_read(const char* path, ntc_bloom_header* h, void* counter_bytes, uint64_t cap_bytes) { return read_file(kCounters, path, h, counter_bytes, cap_bytes); }

} // extern "C"
