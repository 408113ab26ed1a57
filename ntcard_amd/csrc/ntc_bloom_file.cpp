// ntc_bloom_file.cpp — the host side of the Bloom filters (include/ntcard_hip.h: ntc_bloom_size, ntc_bloom_write, ntc_bloom_read, ntc_cbloom_write,
// ntc_cbloom_read, ntc_bbloom_fpr, ntc_bbloom_size, ntc_bbloom_write, ntc_bbloom_read): the sizing formulas and the three filter files — a plain filter's
// bits, a counting filter's counters and a blocked filter's bits behind the same header.  Plain host C++ over the C ABI's types, like ntc_sig_file.cpp: it reads files from outside the program, and builds — and can be checked —
// without the device compiler or the engine (DESIGN.md §4 "Bloom filters", "Blocked filters").
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
const char kBlockedMagic[8] = {'N', 'T', 'C', 'B', 'B', '1', '\0', '\0'};
constexpr uint64_t kMaxBits = 1ull << 40;
struct FileCloser {
	FILE* f;
	~FileCloser()
	{
		if (f) std::fclose(f);
	}
};
// the three kinds of file: the magic, the bytes behind the header for a header's m_bits, what the header's `reserved` holds (0; a blocked filter: its
// block size in bits, of which m_bits is a multiple), and the names the messages use
struct Kind {
	const char* magic; // 8 bytes
	bool counters;     // m_bits counts bytes, not bits
	uint32_t reserved; // 0, or the block size
	const char* write_name;
	const char* read_name;
	const char* what;  // "filter" / "counting filter" / "blocked filter"
	const char* ranges; // the header fields' ranges, for the message of a refused write
	uint64_t body(uint64_t m) const { return counters ? m : (m + 7) / 8; }
};
const Kind kBits{kBloomMagic, false, 0, "ntc_bloom_write", "ntc_bloom_read", "filter", "reserved 0, m_bits 1..2^40-1"};
const Kind kCounters{kCountingMagic, true, 0, "ntc_cbloom_write", "ntc_cbloom_read", "counting filter", "reserved 0, m_bits 1..2^40-1"};
const Kind kBlocked{kBlockedMagic, false, NTC_BBLOOM_BLOCK_BITS, "ntc_bbloom_write", "ntc_bbloom_read", "blocked filter", "reserved 512, m_bits a multiple of 512 in 512..2^40-512"};
bool good_header(const Kind& kd, const ntc_bloom_header& h)
{
	if (kd.reserved && (h.m_bits < kd.reserved || h.m_bits % kd.reserved != 0)) return false;
	return h.k >= 1 && h.k <= ntc_max_k() && h.n_hash >= 1 && h.n_hash <= 32 && h.strand <= 2 && h.reserved == kd.reserved && h.m_bits >= 1 && h.m_bits < kMaxBits;
}
bool blocked_bits(uint64_t m_bits) { return m_bits >= NTC_BBLOOM_BLOCK_BITS && m_bits < kMaxBits && m_bits % NTC_BBLOOM_BLOCK_BITS == 0; }

// The false positive rate of a blocked filter of n_blocks blocks that holds n distinct k-mers: the load j of a block is Poisson(l), l = n / n_blocks, and
// a block with j k-mers answers a foreign k-mer like a 512-bit filter with j h insertions: sum_j P(j; l) (1 - (1 - 1/512)^(j h))^h.  The terms are
// summed from the mode outwards, each Poisson weight through lgamma, until the tail left on either side is below 1e-15 of the sum: beyond j the upper
// tail is at most P(j) (j + 1) / (j + 1 - l), below j the lower one at most P(j) l / (l - j) (the weights fall geometrically), and the factor is <= 1.
// From l = 2^17 on every term that matters has (1 - 1/512)^(j h) < 2^-64: the rate is 1.
double blocked_fpr(double n, double n_blocks, uint32_t n_hash)
{
	const double l = n / n_blocks, h = (double)n_hash;
	if (!(l > 0.0)) return 0.0;
	if (l >= 131072.0) return 1.0;
	const double ln_l = std::log(l), ln_keep = std::log1p(-1.0 / (double)NTC_BBLOOM_BLOCK_BITS);
	auto term = [&](double j, double* weight) {
		const double w = std::exp(j * ln_l - l - std::lgamma(j + 1.0));
		*weight = w;
		return w * std::pow(-std::expm1(j * h * ln_keep), h);
	};
	const double mode = std::floor(l);
	double sum = 0.0, w = 0.0;
	for (double j = mode;; j += 1.0) { // the mode and upwards
		sum += term(j, &w);
		if (j + 1.0 > l && (w == 0.0 || w * (j + 1.0) / (j + 1.0 - l) < 1e-15 * sum)) break;
	}
	for (double j = mode - 1.0; j >= 1.0; j -= 1.0) { // downwards (the term of j = 0 is 0)
		sum += term(j, &w);
		if (w * l / (l - j) < 1e-15 * sum) break;
	}
	return sum < 1.0 ? sum : 1.0;
}

int write_file(const Kind& kd, const char* path, const ntc_bloom_header* h, const void* filter_bytes)
{
	if (!path || !h || !filter_bytes) return ntc_internal_fail(NTC_ERR_ARG, "%s: null argument", kd.write_name);
	if (!good_header(kd, *h))
		return ntc_internal_fail(NTC_ERR_ARG, "%s: bad header (k 1..%u, n_hash 1..32, strand 0..2, %s)", kd.write_name, ntc_max_k(), kd.ranges);
	const uint64_t bytes = kd.body(h->m_bits);
	const std::string part = std::string(path) + ".part";
	FileCloser fc{std::fopen(part.c_str(), "wb")};
	if (!fc.f) return ntc_internal_fail(NTC_ERR_ARG, "%s: cannot write %s", kd.write_name, path);
	const uint32_t head[4] = {h->k, h->n_hash, h->strand, kd.reserved};
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
	if (!good_header(kd, x)) return ntc_internal_fail(NTC_ERR_ARG, "%s: %s: bad header", who, path);
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
int ntc_bbloom_write(const char* path, const ntc_bloom_header* h, const void* filter_bytes) { return write_file(kBlocked, path, h, filter_bytes); }
int ntc_bbloom_read(const char* path, ntc_bloom_header* h, void* filter_bytes, uint64_t cap_bytes) { return read_file(kBlocked, path, h, filter_bytes, cap_bytes); }

int ntc_bbloom_fpr(uint64_t n_distinct, uint64_t m_bits, uint32_t n_hash, double* fpr)
{
	if (!fpr) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_fpr: null fpr");
	if (!blocked_bits(m_bits)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_fpr: m_bits=%llu is no multiple of 512 in 512..2^40-512", (unsigned long long)m_bits);
	if (n_hash < 1 || n_hash > 32) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_fpr: n_hash=%u outside 1..32", n_hash);
	*fpr = blocked_fpr((double)n_distinct, (double)(m_bits / NTC_BBLOOM_BLOCK_BITS), n_hash);
	return 0;
}

int ntc_bbloom_size(uint64_t n_distinct, uint32_t n_hash, double fpr, uint64_t* m_bits)
{
	if (!m_bits) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_size: null m_bits");
	if (n_distinct == 0) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_size: n_distinct is 0");
	if (n_hash < 1 || n_hash > 32) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_size: n_hash=%u outside 1..32", n_hash);
	if (!(fpr > 0.0 && fpr < 1.0)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_size: fpr=%g outside (0, 1)", fpr);
	// the rate falls monotonically in n_blocks: bisect for the first n_blocks whose rate is <= fpr; lo's is above it (lo = 0: no filter), hi's is not
	uint64_t lo = 0, hi = kMaxBits / NTC_BBLOOM_BLOCK_BITS - 1;
	if (blocked_fpr((double)n_distinct, (double)hi, n_hash) > fpr)
		return ntc_internal_fail(NTC_ERR_ARG, "ntc_bbloom_size: %llu distinct k-mers at fpr %g need 2^40 bits or more", (unsigned long long)n_distinct, fpr);
	while (hi - lo > 1) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (blocked_fpr((double)n_distinct, (double)mid, n_hash) <= fpr)
			hi = mid;
		else
			lo = mid;
	}
	*m_bits = hi * NTC_BBLOOM_BLOCK_BITS;
	return 0;
}

} // extern "C"
