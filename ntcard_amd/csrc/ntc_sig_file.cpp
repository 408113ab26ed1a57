// ntc_sig_file.cpp — signatures on the host: the signature file format (include/ntcard_hip.h: ntc_signature_write, ntc_signature_read) and the merge walk
// over two sorted hash lists (ntc_signature_compare).  Plain host C++ over the C ABI's types: it reads files from outside the program, and builds — and can be
// checked — without the device compiler or the engine (DESIGN.md §4 "Signatures").
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/ntcard_hip.h"

int ntc_internal_fail(int code, const char* fmt, ...); // ntc_lifecycle.hip: sets ntc_last_error()

namespace {
const char kSigMagic[8] = {'N', 'T', 'C', 'S', 'I', 'G', '1', '\0'};
struct FileCloser {
	FILE* f;
	~FileCloser()
	{
		if (f) std::fclose(f);
	}
};
} // namespace

extern "C" {

int ntc_signature_compare(const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb, uint64_t* n_common)
{
	if (!n_common || (!a && na) || (!b && nb)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_compare: null argument");
	for (uint64_t i = 1; i < na; ++i)
		if (a[i - 1] >= a[i]) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_compare: the first list is not strictly ascending at entry %llu", (unsigned long long)i);
	for (uint64_t i = 1; i < nb; ++i)
		if (b[i - 1] >= b[i]) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_compare: the second list is not strictly ascending at entry %llu", (unsigned long long)i);
	uint64_t i = 0, j = 0, c = 0;
	while (i < na && j < nb) {
		if (a[i] < b[j])
			++i;
		else if (b[j] < a[i])
			++j;
		else
			++c, ++i, ++j;
	}
	*n_common = c;
	return 0;
}

int ntc_signature_write(const char* path, const ntc_sig_header* h, const uint64_t* hashes, const uint32_t* counts)
{
	if (!path || !h || ((!hashes || !counts) && h->n)) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: null argument");
	const size_t ml = strnlen(h->mask, NTC_SIG_MASK_MAX);
	if (ml == 0 || ml >= NTC_SIG_MASK_MAX || ml != h->k || h->strand > 2 || h->hpc > 1 || h->s_bits < 2 || h->s_bits > 24)
		return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: bad header (the mask has k characters, strand 0..2, hpc 0..1, s_bits 2..24)");
	for (size_t i = 0; i < ml; ++i)
		if (h->mask[i] != '0' && h->mask[i] != '1') return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: the mask holds a character that is neither '0' nor '1'");
	for (uint64_t i = 1; i < h->n; ++i)
		if (hashes[i - 1] >= hashes[i]) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: the hashes are not strictly ascending at entry %llu", (unsigned long long)i);
	FileCloser fc{std::fopen(path, "wb")};
	if (!fc.f) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: cannot write %s", path);
	const uint32_t head[6] = {h->k, h->gap, h->strand, h->hpc, h->s_bits, (uint32_t)ml};
	char mask[NTC_SIG_MASK_MAX + 8] = {0};
	std::memcpy(mask, h->mask, ml);
	const size_t padded = (ml + 7) & ~(size_t)7;
	bool ok = std::fwrite(kSigMagic, 1, 8, fc.f) == 8 && std::fwrite(head, 4, 6, fc.f) == 6 && std::fwrite(&h->n, 8, 1, fc.f) == 1 && std::fwrite(mask, 1, padded, fc.f) == padded;
	ok = ok && (h->n == 0 || (std::fwrite(hashes, 8, h->n, fc.f) == h->n && std::fwrite(counts, 4, h->n, fc.f) == h->n));
	FILE* f = fc.f;
	fc.f = nullptr;
	if (std::fclose(f) != 0 || !ok) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_write: cannot write %s", path);
	return 0;
}

int ntc_signature_read(const char* path, ntc_sig_header* h, uint64_t* hashes, uint32_t* counts, uint64_t cap)
{
	if (!path || !h) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: null argument");
	FileCloser fc{std::fopen(path, "rb")};
	if (!fc.f) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: cannot read %s", path);
	char magic[8];
	uint32_t head[6];
	uint64_t n = 0;
	if (std::fseek(fc.f, 0, SEEK_END) != 0) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: cannot read %s", path);
	const long file_len = std::ftell(fc.f);
	if (file_len < 0 || std::fseek(fc.f, 0, SEEK_SET) != 0) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: cannot read %s", path);
	if (std::fread(magic, 1, 8, fc.f) != 8 || std::memcmp(magic, kSigMagic, 8) != 0) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is not a signature file", path);
	if (std::fread(head, 4, 6, fc.f) != 6 || std::fread(&n, 8, 1, fc.f) != 1 || head[5] == 0 || head[5] >= NTC_SIG_MASK_MAX || head[5] != head[0] || head[2] > 2 || head[3] > 1)
		return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s: bad header", path);
	const size_t padded = ((size_t)head[5] + 7) & ~(size_t)7;
	const uint64_t body = (uint64_t)file_len - std::min<uint64_t>((uint64_t)file_len, 8 + 24 + 8 + padded);
	if (n > body / 12 || n * 12 != body) // (n comes from the file: it is checked against the file's length before anything is sized or sought by it)
		return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is cut short or holds more than its header says (%llu pairs, %llu bytes behind the header)", path, (unsigned long long)n, (unsigned long long)body);
	std::memset(h, 0, sizeof *h);
	h->k = head[0], h->gap = head[1], h->strand = head[2], h->hpc = head[3], h->s_bits = head[4], h->n = n;
	char mask[NTC_SIG_MASK_MAX + 8];
	if (std::fread(mask, 1, padded, fc.f) != padded) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is cut short", path);
	std::memcpy(h->mask, mask, head[5]);
	for (uint32_t i = 0; i < head[5]; ++i)
		if (h->mask[i] != '0' && h->mask[i] != '1') return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s: bad mask", path);
	if (!hashes && !counts) return 0;
	if (cap < n) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s holds %llu pairs, the arrays have room for %llu", path, (unsigned long long)n, (unsigned long long)cap);
	if (hashes) {
		if (n && std::fread(hashes, 8, n, fc.f) != n) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is cut short", path);
		for (uint64_t i = 1; i < n; ++i)
			if (hashes[i - 1] >= hashes[i]) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s: the hashes are not strictly ascending", path);
	} else if (std::fseek(fc.f, (long)(n * 8), SEEK_CUR) != 0) {
		return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is cut short", path);
	}
	if (counts && n && std::fread(counts, 4, n, fc.f) != n) return ntc_internal_fail(NTC_ERR_ARG, "ntc_signature_read: %s is cut short", path);
	return 0;
}

} // extern "C"
