// ntsig_cli.cpp — `ntsig`: signature files (`ntcard --signature`, include/ntcard_hip.h: ntc_signature_write) from the command line.
//   ntsig info F.sig            the header: how the file was counted, and how many values it holds
//   ntsig compare A.sig B.sig   |A n B|, Jaccard and both containments — refused when the headers differ in anything but n
// Host code over the library's reader and ntc_signature_compare; needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ntcard_hip.h"

namespace {

const char* const kStrand[3] = {"canonical", "forward", "reverse"};

struct Sig {
	ntc_sig_header h;
	std::vector<uint64_t> hashes;
	std::vector<uint32_t> counts;
};

bool load(const char* path, Sig& s, bool pairs)
{
	if (ntc_signature_read(path, &s.h, nullptr, nullptr, 0) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return false;
	}
	if (!pairs) return true;
	s.hashes.resize(s.h.n);
	s.counts.resize(s.h.n);
	uint64_t dummy_h = 0;
	uint32_t dummy_c = 0;
	if (ntc_signature_read(path, &s.h, s.h.n ? s.hashes.data() : &dummy_h, s.h.n ? s.counts.data() : &dummy_c, s.h.n) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return false;
	}
	return true;
}

void print_header(const char* path, const ntc_sig_header& h)
{
	std::printf("file\t%s\nk\t%u\nmask\t%s\ngap\t%u\nstrand\t%s\nhpc\t%u\nsBits\t%u\nn\t%llu\n", path, h.k, h.mask, h.gap, kStrand[h.strand], h.hpc, h.s_bits,
	            (unsigned long long)h.n);
}

int usage()
{
	std::fprintf(stderr, "Usage: ntsig info F.sig\n       ntsig compare A.sig B.sig\n");
	return EXIT_FAILURE;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 2) return usage();
	const std::string cmd(argv[1]);
	if (cmd == "info" && argc == 3) {
		Sig s;
		if (!load(argv[2], s, false)) return EXIT_FAILURE;
		print_header(argv[2], s.h);
		return EXIT_SUCCESS;
	}
	if (cmd == "compare" && argc == 4) {
		Sig a, b;
		if (!load(argv[2], a, true) || !load(argv[3], b, true)) return EXIT_FAILURE;
		const char* differs = nullptr;
		if (a.h.k != b.h.k) differs = "k";
		else if (std::strcmp(a.h.mask, b.h.mask) != 0) differs = "mask";
		else if (a.h.gap != b.h.gap) differs = "gap";
		else if (a.h.strand != b.h.strand) differs = "strand";
		else if (a.h.hpc != b.h.hpc) differs = "hpc";
		else if (a.h.s_bits != b.h.s_bits) differs = "sBits";
		if (differs) {
			std::fprintf(stderr, "ntsig: %s and %s were counted differently (%s differs): their values cannot be compared\n", argv[2], argv[3], differs);
			return EXIT_FAILURE;
		}
		uint64_t common = 0;
		if (ntc_signature_compare(a.hashes.data(), a.h.n, b.hashes.data(), b.h.n, &common) != 0) {
			std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
			return EXIT_FAILURE;
		}
		const uint64_t uni = a.h.n + b.h.n - common;
		std::printf("n_a\t%llu\nn_b\t%llu\ncommon\t%llu\n", (unsigned long long)a.h.n, (unsigned long long)b.h.n, (unsigned long long)common);
		std::printf("jaccard\t%.6f\ncontainment_a_in_b\t%.6f\ncontainment_b_in_a\t%.6f\n", uni ? (double)common / (double)uni : 0.0,
		            a.h.n ? (double)common / (double)a.h.n : 0.0, b.h.n ? (double)common / (double)b.h.n : 0.0);
		return EXIT_SUCCESS;
	}
	return usage();
}
