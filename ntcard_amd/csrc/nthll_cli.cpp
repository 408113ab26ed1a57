// nthll_cli.cpp — drop-in `nthll` front end: HyperLogLog-style estimate of the
// number of distinct k-mers: canonical as in the reference, or of one strand (--strand), of plain k-mers (one line per k of -k K[,K...]) or
// under spaced seeds (--seed=MASK[,MASK...], one line per mask).  Mirrors nthll.cpp: options (:55-68,150-186), `@list`
// (:187-198), one worker per input file (:218-237), the same record splitters as ntcard except that
// any first line that is neither '>' nor '@' is taken as header-less SAM (:71-90), and the single
// result line on stdout (:258).  Hashing, register update and max-merge run on the GPU through
// ntc_hll_create_ex / ntc_submit / ntc_hll_finish; the estimate is ntc_hll_estimate_strand (nthll.cpp:247-254).
#include <getopt.h>

#include <atomic>
#include <thread>

#include "cli_common.hpp"

const char* const cli::kProgram = "nthll";

namespace {

using namespace cli;

void process_file(const std::string& path, ntc_engine* eng)
{
	LineReader in(path);
	std::string first;
	in.getline(first);
	const char c0 = first.empty() ? '\0' : first[0];
	bool sam_has_header = true;
	unsigned type = sniff(first, sam_has_header);
	if (c0 != '>' && c0 != '@') { // nthll.cpp:87-89: no field check, always header-less SAM
		type = 2;
		sam_has_header = false;
	}
	Batcher batch(eng);
	if (type == 0)
		parse_fastq_blocks(in, eng);
	else if (type == 1)
		parse_fasta_blocks(in, eng, batch);
	else
		parse_sam_blocks(in, eng, batch, first, sam_has_header);
	batch.flush();
}

} // namespace

int main(int argc, char** argv)
{
	static const char shortopts[] = "t:k:b:s:hc";
	enum { OPT_HELP = 1, OPT_VERSION, OPT_SEED, OPT_STRAND, OPT_HPC };
	static const struct option longopts[] = { { "threads", required_argument, nullptr, 't' },
		                                      { "kmer", required_argument, nullptr, 'k' },
		                                      { "bit", required_argument, nullptr, 'b' },
		                                      { "sit", required_argument, nullptr, 's' },
		                                      { "hash", required_argument, nullptr, 'h' },
		                                      { "help", no_argument, nullptr, OPT_HELP },
		                                      { "version", no_argument, nullptr, OPT_VERSION },
		                                      { "seed", required_argument, nullptr, OPT_SEED },
		                                      { "strand", required_argument, nullptr, OPT_STRAND },
		                                      { "hpc", no_argument, nullptr, OPT_HPC },
		                                      { nullptr, 0, nullptr, 0 } };
	unsigned threads = 1, n_bits = 16, s_unused = 22;
	std::vector<uint32_t> klist;    // -k K[,K...] (none given: 64)
	std::vector<std::string> seeds; // --seed: masks of '0' / '1' (include/ntcard_hip.h: ntc_hll_create_ex)
	uint32_t strand = 0;            // --strand: 0 canonical, 1 forward, 2 reverse
	bool hpc = false;               // --hpc: NTC_FLAG_HPC
	bool die = false;
	for (int c; (c = getopt_long(argc, argv, shortopts, longopts, nullptr)) != -1;) {
		bool clean = true;
		switch (c) {
		case '?': die = true; break;
		case 't': clean = parse_value(optarg, threads); break;
		case 'b': clean = parse_value(optarg, n_bits); break;
		case 's': clean = parse_value(optarg, s_unused); break;
		case 'k': {
			klist.clear();
			const std::string arg(optarg);
			for (size_t b = 0; clean && b <= arg.size();) {
				const size_t e = arg.find(',', b);
				unsigned v = 0;
				clean = parse_value(arg.substr(b, e == std::string::npos ? std::string::npos : e - b).c_str(), v);
				klist.push_back(v);
				if (e == std::string::npos) break;
				b = e + 1;
			}
			break;
		}
		case OPT_SEED: {
			const std::string arg(optarg);
			for (size_t b = 0; b <= arg.size();) {
				const size_t e = arg.find(',', b);
				seeds.push_back(arg.substr(b, e == std::string::npos ? std::string::npos : e - b));
				if (e == std::string::npos) break;
				b = e + 1;
			}
			break;
		}
		case OPT_STRAND: {
			const std::string arg(optarg);
			if (arg == "canonical")
				strand = 0;
			else if (arg == "forward")
				strand = 1;
			else if (arg == "reverse")
				strand = 2;
			else {
				std::cerr << kProgram << ": --strand: `" << arg << "' is none of canonical, forward, reverse\n";
				return EXIT_FAILURE;
			}
			break;
		}
		case OPT_HPC: hpc = true; break;
		case 'c': break; // canonical hashing is always on (nthll.cpp:51,167-169)
		case OPT_HELP:
			std::cerr << "Usage: nthll [OPTION]... FILE(S)...\n"
			          << "Estimates the number of distinct k-mers (F0) in FILE(S) on an AMD MI355X.\n\n"
			          << "  -t, --threads=N\tparser threads [1]\n  -k, --kmer=N[,N...]\tk-mer length(s), one result line each [64]\n"
			          << "  -b, --bit=N\tlog2 of the number of registers [16]\n"
			          << "      --seed=MASK[,MASK...]\tspaced seeds instead of -k: strings of 0 (don't care) and 1 (counted), one result line each\n"
			          << "      --strand=canonical|forward|reverse\twhich value of a k-mer is hashed [canonical]\n"
			          << "      --hpc\thash homopolymer-compressed k-mers: every run of one base is collapsed to its first letter before the k-mers are taken\n"
			          << "      --help\tdisplay this help and exit\n      --version\toutput version information and exit\n";
			return EXIT_SUCCESS;
		case OPT_VERSION:
			std::cerr << "nthll 1.0.0 \nMI355X (gfx950) engine, C ABI version " << ntc_abi_version() << "\n";
			return EXIT_SUCCESS;
		default: break;
		}
		if (optarg != nullptr && !clean) {
			std::cerr << kProgram << ": invalid option: `-" << (char)c << optarg << "'\n";
			return EXIT_FAILURE;
		}
	}
	if (argc - optind < 1) {
		std::cerr << kProgram << ": missing arguments\n";
		die = true;
	}
	if (die) {
		std::cerr << "Try `" << kProgram << " --help' for more information.\n";
		return EXIT_FAILURE;
	}
	// every argument error is reported before a device is touched
	if (!seeds.empty() && !klist.empty()) {
		std::cerr << kProgram << ": --seed cannot be combined with -k\n";
		return EXIT_FAILURE;
	}
	for (const std::string& m : seeds) {
		if (m.empty() || m.find_first_not_of("01") != std::string::npos || m.find('1') == std::string::npos) {
			std::cerr << kProgram << ": --seed: `" << m << "' is not a mask of 0 and 1 with at least one 1\n";
			return EXIT_FAILURE;
		}
		if (m.size() > ntc_max_k()) {
			std::cerr << kProgram << ": --seed: a mask of " << m.size() << " positions is longer than the " << ntc_max_k() << " this GPU engine supports\n";
			return EXIT_FAILURE;
		}
	}
	if (seeds.empty() && klist.empty()) klist.push_back(64);
	if (std::max(seeds.size(), klist.size()) > NTC_MAX_K_LIST) {
		std::cerr << kProgram << ": at most " << NTC_MAX_K_LIST << (seeds.empty() ? " values of k" : " seeds") << " per run\n";
		return EXIT_FAILURE;
	}
	for (const uint32_t k : klist)
		if (k < 1 || k > ntc_max_k()) { // engine limit the reference does not have (README "Limits")
			std::cerr << kProgram << ": k=" << k << " is outside the range 1.." << ntc_max_k() << " this GPU engine supports\n";
			return EXIT_FAILURE;
		}
	std::vector<std::string> files;
	for (int i = optind; i < argc; ++i) {
		std::string f(argv[i]);
		if (!f.empty() && f[0] == '@') {
			LineReader list(f.substr(1));
			std::string name;
			while (list.getline(name))
				files.push_back(name);
		} else {
			files.push_back(f);
		}
	}
	int device = 0;
	if (const char* dev = std::getenv("NTCARD_DEVICE")) device = std::atoi(dev);
	ntc_hll_config cfg;
	std::memset(&cfg, 0, sizeof cfg);
	std::vector<const char*> seed_ptrs;
	if (!seeds.empty()) {
		for (const auto& m : seeds)
			seed_ptrs.push_back(m.c_str());
		cfg.n_seeds = (uint32_t)seed_ptrs.size();
		cfg.seeds = seed_ptrs.data();
	} else {
		cfg.n_k = (uint32_t)klist.size();
		cfg.k = klist.data();
	}
	cfg.n_bits = n_bits;
	cfg.device = device;
	cfg.flags = (strand == 1 ? NTC_FLAG_STRAND_FORWARD : strand == 2 ? NTC_FLAG_STRAND_REVERSE : 0u) | (hpc ? NTC_FLAG_HPC : 0u);
	ntc_engine* eng = nullptr;
	if (ntc_hll_create_ex(&cfg, &eng) != 0) die_engine();
	std::atomic<size_t> next(0);
	auto worker = [&]() {
		for (size_t i; (i = next.fetch_add(1)) < files.size();)
			process_file(files[files.size() - i - 1], eng); // nthll.cpp:225-226 walks the list backwards
	};
	std::vector<std::thread> pool;
	cli::g_file_helpers = std::max<unsigned>(1, (threads ? threads : 1) / (unsigned)std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, files.size())));
	for (unsigned t = 1; t < (threads ? threads : 1) && t < files.size(); ++t)
		pool.emplace_back(worker);
	worker();
	for (auto& th : pool)
		th.join();
	const size_t n_planes = std::max(seeds.size(), klist.size());
	std::vector<uint8_t> regs(n_planes << n_bits);
	if (ntc_hll_finish(eng, regs.data(), nullptr) != 0) die_engine();
	ntc_destroy(eng);
	for (size_t i = 0; i < n_planes; ++i) { // one line per plane, in list order
		double est = 0;
		if (ntc_hll_estimate_strand(regs.data() + (i << n_bits), n_bits, strand, &est) != 0) die_engine();
		std::cout << "F0, Exp# of distnt kmers(";
		if (seeds.empty())
			std::cout << "k=" << klist[i];
		else
			std::cout << "seed=" << seeds[i];
		std::cout << "): " << (unsigned long long)est << "\n";
	}
	return 0;
}
