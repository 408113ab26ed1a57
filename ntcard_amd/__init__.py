"""ntcard_amd — MI355X (gfx950) engine for ntCard's ntHash -> sample -> count hot path.

Product code lives in ntcard_amd/csrc (HIP kernels + the C ABI of include/ntcard_hip.h); this
package is the thin Python mirror of that ABI used by tests and bench.py.
"""
from ._abi import ABI_SYMBOLS, LIB_PATH, NtcError  # noqa: F401
from .engine import (FLAG_ALWAYS_LOG, FLAG_PARTITION_ALWAYS, FLAG_LANE_KERNEL, FLAG_DIRECT_ATOMICS, FLAG_REQUIRE_TILED, FLAG_DEFER_REDO, FLAG_SIMPLE_KERNEL, FLAG_STRAND_FORWARD, FLAG_STRAND_REVERSE, FLAG_STRAND_TILED, FLAG_HPC, FLAG_SIGNATURE, Engine, HllEngine, hll_estimate, estimate, merge_devices, gen_reads_device, gen_reads_tiled_device, tiled_bytes, long_plan, hpc_compress, hpc_compress_device, tile_reads, tile_reads_ragged, hash_dump_device, hash_dump_seed_device, hash_dump_strand_device, s_bits_for_input, value_hist_device, narrow_u16_device, sum_slices_u16_device, value_hist_u16_device, signature_compare, signature_write, signature_read, signature_sort_device, signature_compare_device, signature_matrix_device,  # noqa: F401
                     signature_gather_device, GATHER_ROW_DTYPE, signature_union_device, signature_select_device, signature_hist_device, write_hist, k1_variant_stats, K1_REGIMES)
from .bloom import BBLOOM_BLOCK_BITS, BLOOM_BLOCK, BlockedBloomFilter, BloomFilter, CountingBloomFilter, bbloom_fpr, bbloom_size, bloom_size  # noqa: F401
