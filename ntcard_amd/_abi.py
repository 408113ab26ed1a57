"""ctypes binding of ntcard_amd/lib/libntcard_hip.so (include/ntcard_hip.h).

There is no CPU fallback: loading fails loudly if the library was not built, and every compute
entry point fails with NTC_ERR_DEVICE when no HIP device is present.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libntcard_hip.so")

# every symbol include/ntcard_hip.h declares
ABI_SYMBOLS = [
    "ntc_abi_version", "ntc_max_k", "ntc_last_error", "ntc_create", "ntc_destroy", "ntc_reset",
    "ntc_submit", "ntc_submit_spans", "ntc_submit_device", "ntc_sync", "ntc_finish", "ntc_device_state",
    "ntc_hash_dump_device", "ntc_hash_dump_k1_device", "ntc_gen_reads_device", "ntc_estimate", "ntc_write_hist",
    "ntc_kernel_time", "ntc_apply_time", "ntc_fixup_time", "ntc_merge_allocations", "ntc_update_mode", "ntc_flush", "ntc_set_profiling", "ntc_merge_counters", "ntc_merge_devices", "ntc_value_hist_device", "ntc_hll_create", "ntc_hll_finish", "ntc_hll_estimate", "ntc_hll_create_ex", "ntc_hll_estimate_strand",
    "ntc_submit_tiled_device", "ntc_submit_tiled_ragged_device", "ntc_submit_tiled_bins_device", "ntc_tiled_bytes", "ntc_gen_reads_tiled_device",
    "ntc_narrow_u16_device", "ntc_sum_slices_u16_device", "ntc_value_hist_u16_device",
    "ntc_log_export_device", "ntc_log_replace_device",
    "ntc_create_seeded", "ntc_hash_dump_seed_device", "ntc_hash_dump_strand_device",
    "ntc_submit_long_device", "ntc_long_plan", "ntc_long_stats", "ntc_long_time",
    "ntc_hpc_compress", "ntc_hpc_compress_device", "ntc_hpc_stats", "ntc_hpc_time",
    "ntc_signature_size", "ntc_signature", "ntc_signature_inject", "ntc_signature_inject_device", "ntc_signature_compare", "ntc_signature_stats",
    "ntc_signature_time", "ntc_signature_header", "ntc_signature_write", "ntc_signature_read",
    "ntc_signature_device", "ntc_signature_sort_time", "ntc_signature_sort_device", "ntc_signature_compare_device", "ntc_signature_matrix_device",
    "ntc_signature_gather_device",
    "ntc_signature_union_device", "ntc_signature_select_device", "ntc_signature_hist_device",
    "ntc_k1_variant_stats",
    "ntc_bloom_size", "ntc_bloom_insert_device", "ntc_bloom_query_device", "ntc_bloom_insert_hashes_device", "ntc_bloom_query_hashes_device",
    "ntc_bloom_popcount_device", "ntc_bloom_or_device", "ntc_bloom_write", "ntc_bloom_read",
    "ntc_cbloom_insert_device", "ntc_cbloom_query_device", "ntc_cbloom_profile_device", "ntc_cbloom_insert_hashes_device", "ntc_cbloom_query_hashes_device",
    "ntc_cbloom_threshold_device", "ntc_bloom_insert_solid_device", "ntc_cbloom_add_device", "ntc_cbloom_hist_device", "ntc_cbloom_write", "ntc_cbloom_read",
    "ntc_bbloom_fpr", "ntc_bbloom_size", "ntc_bbloom_insert_device", "ntc_bbloom_query_device", "ntc_bbloom_insert_hashes_device", "ntc_bbloom_query_hashes_device",
    "ntc_bbloom_hist_device", "ntc_bbloom_insert_solid_device", "ntc_bbloom_write", "ntc_bbloom_read",
]

BLOOM_BLOCK = 4096  # NTC_BLOOM_BLOCK
BBLOOM_BLOCK_BITS = 512  # NTC_BBLOOM_BLOCK_BITS


class NtcBloomHeader(C.Structure):
    """ntc_bloom_header"""
    _fields_ = [
        ("k", C.c_uint32),
        ("n_hash", C.c_uint32),
        ("strand", C.c_uint32),
        ("reserved", C.c_uint32),
        ("m_bits", C.c_uint64),
        ("n_inserted", C.c_uint64),
    ]


class NtcGatherRow(C.Structure):
    """ntc_gather_row"""
    _fields_ = [
        ("ref", C.c_uint32),
        ("reserved", C.c_uint32),
        ("common", C.c_uint64),
        ("unique", C.c_uint64),
        ("unique_weight", C.c_uint64),
    ]


class NtcK1VariantInfo(C.Structure):
    """ntc_k1_variant_info"""
    _fields_ = [
        ("multi", C.c_uint8), ("mode", C.c_uint8), ("pref", C.c_uint8), ("dump", C.c_uint8), ("tiled", C.c_uint8), ("one", C.c_uint8), ("sig", C.c_uint8),
        ("reserved", C.c_uint8),
        ("launches", C.c_uint64),
        ("regime", C.c_uint64 * 8),
        ("last_grid", C.c_uint32),
        ("last_wpb", C.c_uint32),
        ("last_stride", C.c_uint32),
        ("reserved2", C.c_uint32),
        ("last_n_slots", C.c_uint64),
    ]


class NtcSigHeader(C.Structure):
    """ntc_sig_header"""
    _fields_ = [
        ("k", C.c_uint32),
        ("gap", C.c_uint32),
        ("strand", C.c_uint32),
        ("hpc", C.c_uint32),
        ("s_bits", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n", C.c_uint64),
        ("mask", C.c_char * 608),
    ]


class NtcHllConfig(C.Structure):
    """ntc_hll_config"""
    _fields_ = [
        ("n_k", C.c_uint32),
        ("k", C.POINTER(C.c_uint32)),
        ("n_seeds", C.c_uint32),
        ("seeds", C.POINTER(C.c_char_p)),
        ("n_bits", C.c_uint32),
        ("device", C.c_int32),
        ("stream", C.c_void_p),
        ("flags", C.c_uint32),
    ]


class NtcConfig(C.Structure):
    _fields_ = [
        ("n_k", C.c_uint32),
        ("k", C.POINTER(C.c_uint32)),
        ("gap", C.c_uint32),
        ("r_bits", C.c_uint32),
        ("s_bits", C.c_uint32),
        ("device", C.c_int32),
        ("stream", C.c_void_p),
        ("ext_sketch", C.c_void_p),
        ("ext_f1", C.c_void_p),
        ("flags", C.c_uint32),
        ("log_entries", C.c_uint64),
    ]


class NtcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ntCard: {msg} (status {code})")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ntcard_amd/csrc`). The HIP extension is mandatory; there is no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP runtime; if this process uses torch on the GPU as well, torch has to bring its
    # runtime up before ours touches the device (the other order leaves torch without visible GPUs).
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available():
        torch.cuda.init()
    L = C.CDLL(LIB_PATH)
    u32, u64, i32, p = C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p
    L.ntc_abi_version.restype = u32
    L.ntc_max_k.restype = u32
    L.ntc_last_error.restype = C.c_char_p
    L.ntc_create.argtypes = [C.POINTER(NtcConfig), C.POINTER(p)]
    L.ntc_create_seeded.argtypes = [C.POINTER(NtcConfig), u32, C.POINTER(C.c_char_p), C.POINTER(p)]
    L.ntc_destroy.argtypes = [p]
    L.ntc_destroy.restype = None
    L.ntc_reset.argtypes = [p]
    L.ntc_submit.argtypes = [p, p, p, u64]
    L.ntc_submit_spans.argtypes = [p, p, p, p, u64]
    L.ntc_submit_device.argtypes = [p, p, u64, u32, u32]
    L.ntc_submit_tiled_device.argtypes = [p, p, u64, u32]
    L.ntc_submit_tiled_ragged_device.argtypes = [p, p, u64, u32, p]
    L.ntc_submit_tiled_bins_device.argtypes = [p, u32, p, p, p, p]
    L.ntc_tiled_bytes.argtypes = [u64, u32]
    L.ntc_tiled_bytes.restype = u64
    L.ntc_gen_reads_tiled_device.argtypes = [i32, p, p, u64, u64, u64, u32, u32, u64]
    L.ntc_submit_long_device.argtypes = [p, p, p, u64, u32]
    L.ntc_long_plan.argtypes = [u32, u32, u64, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_long_stats.argtypes = [p, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_long_time.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ntc_hpc_compress.argtypes = [p, u64, p, C.POINTER(u64)]
    L.ntc_hpc_compress_device.argtypes = [i32, p, p, p, u64, p, p]
    L.ntc_hpc_stats.argtypes = [p, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_hpc_time.argtypes = [p, C.POINTER(C.c_double)]
    L.ntc_signature_size.argtypes = [p, u32, C.POINTER(u64)]
    L.ntc_signature.argtypes = [p, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_signature_inject.argtypes = [p, u32, p, p, u64]
    L.ntc_signature_inject_device.argtypes = [p, u32, p, p, u64]
    L.ntc_signature_compare.argtypes = [p, u64, p, u64, C.POINTER(u64)]
    L.ntc_signature_stats.argtypes = [p, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_signature_time.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ntc_signature_header.argtypes = [p, u32, C.POINTER(NtcSigHeader)]
    L.ntc_signature_write.argtypes = [C.c_char_p, C.POINTER(NtcSigHeader), p, p]
    L.ntc_signature_read.argtypes = [C.c_char_p, C.POINTER(NtcSigHeader), p, p, u64]
    L.ntc_signature_device.argtypes = [p, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_signature_sort_time.argtypes = [p, C.POINTER(C.c_double)]
    L.ntc_signature_sort_device.argtypes = [i32, p, p, p, u64]
    L.ntc_signature_compare_device.argtypes = [i32, p, p, p, u64, p, p, u64, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_signature_matrix_device.argtypes = [i32, p, u32, C.POINTER(p), C.POINTER(u64), p]
    L.ntc_signature_gather_device.argtypes = [i32, p, p, p, u64, u32, C.POINTER(p), C.POINTER(u64), u64, C.POINTER(NtcGatherRow), u32, C.POINTER(u32),
                                              C.POINTER(u64), C.POINTER(u64)]
    L.ntc_signature_union_device.argtypes = [i32, p, u32, C.POINTER(p), C.POINTER(p), C.POINTER(u64), p, p, u64, C.POINTER(u64)]
    L.ntc_signature_select_device.argtypes = [i32, p, p, p, u64, u32, C.POINTER(p), C.POINTER(u64), u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_signature_hist_device.argtypes = [i32, p, p, u64, u32, p, C.POINTER(u64)]
    L.ntc_sync.argtypes = [p]
    L.ntc_finish.argtypes = [p, p, p, p]
    L.ntc_merge_counters.argtypes = [p, p, p]
    L.ntc_merge_devices.argtypes = [C.POINTER(p), i32]
    L.ntc_value_hist_device.argtypes = [i32, p, p, u64, p]
    L.ntc_narrow_u16_device.argtypes = [i32, p, p, u64, p]
    L.ntc_sum_slices_u16_device.argtypes = [i32, p, p, u64, u32, u64]
    L.ntc_value_hist_u16_device.argtypes = [i32, p, p, u64, p]
    L.ntc_device_state.argtypes = [p, C.POINTER(p), C.POINTER(u64), C.POINTER(p)]
    L.ntc_log_export_device.argtypes = [p, u32, p, C.POINTER(u64), C.POINTER(u64)]
    L.ntc_log_replace_device.argtypes = [p, p, u64]
    L.ntc_hash_dump_device.argtypes = [i32, p, p, u64, u32, u32, u32, u32, u32, p, p]
    L.ntc_hash_dump_k1_device.argtypes = [i32, p, p, u64, u32, u32, u32, u32, u32, p, p]
    L.ntc_hash_dump_seed_device.argtypes = [i32, p, p, u64, u32, u32, C.c_char_p, u32, p, p]
    L.ntc_hash_dump_strand_device.argtypes = [i32, p, p, u64, u32, u32, C.c_char_p, u32, u32, p, p]
    L.ntc_gen_reads_device.argtypes = [i32, p, p, u64, u64, u64, u32, u32, u32, u64]
    L.ntc_estimate.argtypes = [p, u32, u32, u32, C.POINTER(C.c_double), p]
    L.ntc_write_hist.argtypes = [C.c_char_p, u64, C.c_double, p, u32]
    L.ntc_kernel_time.argtypes = [p, C.POINTER(C.c_double), C.POINTER(u64)]
    L.ntc_apply_time.argtypes = [p, C.POINTER(C.c_double), C.POINTER(u64)]
    L.ntc_fixup_time.argtypes = [p, C.POINTER(C.c_double)]
    L.ntc_merge_allocations.argtypes = [p, C.POINTER(u64)]
    L.ntc_flush.argtypes = [p]
    L.ntc_update_mode.argtypes = [p, C.POINTER(u32)]
    L.ntc_set_profiling.argtypes = [p, C.c_int]
    L.ntc_hll_create.argtypes = [u32, u32, i32, p, C.POINTER(p)]
    L.ntc_hll_finish.argtypes = [p, p, p]
    L.ntc_hll_estimate.argtypes = [p, u32, C.POINTER(C.c_double)]
    L.ntc_hll_create_ex.argtypes = [C.POINTER(NtcHllConfig), C.POINTER(p)]
    L.ntc_hll_estimate_strand.argtypes = [p, u32, u32, C.POINTER(C.c_double)]
    L.ntc_k1_variant_stats.argtypes = [u32, C.POINTER(NtcK1VariantInfo)]
    L.ntc_bloom_size.argtypes = [u64, u32, C.c_double, C.POINTER(u64)]
    L.ntc_bloom_insert_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_bloom_query_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, p, p]
    L.ntc_bloom_insert_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64]
    L.ntc_bloom_query_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64, p]
    L.ntc_bloom_popcount_device.argtypes = [i32, p, p, u64, C.POINTER(u64)]
    L.ntc_bloom_or_device.argtypes = [i32, p, p, p, u64]
    L.ntc_bloom_write.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p]
    L.ntc_bloom_read.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p, u64]
    L.ntc_cbloom_insert_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_cbloom_query_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, u32, p, p]
    L.ntc_cbloom_profile_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, p]
    L.ntc_cbloom_insert_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64]
    L.ntc_cbloom_query_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64, p]
    L.ntc_cbloom_threshold_device.argtypes = [i32, p, p, u64, u32, p]
    L.ntc_bloom_insert_solid_device.argtypes = [i32, p, p, u64, u32, p, u64, u32, u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_cbloom_add_device.argtypes = [i32, p, p, p, u64]
    L.ntc_cbloom_hist_device.argtypes = [i32, p, p, u64, p]
    L.ntc_cbloom_write.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p]
    L.ntc_cbloom_read.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p, u64]
    L.ntc_bbloom_fpr.argtypes = [u64, u64, u32, C.POINTER(C.c_double)]
    L.ntc_bbloom_size.argtypes = [u64, u32, C.c_double, C.POINTER(u64)]
    L.ntc_bbloom_insert_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_bbloom_query_device.argtypes = [i32, p, p, u64, u32, u32, u32, p, p, u64, p, p]
    L.ntc_bbloom_insert_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64]
    L.ntc_bbloom_query_hashes_device.argtypes = [i32, p, p, u64, u32, u32, p, u64, p]
    L.ntc_bbloom_hist_device.argtypes = [i32, p, p, u64, p]
    L.ntc_bbloom_insert_solid_device.argtypes = [i32, p, p, u64, u32, p, u64, u32, u32, u32, u32, p, p, u64, C.POINTER(u64)]
    L.ntc_bbloom_write.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p]
    L.ntc_bbloom_read.argtypes = [C.c_char_p, C.POINTER(NtcBloomHeader), p, u64]
    for name in ABI_SYMBOLS:
        fn = getattr(L, name)
        if name not in ("ntc_abi_version", "ntc_max_k", "ntc_last_error", "ntc_destroy", "ntc_tiled_bytes"):
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise NtcError(rc, lib().ntc_last_error().decode("utf-8", "replace"))
