"""The fix-up kernels K1f (ntcard_amd/csrc/ntc_sketch_k1h.hip: the F1 role and the suspect role of k1h_fix_kernel, k1h_slow_kernel) on the directed
case families of tests/k1f_cases.py.  tests/test_k1f_cases_host.py runs the same families through the CPU emulator and asserts what they cover (every
combination of dirty pieces, ties, mark 2, every offset, every position of a dirty byte); here they go through the HIP kernels, and every comparison is
EXACT: F1, every uint16 counter and the value histogram against tests/orc.py.

Every tile family runs on the fast path (the engine's defaults) and on the slow path (NTC_K1H_SUS_CAP = 7: the suspect lists overflow, k1h_slow_kernel
re-derives every window near a dirty piece from the bytes); on top of that: reference-table slot bytes (slow path by a byte), deferred fix-ups (one K1f
over three launches), unused slots of the last tile that hold anything, spaced seeds, K1f's hit-log regions running full, and the long path under a k
list (trimmed piece lengths: real data behind a "read's" end)."""
import functools

import numpy as np
import pytest

import k1f_cases as kc
import orc
from gpu_support import nt, on_device  # noqa: F401
from support import assert_same_sketch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R_BITS = 14


FAMILIES = {}
for _k in kc.F1_K:
    for _L in kc.f1_lengths(_k):
        FAMILIES[f"f1_single-k{_k}-L{_L}"] = functools.partial(kc.f1_single, _k, _L)
    FAMILIES[f"f1_pairs-k{_k}"] = functools.partial(kc.f1_pairs, _k)
    FAMILIES[f"f1_runs-k{_k}"] = functools.partial(kc.f1_runs, _k)
    for _L in kc.suspects_end_lengths(_k):
        FAMILIES[f"suspects_end-k{_k}-L{_L}"] = functools.partial(kc.suspects_end, _k, _L)
FAMILIES["bytes256"] = kc.bytes256
for _k, _sb in ((12, 7), (17, 7), (32, 7), (32, 8), (32, 11)):
    FAMILIES[f"suspects-k{_k}-s{_sb}"] = functools.partial(kc.suspects, _k, _sb)
for _C, _k in kc.RAGGED:
    FAMILIES[f"ragged-C{_C}-k{_k}"] = functools.partial(kc.ragged, _C, _k)
FAMILIES["dense"] = kc.dense
SPACED = {}
for _k, _gap in ((12, 2), (32, 8)):
    SPACED[f"suspects-k{_k}-g{_gap}"] = functools.partial(kc.suspects, _k, 7, _gap)
    for _L in kc.f1_lengths(_k):
        SPACED[f"f1_single-k{_k}-g{_gap}-L{_L}"] = functools.partial(kc.f1_single, _k, _L, 7, _gap)
SLOTS = {f"slot_bytes-{v}": functools.partial(kc.slot_bytes, v) for v in kc.SLOT_BYTES}
ALL = dict(FAMILIES, **SPACED, **SLOTS)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return ALL[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = case_of(name)
    oc, of1 = orc.sketch_reads(c.reads, [c.k], c.gap, R_BITS, c.s_bits)
    return oc, of1


def submit(e, case, keep, unused=ord("A")):
    t = torch.from_numpy(kc.tile(case.reads, case.read_len, unused)).cuda()
    keep.append(t)
    if case.tails is None:
        e.submit_tiled_device(t.data_ptr(), len(case.reads), case.read_len)
    else:
        d = torch.from_numpy(case.tails.reshape(-1).astype(np.int32)).cuda()
        keep.append(d)
        e.submit_tiled_ragged_device(t.data_ptr(), len(case.reads), case.read_len // 16, d.data_ptr())


def run(nt, name, flags=0, unused=ord("A"), log_entries=0):
    case = case_of(name)
    keep = []
    with nt.Engine([case.k], gap=case.gap, r_bits=R_BITS, s_bits=case.s_bits, flags=flags | nt.FLAG_REQUIRE_TILED, log_entries=log_entries) as e:
        submit(e, case, keep, unused)
        return e.finish(counters=True)


check = functools.partial(assert_same_sketch, hist_r_bits=R_BITS)  # F1, every counter and the value histogram


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fast_path(nt, name):
    check(run(nt, name), oracle(name), name)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_slow_path_by_suspect_overflow(nt, monkeypatch, name):
    monkeypatch.setenv("NTC_K1H_SUS_CAP", "7")
    check(run(nt, name), oracle(name), name)


@pytest.mark.parametrize("name", list(SLOTS))
def test_slow_path_by_a_table_slot_byte(nt, name):
    check(run(nt, name), oracle(name), name)


@pytest.mark.parametrize("middle", ["suspects-k32-s7", "slot_bytes-4"])
def test_deferred_fixups_over_three_launches(nt, middle):
    """NTC_FLAG_DEFER_REDO: three families of different read length in one engine before finish — ONE K1f over three launches (blockIdx.y).  With the slot
    bytes in the middle one only that launch takes the slow path; the other two must still be exact"""
    names = ["f1_single-k32-L48", middle, "suspects_end-k32-L64"]
    assert len({case_of(n).read_len for n in names}) == 3
    keep = []
    with nt.Engine([32], r_bits=R_BITS, s_bits=7, flags=nt.FLAG_REQUIRE_TILED | nt.FLAG_DEFER_REDO) as e:
        for n in names:
            submit(e, case_of(n), keep)
        got = e.finish(counters=True)
    oc = sum(oracle(n)[0].astype(np.uint32) for n in names)
    assert oc.max() < 65536
    check(got, (oc.astype(np.uint16), sum(oracle(n)[1] for n in names)), names)


@pytest.mark.parametrize("unused", [ord("N"), 0x01, 0xFF])
def test_unused_slots_hold_anything(nt, unused):
    """the slots behind the batch's last read are ignored whatever they hold (include/ntcard_hip.h): N, a reference-table slot byte (it must not send the
    launch down the slow path either: nothing may change), 0xFF"""
    name = "suspects-k32-s7"
    got = run(nt, name, unused=unused)
    check(got, oracle(name), (name, unused))
    ref = run(nt, name)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("name", list(SPACED))
def test_spaced_seed(nt, name):
    check(run(nt, name), oracle(name), name)


def test_hit_log_regions_of_k1f_run_full(nt):
    """kc.dense with log_entries = 2^18 (regions of 256 entries): the K1f waves that share the dense block's suspect region find their hit-log regions full
    and fall back to device atomics (count_hit: pos >= klog_cap); tests/test_k1f_cases_host.py asserts the density"""
    check(run(nt, "dense", log_entries=1 << 18), oracle("dense"), "dense")
    check(run(nt, "dense", log_entries=1 << 18, flags=nt.FLAG_ALWAYS_LOG | nt.FLAG_PARTITION_ALWAYS), oracle("dense"), "dense, partitioned")


# ---- the long path under a k list ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_oracle(kl):
    return orc.sketch_reads([kc.trimmed(kl)], list(kl), 0, R_BITS, 7)


def count_trimmed(nt, kl, klist):
    seq = kc.trimmed(kl)
    d, offs = on_device([seq])
    with nt.Engine(list(klist), r_bits=R_BITS, s_bits=7, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_long_device(d.data_ptr(), offs, kc.TRIMMED_PIECE)
        got = e.finish(counters=True)
        pieces, seqs = e.long_stats()
    assert seqs == 1 and pieces == nt.long_plan(max(klist), kc.TRIMMED_PIECE, len(seq))[0] and pieces < 300
    return got


@pytest.mark.parametrize("kl", kc.TRIMMED_LISTS, ids=str)
@pytest.mark.parametrize("env", [None, ("NTC_LONG_ROUND_BYTES", "1"), ("NTC_K1H_SUS_CAP", "7")], ids=["default", "rounds", "sus_cap7"])
def test_trimmed_pieces_under_a_k_list(nt, monkeypatch, kl, env):
    if env:
        monkeypatch.setenv(*env)
    check(count_trimmed(nt, kl, kl), long_oracle(kl), (kl, env))


@pytest.mark.parametrize("kl", kc.TRIMMED_LISTS, ids=str)
def test_trimmed_inputs_under_the_largest_k_alone(nt, kl):
    """the single-k engines [32] and [27] on the same buffers (the same cut, no trimming)"""
    oc, of1 = long_oracle(kl)
    ki = list(kl).index(max(kl))
    check(count_trimmed(nt, kl, (max(kl),)), (oc[ki:ki + 1], of1[ki:ki + 1]), kl)
