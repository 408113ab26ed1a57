#!/usr/bin/env python3
"""tools/sig_sort_time.py — what the device side of signatures behind the container costs (profiles/signature.txt, "Sort, compare, matrix").
(1) ntc_signature, wall clock, on the engine state of tools/sig_time.py's protocol (10 M genome-like 150-base reads, k = 32, sBits 7 and 11) and on the
    593-entry plane of the test reads (tests/sig_model.py); with --root this is run against another tree's ntcard_amd (the parent commit's, whose
    ntc_signature sorts on the host) — the sections below need this commit's and are skipped there.
(2) the sort alone: the engine's T_SIG_SORT spans (HIP events, ntc_signature_sort_time) at the two engine sizes, and ntc_signature_sort_device between two
    HIP events on signature-shaped pairs of 407 213, 6 534 307 and 50 M entries (its scratch allocation included), beside a device copy of the same pairs.
(3) ntc_signature_compare_device on two lists of ~6.5 M with about half in common, against the host's ntc_signature_compare; (4) the matrix of 16 such
    lists against 120 host compares.
Every figure is the MEDIAN of --reps repeats behind one warm-up, with min .. max behind it."""
import argparse
import ctypes as C
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--sbits", default="7,11")
ap.add_argument("--sizes", default="407213,6534307,50000000")
ap.add_argument("--list", type=int, default=6_534_307, help="entries of a list of (3) and (4)")
ap.add_argument("--sigs", type=int, default=16)
ap.add_argument("--only", default="1,2,3,4")
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, args.root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402
import sig_model  # noqa: E402

NEW = hasattr(nt, "signature_sort_device")
only = set(int(x) for x in args.only.split(","))
fmt = lambda xs: "%.3f (%.3f .. %.3f)" % (float(np.median(xs)), min(xs), max(xs))
print("device: %s; ntcard_amd of %s (%s); median of %d repeats (min .. max) behind one warm-up" %
      (torch.cuda.get_device_name(0), os.path.relpath(args.root, HERE), "device sort" if NEW else "host sort", args.reps), flush=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_signature(e, label):
    e.set_profiling(True)
    n = e.signature_size()
    e.signature()  # warm-up: the scratch is allocated
    s0 = e.signature_sort_time() if NEW else 0.0
    ms = [wall(e.signature) for _ in range(args.reps)]
    sort_ms = (e.signature_sort_time() - s0) / args.reps if NEW else float("nan")
    dev = [wall(e.signature_device) for _ in range(args.reps)] if NEW else [float("nan")]
    print("%-28s %10d pairs   ntc_signature %28s ms   of it sort spans %8.3f ms   ntc_signature_device %28s ms" % (label, n, fmt(ms), sort_ms, fmt(dev)), flush=True)


if 1 in only:
    print("\n(1) ntc_signature, wall clock (compaction + sort + copy to the host)")
    L, stride = 150, 152
    d = torch.empty(args.reads * stride + 16, dtype=torch.uint8, device="cuda")
    nt.gen_reads_device(d.data_ptr(), 9, 0, args.reads, L, stride, 1, genome_len=100_000_000)
    torch.cuda.synchronize()
    for s_bits in [int(x) for x in args.sbits.split(",")]:
        with nt.Engine([32], r_bits=27, s_bits=s_bits, flags=nt.FLAG_LANE_KERNEL, signature=True) as e:
            e.submit_device(d.data_ptr(), args.reads, L, stride)
            time_signature(e, "%d reads, sBits %d" % (args.reads, s_bits))
    del d
    with nt.Engine([32], r_bits=14, s_bits=7, signature=True) as e:
        e.submit_reads(list(sig_model.equal_reads()))
        time_signature(e, "test reads, sBits 7")


def sig_shaped(n):
    """ntComp's two patterns at s = 7 in front, random bits behind; as int64 bit patterns on the device"""
    r = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda")
    one = (r & (2**56 - 1)) | (1 << 56)
    two = (r & (2**57 - 1)) | (63 << 57)
    return torch.where(torch.rand(n, device="cuda") < 0.5, one, two)


if 2 in only and NEW:
    print("\n(2) ntc_signature_sort_device on signature-shaped pairs (HIP events round the call: scratch allocation, histogram read-back and passes); "
          "a pass = count (8 B read per pair) + scatter (12 B read, 12 B written); copy = a device copy of the pairs (12 B read, 12 B written)")
    print("%12s %26s %7s %8s %14s %26s %12s" % ("pairs", "sort ms", "passes", "skipped", "GB/s of passes", "copy ms", "copy GB/s"))
    for n in [int(x) for x in args.sizes.split(",")]:
        keys = sig_shaped(n)
        vals = torch.arange(n, dtype=torch.int32, device="cuda")
        skipped = sum(1 for s in range(0, 64, 8) if int(((keys >> s) & 255).min()) == int(((keys >> s) & 255).max()))
        k, v = keys.clone(), vals.clone()
        nt.signature_sort_device(k.data_ptr(), v.data_ptr(), n)
        assert bool((k[1:] >= k[:-1]).all())  # (these keys are non-negative as int64)
        ms = []
        for _ in range(args.reps):
            k.copy_(keys), v.copy_(vals)
            ms.append(events(lambda: nt.signature_sort_device(k.data_ptr(), v.data_ptr(), n)))
        k2, v2 = torch.empty_like(keys), torch.empty_like(vals)
        cp = [events(lambda: (k2.copy_(keys), v2.copy_(vals))) for _ in range(args.reps + 1)][1:]
        passes = 8 - skipped
        print("%12d %26s %7d %8d %14.1f %26s %12.1f" % (n, fmt(ms), passes, skipped, n * (8 + 32 * passes) / np.median(ms) / 1e6, fmt(cp), n * 24 / np.median(cp) / 1e6), flush=True)
        del keys, vals, k, v, k2, v2


def host_compare(a, b):
    c = C.c_uint64()
    nt._abi.check(nt._abi.lib().ntc_signature_compare(a.ctypes.data_as(C.c_void_p), a.size, b.ctypes.data_as(C.c_void_p), b.size, C.byref(c)))
    return c.value


if (3 in only or 4 in only) and NEW:
    pool = torch.unique(torch.randint(1, 2**62, (2 * args.list,), dtype=torch.int64, device="cuda"))  # (non-negative: int64 order = uint64 order)
    dl = [pool[torch.rand(pool.numel(), device="cuda") < 0.5].contiguous() for _ in range(args.sigs)]
    hl = [x.cpu().numpy().view(np.uint64) for x in dl]
    del pool

if 3 in only and NEW:
    a, b = dl[0], dl[1]
    want = host_compare(hl[0], hl[1])
    print("\n(3) two lists of %d and %d entries, %d in common" % (a.numel(), b.numel(), want))
    assert nt.signature_compare_device(a.data_ptr(), 0, a.numel(), b.data_ptr(), 0, b.numel())[0] == want
    dev = [wall(lambda: nt.signature_compare_device(a.data_ptr(), 0, a.numel(), b.data_ptr(), 0, b.numel())) for _ in range(args.reps)]

    def with_upload():
        x, y = torch.from_numpy(hl[0].view(np.int64)).cuda(), torch.from_numpy(hl[1].view(np.int64)).cuda()
        nt.signature_compare_device(x.data_ptr(), 0, x.numel(), y.data_ptr(), 0, y.numel())
    with_upload()
    up = [wall(with_upload) for _ in range(args.reps)]
    host = [wall(lambda: host_compare(hl[0], hl[1])) for _ in range(args.reps)]
    print("ntc_signature_compare_device %s ms   with the upload of both lists %s ms   host ntc_signature_compare %s ms" % (fmt(dev), fmt(up), fmt(host)), flush=True)

if 4 in only and NEW:
    ptrs, ns = [x.data_ptr() for x in dl], [x.numel() for x in dl]
    m = nt.signature_matrix_device(ptrs, ns)
    assert int(m[0, 1]) == host_compare(hl[0], hl[1]) and int(m[args.sigs - 2, args.sigs - 1]) == host_compare(hl[-2], hl[-1])
    dev = [wall(lambda: nt.signature_matrix_device(ptrs, ns)) for _ in range(args.reps)]
    pairs = [(i, j) for i in range(args.sigs) for j in range(i + 1, args.sigs)]
    host = [wall(lambda: [host_compare(hl[i], hl[j]) for i, j in pairs]) for _ in range(3)]
    print("\n(4) %d lists of ~%d entries, %d pairs: ntc_signature_matrix_device %s ms   %d host compares %s ms (three repeats)" %
          (args.sigs, ns[0], len(pairs), fmt(dev), len(pairs), fmt(host)), flush=True)
