#!/usr/bin/env python3
"""tools/nthll_time.py — nthll engines (ntc_hll_create_ex) on the general kernel K1: device-resident genome-like reads (10 M x 150 bp per submit, row
slots, b = 16).  Per case and strand: the device time of one submit — every plane's threshold refresh and hash launch, between two events on the
engine's stream — median of --reps in-process repeats after a warm-up submit (warm registers: the threshold has moved), with the spread (min .. max).
--root DIR times another tree (the parent commit: it has one plain k and no strands, so only the canonical k rows are printed)."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--reads", type=int, default=10_000_000)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

n, L, stride, n_bits = args.reads, 150, 152, 16
rows = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(rows.data_ptr(), 9, 0, n, L, stride, 1, genome_len=100_000_000)
torch.cuda.synchronize()
extended = hasattr(nt.HllEngine, "from_seeds")
gap32_8 = "1" * 12 + "0" * 8 + "1" * 12


def timed(make):
    """-> (median, min, max) of the hash ms per submit; the engine runs on the default stream, which is where torch records its events"""
    e = make()
    try:
        e.submit_device(rows.data_ptr(), n, L, stride)  # warm-up: the registers fill, the sub-batches double up to the whole submit
        e.sync()
        ms = []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.submit_device(rows.data_ptr(), n, L, stride)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
    finally:
        e.close()
    return statistics.median(ms), min(ms), max(ms)


cases = [("k=32", "canonical", lambda: nt.HllEngine(32, n_bits)), ("k=64", "canonical", lambda: nt.HllEngine(64, n_bits))]
if extended:
    for k in (32, 64):
        for s in ("forward", "reverse"):
            cases.append(("k=%d" % k, s, lambda k=k, s=s: nt.HllEngine([k], n_bits, strand=s)))
    for s in ("canonical", "forward"):
        cases.append(("seed 32 / gap 8", s, lambda s=s: nt.HllEngine.from_seeds([gap32_8], n_bits, strand=s)))
    cases.append(("k=32,64 (two planes)", "canonical", lambda: nt.HllEngine([32, 64], n_bits)))
print("tree: %s   device: %s   %d x %d bp per submit, b = %d, median (min .. max) of %d" % (args.root, torch.cuda.get_device_name(0), n, L, n_bits, args.reps))
print("%-24s %-10s %28s" % ("case", "strand", "hash ms per submit"))
for name, s, make in cases:
    print("%-24s %-10s %9.3f (%8.3f ..%9.3f)" % ((name, s) + timed(make)), flush=True)
