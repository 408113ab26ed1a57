#!/usr/bin/env python3
"""tools/strand_time.py — one-strand counting (NTC_FLAG_STRAND_FORWARD / _REVERSE) against canonical on the general kernel K1:
device-resident genome-like reads (10 M x 150 bp per submit, row slots, rBits 27, sBits 7).  Per case and strand: the hash kernels' and the
sketch update's time per submit (the engine's timers) and the wall clock of the step (submit + flush + sync), median of --reps in-process
repeats after a warm-up submit, with the spread (min .. max).  Canonical k = 32 and 32 / gap 8 run with NTC_FLAG_LANE_KERNEL so that they are
K1's like their one-strand forms; the tiled rows show what a strand engine's re-layout of a tiled batch costs, next to K1h + K1f on the same
tiles.  --root DIR times another tree (the parent commit: it has no strands, so only the canonical rows are printed)."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--reads", type=int, default=10_000_000)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

n, L, stride, r_bits, s_bits = args.reads, 150, 152, 27, 7
rows = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(rows.data_ptr(), 9, 0, n, L, stride, 1, genome_len=100_000_000)
tiles = torch.empty(nt.tiled_bytes(n, L), dtype=torch.uint8, device="cuda")
nt.gen_reads_tiled_device(tiles.data_ptr(), 9, 0, n, L, 1, genome_len=100_000_000)
torch.cuda.synchronize()
has_strands = hasattr(nt, "FLAG_STRAND_FORWARD")
strands = ["canonical"] + (["forward", "reverse"] if has_strands else [])


def timed(make, tiled):
    """-> [(median, min, max)] of hash ms, apply ms, step ms per submit"""
    e = make()
    try:
        e.set_profiling(True)
        submit = (lambda: e.submit_tiled_device(tiles.data_ptr(), n, L)) if tiled else (lambda: e.submit_device(rows.data_ptr(), n, L, stride))
        submit()  # warm-up: log mode probe, first apply, scratch allocations
        e.flush()
        e.sync()
        hs, aps, ws = [], [], []
        for _ in range(args.reps):
            k0, a0 = e.kernel_time()[0], e.apply_time()[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            submit()
            e.flush()
            e.sync()
            ws.append((time.perf_counter() - t0) * 1e3)
            hs.append(e.kernel_time()[0] - k0)
            aps.append(e.apply_time()[0] - a0)
    finally:
        e.close()
    return [(statistics.median(v), min(v), max(v)) for v in (hs, aps, ws)]


def engine(klist, gap=0, flags=0):
    def make(strand):
        kw = dict(r_bits=r_bits, s_bits=s_bits, flags=flags if strand == "canonical" else 0)
        if strand != "canonical":
            kw["strand"] = strand
        return nt.Engine(klist, gap=gap, **kw)
    return make


LANE = nt.FLAG_LANE_KERNEL
cases = [
    ("k=32", engine([32], flags=LANE), False, strands),
    ("k=64", engine([64]), False, strands),
    ("k=32,64,96,128", engine([32, 64, 96, 128], flags=LANE), False, strands),
    ("k=32 -g 8", engine([32], gap=8, flags=LANE), False, strands),
    ("k=32 tiled batch, re-laid out for K1", engine([32], flags=LANE), True, strands),
    ("k=32 tiled batch, K1h + K1f", engine([32]), True, ["canonical"]),
]
print("tree: %s   device: %s   %d x %d bp per submit, rBits %d, sBits %d, median (min .. max) of %d" %
      (args.root, torch.cuda.get_device_name(0), n, L, r_bits, s_bits, args.reps))
print("%-38s %-10s %26s %26s %26s" % ("case", "strand", "hash ms", "apply ms", "step ms"))
for name, make, tiled, ss in cases:
    for s in ss:
        r = timed(lambda: make(s), tiled)
        print("%-38s %-10s " % (name, s) + " ".join("%8.3f (%7.3f ..%8.3f)" % t for t in r), flush=True)
