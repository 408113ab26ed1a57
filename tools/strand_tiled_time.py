#!/usr/bin/env python3
"""tools/strand_tiled_time.py — a one-strand engine on the tiled kernels (NTC_FLAG_STRAND_TILED) against the same engine on the general kernel and against
canonical K1h + K1f, all from the SAME device-resident tiles: 10 M genome-like 150 bp reads per submit, rBits 27, sBits 7, median (min .. max) of --reps
in-process repeats after a warm-up submit.  Three columns per case:
  (a) general   the strand engine without the flag: tiles re-laid out as row slots, then K1's one-strand form (what a strand engine did before the flag
                existed; --root DIR times another tree, e.g. the parent commit's, which has this column and (c) only)
  (b) tiled     the one-strand K1h kernels + K1f, forward and reverse
  (c) canonical K1h + K1f
The engine's timers (ntc_kernel_time, ntc_fixup_time, ntc_apply_time) are separate spans on its stream: "hash" = the hash kernels alone (K1h; for (a) K1
alone — the re-layout pass runs outside every span and shows only in the step), "fix-up" = K1f (0 for (a)), "apply" = the sketch update, "step" = wall
clock of submit + flush + sync.  "hash+fix" is the per-repeat sum of the first two.  Per engine two runs, without NTC_FLAG_DEFER_REDO (K1f behind every K1h
launch) and with it (one K1f over the waiting launches); the step and the apply are the non-deferring run's.  The update mode the engine ends in is printed
too.  Last lines per case: (b) against (a), and the pass condition — hash+fix of (b) minus that of (c) against the spread of (c)'s repeats, non-deferring."""
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

n, L, r_bits, s_bits = args.reads, 150, 27, 7
tiles = torch.empty(nt.tiled_bytes(n, L), dtype=torch.uint8, device="cuda")
nt.gen_reads_tiled_device(tiles.data_ptr(), 9, 0, n, L, 1, genome_len=100_000_000)
torch.cuda.synchronize()
has_tiled = hasattr(nt, "FLAG_STRAND_TILED")


def med(v):
    return (statistics.median(v), min(v), max(v))


def timed(make, defer):
    """-> dict of (median, min, max) per timer, and the update mode at the end"""
    e = make(nt.FLAG_DEFER_REDO if defer else 0)
    try:
        e.set_profiling(True)
        for _ in range(2):  # warm-up: log mode probe, first apply, scratch allocations
            e.submit_tiled_device(tiles.data_ptr(), n, L)
            e.flush()
            e.sync()
        hs, fs, aps, ws = [], [], [], []
        for _ in range(args.reps):
            k0, f0, a0 = e.kernel_time()[0], e.fixup_time(), e.apply_time()[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.submit_tiled_device(tiles.data_ptr(), n, L)
            e.flush()
            e.sync()
            ws.append((time.perf_counter() - t0) * 1e3)
            hs.append(e.kernel_time()[0] - k0)
            fs.append(e.fixup_time() - f0)
            aps.append(e.apply_time()[0] - a0)
        mode = e.update_mode()
    finally:
        e.close()
    return dict(hash=med(hs), fix=med(fs), hf=med([h + f for h, f in zip(hs, fs)]), apply=med(aps), step=med(ws), mode="direct atomics" if mode else "hit log")


def engine(klist, gap, strand, tiled_route):
    def make(extra):
        kw = dict(r_bits=r_bits, s_bits=s_bits, flags=extra)
        if strand != "canonical":
            kw["strand"] = strand
            if tiled_route:
                kw["strand_tiled"] = True
                kw["flags"] = extra | nt.FLAG_REQUIRE_TILED
        return nt.Engine(klist, gap=gap, **kw)
    return make


def fmt(t):
    return "%7.3f (%6.3f ..%7.3f)" % t


cases = [("k=32", [32], 0), ("k=21", [21], 0), ("k=32 -g 8", [32], 8), ("k=21,25,31", [21, 25, 31], 0)]
print("tree: %s   device: %s   %d x %d bp per submit from tiles, rBits %d, sBits %d, median (min .. max) of %d, ms per submit" %
      ("this tree" if args.root == os.path.dirname(os.path.dirname(os.path.abspath(__file__))) else "the tree given with --root", torch.cuda.get_device_name(0), n, L, r_bits, s_bits, args.reps))
print("%-12s %-22s %24s %24s %24s %24s %24s %24s %24s  %s" % ("case", "column", "hash", "fix-up", "hash+fix", "hash (deferring)", "fix-up (deferring)", "apply", "step", "update mode"))
for name, klist, gap in cases:
    cols = [("(a) general " + s, engine(klist, gap, s, False)) for s in ("forward", "reverse")]
    if has_tiled:
        cols += [("(b) tiled " + s, engine(klist, gap, s, True)) for s in ("forward", "reverse")]
    cols.append(("(c) canonical", engine(klist, gap, "canonical", False)))
    got = {}
    for col, make in cols:
        nd, df = timed(make, False), timed(make, True)
        got[col] = nd
        print("%-12s %-22s %s %s %s %s %s %s %s  %s" % (name, col, fmt(nd["hash"]), fmt(nd["fix"]), fmt(nd["hf"]), fmt(df["hash"]), fmt(df["fix"]), fmt(nd["apply"]), fmt(nd["step"]),
                                                     nd["mode"]), flush=True)
    if has_tiled:
        c = got["(c) canonical"]["hf"]
        for s in ("forward", "reverse"):
            a, b = got["(a) general " + s], got["(b) tiled " + s]
            print("%-12s (b)/(a) %s: hash+fix against K1 alone %.3f, step %.3f;  (b) - (c) hash+fix = %+.3f ms, spread of (c) = %.3f ms: %s" %
                  (name, s, b["hf"][0] / a["hf"][0], b["step"][0] / a["step"][0], b["hf"][0] - c[0], c[2] - c[1],
                   "within" if b["hf"][0] - c[0] <= c[2] - c[1] else "EXCEEDS"), flush=True)
