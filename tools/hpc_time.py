#!/usr/bin/env python3
"""tools/hpc_time.py — homopolymer-compressed counting through ntc_submit_long_device (NTC_FLAG_HPC; k = 32, sBits 7, 1.5 G genome-like bases per
submit; one engine at a time, one host thread), for (a) one sequence and (b) the same bases as sequences of 10 kb +- 50 %:
  compaction ms (ntc_hpc_time: mark + flag + scan + scatter + offsets kernels), the cut, gather and hash + fix-up ms behind it (the engine's timers)
  and the whole step (submit + finish, wall clock) — next to the same step WITHOUT the flag on the same bytes, and to a plain device copy of the
  source bytes.  Every figure is the MEDIAN of --reps in-process repeats behind one warm-up submit, with the spread (min .. max) behind it.
The generator's bases are uniform, so runs are short (a quarter of the bytes is dropped); --stretch N repeats every base 1 .. N times first."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("-k", "--klist", default="32")
ap.add_argument("--bases", type=int, default=1_500_000_000)
ap.add_argument("--piece", type=int, default=1008)
ap.add_argument("--stretch", type=int, default=1, help="repeat every generated base 1 .. N times (uniform), so that runs are longer")
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

klist = [int(x) for x in args.klist.split(",")]
r_bits, s_bits = 27, 7
rl = 1000
n_reads = args.bases // rl
total = n_reads * rl
d = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(d.data_ptr(), 9, 0, n_reads, rl, rl, 1, genome_len=100_000_000)  # stride == length: the reads lie behind one another
if args.stretch > 1:
    gen = torch.Generator(device="cuda").manual_seed(3)
    reps = torch.randint(1, args.stretch + 1, (total,), device="cuda", generator=gen)
    d = torch.cat((torch.repeat_interleave(d[:total], reps)[:total], d[total:]))
torch.cuda.synchronize()
print("device: %s; %d bases per submit, k = %s, sBits %d, rBits %d, piece_len %d, stretch %d; median of %d repeats (min .. max)" %
      (torch.cuda.get_device_name(0), total, args.klist, s_bits, r_bits, args.piece, args.stretch, args.reps), flush=True)


def ragged_offsets(n_bytes, seed=1):
    gen = np.random.default_rng(seed)
    lens = gen.integers(5000, 15001, size=n_bytes // 5000 + 1).astype(np.uint64)
    offs = np.concatenate(([0], np.cumsum(lens, dtype=np.uint64))).astype(np.uint64)
    offs = offs[offs < n_bytes]
    return np.concatenate((offs, [n_bytes])).astype(np.uint64)


shapes = [("(a) one sequence", np.array([0, total], dtype=np.uint64)), ("(b) 10 kb +- 50 %", ragged_offsets(total))]


def device_case(offs, hpc):
    """-> per column (hpc, cut, gather, hash + fix-up, step ms per submit) its (median, min, max) over --reps; pieces and bytes kept per submit"""
    rows = []
    with nt.Engine(klist, r_bits=r_bits, s_bits=s_bits, hpc=hpc) as e:
        e.set_profiling(True)
        e.submit_long_device(d.data_ptr(), offs, args.piece)  # warm-up: scratch, log mode probe, first apply
        e.finish(p_hist=False)
        pieces, kept = e.long_stats()[0], e.hpc_stats()[1]
        for _ in range(args.reps):
            c0, g0 = e.long_time()
            h0 = e.kernel_time()[0] + e.fixup_time()
            p0 = e.hpc_time()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.submit_long_device(d.data_ptr(), offs, args.piece)
            e.finish(p_hist=False)
            dt = (time.perf_counter() - t0) * 1e3
            c1, g1 = e.long_time()
            rows.append((e.hpc_time() - p0, c1 - c0, g1 - g0, e.kernel_time()[0] + e.fixup_time() - h0, dt))
    cols = np.array(rows)
    return [(float(np.median(c)), float(c.min()), float(c.max())) for c in cols.T], pieces, kept


def copy_ms(n_bytes):
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    best = None
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    return best


print("plain device copy of the %d source bytes: %.3f ms" % (total, copy_ms(total)), flush=True)
fmt = lambda t: "%.3f (%.3f .. %.3f)" % t
print("%-20s %5s %10s %12s %24s %24s %24s %24s %24s" % ("shape", "flag", "pieces", "bytes kept", "compaction ms", "cut ms", "gather ms", "hash+fixup ms", "step ms"))
for name, offs in shapes:
    for hpc in (False, True):
        (hp, cut, gather, hk, dt), pieces, kept = device_case(offs, hpc)
        print("%-20s %5s %10d %12d %24s %24s %24s %24s %24s" % (name, "hpc" if hpc else "-", pieces, kept, fmt(hp), fmt(cut), fmt(gather), fmt(hk), fmt(dt)), flush=True)
