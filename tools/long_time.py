#!/usr/bin/env python3
"""tools/long_time.py — long sequences through ntc_submit_long_device and through the host path behind NTC_LONG_MIN (-k: one k or a list, default 32;
sBits 7, 1.5 G genome-like bases per submit; one engine at a time, one host thread).
  device entry, per piece length: cut ms, gather ms, hash + fix-up ms (the engine's timers) and the whole step (submit + finish, wall clock)
      for (a) one sequence, (b) sequences of 10 kb +- 50 %; and the cut kernel against a plain device copy of the bytes it moves.
      Every figure is the MEDIAN of --reps in-process repeats behind one warm-up submit, with the spread (min .. max) behind it.
      An engine that does not qualify for the cut (a wide list; any list before the shared cut) gathers the sequences whole: pieces 0, cut 0.
  host entry: wall time of ntc_submit + ntc_sync for the same bytes, and for smaller batches, on row slots (NTC_LONG_MIN = 0: the path every
      host batch took before there was a device-side cut) and with the cut (NTC_LONG_MIN = 1)."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("-k", "--klist", default="32", help="k, or a list: 21,25,31")
ap.add_argument("--bases", type=int, default=1_500_000_000)
ap.add_argument("--pieces", default="256,512,1008,4080")
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

klist = [int(x) for x in args.klist.split(",")]
k, r_bits, s_bits = max(klist), 27, 7
rl = 1000
n_reads = args.bases // rl
total = n_reads * rl
d = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(d.data_ptr(), 9, 0, n_reads, rl, rl, 1, genome_len=100_000_000)  # stride == length: the reads lie behind one another
torch.cuda.synchronize()
print("device: %s; %d bases per submit, k = %s, sBits %d, rBits %d; median of %d repeats (min .. max)" % (torch.cuda.get_device_name(0), total, args.klist, s_bits, r_bits, args.reps), flush=True)


def ragged_offsets(n_bytes, seed=1):
    gen = np.random.default_rng(seed)
    lens = gen.integers(5000, 15001, size=n_bytes // 5000 + 1).astype(np.uint64)
    offs = np.concatenate(([0], np.cumsum(lens, dtype=np.uint64))).astype(np.uint64)
    offs = offs[offs < n_bytes]
    return np.concatenate((offs, [n_bytes])).astype(np.uint64)


shapes = [("(a) one sequence", np.array([0, total], dtype=np.uint64)), ("(b) 10 kb +- 50 %", ragged_offsets(total))]


def device_case(offs, piece_len):
    """-> per column (cut, gather, hash + fix-up, step ms per submit) its (median, min, max) over --reps, and the pieces"""
    rows = []
    with nt.Engine(klist, r_bits=r_bits, s_bits=s_bits) as e:
        e.set_profiling(True)
        e.submit_long_device(d.data_ptr(), offs, piece_len)  # warm-up: scratch, log mode probe, first apply
        e.finish(p_hist=False)
        pieces = e.long_stats()[0]
        for _ in range(args.reps):
            c0, g0 = e.long_time()
            h0 = e.kernel_time()[0] + e.fixup_time()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.submit_long_device(d.data_ptr(), offs, piece_len)
            e.finish(p_hist=False)
            dt = (time.perf_counter() - t0) * 1e3
            c1, g1 = e.long_time()
            rows.append((c1 - c0, g1 - g0, e.kernel_time()[0] + e.fixup_time() - h0, dt))
    cols = np.array(rows)
    return [(float(np.median(c)), float(c.min()), float(c.max())) for c in cols.T], pieces


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


print("\ndevice entry (ntc_submit_long_device)")
fmt = lambda t: "%.3f (%.3f .. %.3f)" % t
print("%-20s %9s %10s %24s %24s %24s %24s %11s" % ("shape", "piece_len", "pieces", "cut ms", "gather ms", "hash+fixup ms", "step ms", "cut / copy"))
for name, offs in shapes:
    for pl in [int(x) for x in args.pieces.split(",")]:
        (cut, gather, hk, dt), pieces = device_case(offs, pl)
        cp = copy_ms(pieces * pl) if pieces else 0.0  # a plain copy reads and writes what the cut reads and writes
        print("%-20s %9d %10d %24s %24s %24s %24s %10.0f%%" % (name, pl, pieces, fmt(cut), fmt(gather), fmt(hk), fmt(dt), 100.0 * cp / cut[0] if cut[0] else 0.0), flush=True)

if not args.skip_host:
    host = d[:total].cpu().numpy()

    def host_case(n_bytes, offs, long_min):
        """-> wall ms of ntc_submit + ntc_sync, best of --reps"""
        os.environ["NTC_LONG_MIN"] = str(long_min)
        best = None
        with nt.Engine(klist, r_bits=r_bits, s_bits=s_bits) as e:
            for rep in range(args.reps + 1):  # (the first: staging and scratch grow)
                t0 = time.perf_counter()
                e.submit(host[:n_bytes], offs)
                e.sync()
                dt = (time.perf_counter() - t0) * 1e3
                if rep and (best is None or dt < best):
                    best = dt
            pieces = e.long_stats()[0] // (args.reps + 1)
        os.environ.pop("NTC_LONG_MIN", None)
        return best, pieces

    print("\nhost entry (ntc_submit + ntc_sync, wall ms): row slots = NTC_LONG_MIN=0, cut = NTC_LONG_MIN=1")
    print("%-20s %12s %10s %12s %10s" % ("shape", "bytes", "pieces", "row slots", "cut"))
    for name, offs in shapes:
        rows, _ = host_case(total, offs, 0)
        cut, pieces = host_case(total, offs, 1)
        print("%-20s %12d %10d %12.2f %10.2f" % (name, total, pieces, rows, cut), flush=True)
    want = 8192
    while want * 977 <= total:
        n_bytes = want * 977 + 31
        offs = ragged_offsets(n_bytes)
        rows, _ = host_case(n_bytes, offs, 0)
        cut, pieces = host_case(n_bytes, offs, 1)
        print("%-20s %12d %10d %12.2f %10.2f" % ("(b) smaller batch", n_bytes, pieces, rows, cut), flush=True)
        want *= 2
