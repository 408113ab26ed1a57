#!/usr/bin/env python3
"""tools/long_time.py — long sequences through ntc_submit_long_device and through the host path behind NTC_LONG_MIN (k = 32, sBits 7,
1.5 G genome-like bases per submit; one engine at a time, one host thread).
  device entry, per piece length: cut ms, gather ms, hash + fix-up ms (the engine's timers) and the whole step (submit + finish, wall clock)
      for (a) one sequence, (b) sequences of 10 kb +- 50 %; and the cut kernel against a plain device copy of the bytes it moves.
  host entry: wall time of ntc_submit + ntc_sync for the same bytes, and for smaller batches, on row slots (NTC_LONG_MIN = 0: the path every
      host batch took before there was a device-side cut) and with the cut (NTC_LONG_MIN = 1)."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--bases", type=int, default=1_500_000_000)
ap.add_argument("--pieces", default="256,512,1008,4080")
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

k, r_bits, s_bits = 32, 27, 7
rl = 1000
n_reads = args.bases // rl
total = n_reads * rl
d = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(d.data_ptr(), 9, 0, n_reads, rl, rl, 1, genome_len=100_000_000)  # stride == length: the reads lie behind one another
torch.cuda.synchronize()
print("device: %s; %d bases per submit, k = %d, sBits %d, rBits %d" % (torch.cuda.get_device_name(0), total, k, s_bits, r_bits), flush=True)


def ragged_offsets(n_bytes, seed=1):
    gen = np.random.default_rng(seed)
    lens = gen.integers(5000, 15001, size=n_bytes // 5000 + 1).astype(np.uint64)
    offs = np.concatenate(([0], np.cumsum(lens, dtype=np.uint64))).astype(np.uint64)
    offs = offs[offs < n_bytes]
    return np.concatenate((offs, [n_bytes])).astype(np.uint64)


shapes = [("(a) one sequence", np.array([0, total], dtype=np.uint64)), ("(b) 10 kb +- 50 %", ragged_offsets(total))]


def device_case(offs, piece_len):
    """-> (cut, gather, hash + fix-up, step) ms per submit, the step's best of --reps, and the pieces"""
    best = None
    with nt.Engine([k], r_bits=r_bits, s_bits=s_bits) as e:
        e.set_profiling(True)
        e.submit_long_device(d.data_ptr(), offs, piece_len)  # warm-up: scratch, log mode probe, first apply
        e.finish(p_hist=False)
        pieces = e.long_stats()[0]
        for _ in range(args.reps):
            c0, g0 = e.long_time()
            h0 = e.kernel_time()[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.submit_long_device(d.data_ptr(), offs, piece_len)
            e.finish(p_hist=False)
            dt = (time.perf_counter() - t0) * 1e3
            c1, g1 = e.long_time()
            row = (c1 - c0, g1 - g0, e.kernel_time()[0] - h0, dt)
            if best is None or dt < best[3]:
                best = row
    return best, pieces


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
print("%-20s %9s %10s %10s %10s %14s %10s %12s" % ("shape", "piece_len", "pieces", "cut ms", "gather ms", "hash+fixup ms", "step ms", "cut / copy"))
for name, offs in shapes:
    for pl in [int(x) for x in args.pieces.split(",")]:
        (cut, gather, hk, dt), pieces = device_case(offs, pl)
        cp = copy_ms(pieces * pl)  # a plain copy reads and writes what the cut reads and writes
        print("%-20s %9d %10d %10.3f %10.3f %14.3f %10.3f %11.0f%%" % (name, pl, pieces, cut, gather, hk, dt, 100.0 * cp / cut if cut else 0.0), flush=True)

if not args.skip_host:
    host = d[:total].cpu().numpy()

    def host_case(n_bytes, offs, long_min):
        """-> wall ms of ntc_submit + ntc_sync, best of --reps"""
        os.environ["NTC_LONG_MIN"] = str(long_min)
        best = None
        with nt.Engine([k], r_bits=r_bits, s_bits=s_bits) as e:
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
