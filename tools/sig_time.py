#!/usr/bin/env python3
"""tools/sig_time.py — what NTC_FLAG_SIGNATURE costs (10 M genome-like 150-base reads per submit, k = 32, sBits 7 and 11, device-resident row slots,
profiling on; one engine at a time, one host thread).  The yardstick is the same batch on the same engine WITHOUT the flag under NTC_FLAG_LANE_KERNEL —
the general kernel K1, which is what a signature engine runs: K1 hash ms (ntc_kernel_time) and the whole step (submit + finish, wall clock).  Beside it
the signature engine's K1 ms, insert ms and grow ms (ntc_signature_time), its step, the distinct values it holds and its table slots.  Every figure is the
MEDIAN of --reps in-process repeats behind one warm-up submit (which grows the table to its size), with the spread (min .. max) behind it.
NTC_SIG_LOG_ENTRIES / NTC_SIG_SLOTS in the environment are passed through to the engine (include/ntcard_hip.h)."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("-k", type=int, default=32)
ap.add_argument("--sbits", default="7,11")
ap.add_argument("--rbits", type=int, default=27)
args = ap.parse_args()
sys.path.insert(0, args.root)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

L, stride = 150, 152
d = torch.empty(args.reads * stride + 16, dtype=torch.uint8, device="cuda")
nt.gen_reads_device(d.data_ptr(), 9, 0, args.reads, L, stride, 1, genome_len=100_000_000)
torch.cuda.synchronize()
print("device: %s; %d reads of %d bases per submit (row slots, stride %d), k = %d, rBits %d; median of %d repeats (min .. max); NTC_SIG_LOG_ENTRIES=%s" %
      (torch.cuda.get_device_name(0), args.reads, L, stride, args.k, args.rbits, args.reps, os.environ.get("NTC_SIG_LOG_ENTRIES", "default")), flush=True)


def case(s_bits, signature):
    rows = []
    with nt.Engine([args.k], r_bits=args.rbits, s_bits=s_bits, flags=nt.FLAG_LANE_KERNEL, signature=signature) as e:
        e.set_profiling(True)
        e.submit_device(d.data_ptr(), args.reads, L, stride)  # warm-up: log mode probe, first apply, the table's growth
        e.finish(p_hist=False)
        for _ in range(args.reps):
            k0 = e.kernel_time()[0]
            a0 = e.apply_time()[0]
            i0, g0 = e.signature_time() if signature else (0.0, 0.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.submit_device(d.data_ptr(), args.reads, L, stride)
            e.finish(p_hist=False)
            dt = (time.perf_counter() - t0) * 1e3
            i1, g1 = e.signature_time() if signature else (0.0, 0.0)
            rows.append((e.kernel_time()[0] - k0, e.apply_time()[0] - a0, i1 - i0, g1 - g0, dt))
        distinct = e.signature_size() if signature else 0
        slots, grows = e.signature_stats() if signature else (0, 0)
    cols = np.array(rows)
    return [(float(np.median(c)), float(c.min()), float(c.max())) for c in cols.T], distinct, slots, grows


fmt = lambda t: "%.3f (%.3f .. %.3f)" % t
print("%-6s %-10s %24s %24s %24s %24s %26s %12s %12s %6s" % ("sBits", "engine", "K1 hash ms", "apply ms", "insert ms", "grow ms", "step ms", "distinct", "slots", "grows"))
for s_bits in [int(x) for x in args.sbits.split(",")]:
    for signature in (False, True):
        (k1, ap_ms, ins, grow, dt), distinct, slots, grows = case(s_bits, signature)
        print("%-6d %-10s %24s %24s %24s %24s %26s %12d %12d %6d" % (s_bits, "signature" if signature else "parent", fmt(k1), fmt(ap_ms), fmt(ins), fmt(grow), fmt(dt), distinct, slots, grows),
              flush=True)
