#!/usr/bin/env python3
"""tools/seed_time.py — spaced seeds given as masks (ntc_create_seeded) vs ntcard's -g seed and plain k, on device-resident
genome-like reads (10 M x 150 bp per submit, row slots: K1).  Per case: the hash kernels' time per submit (the engine's kernel
timers) and the whole step (submit + apply, wall clock).  --gap-only: the -g row alone (for the parent commit, --root DIR)."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose ntcard_amd is timed")
ap.add_argument("--gap-only", action="store_true")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

n, L, stride, r_bits, s_bits = 10_000_000, 150, 152, 27, 7
bs = []
for i in range(3):
    d = torch.empty(n * stride + 16, dtype=torch.uint8, device="cuda")
    nt.gen_reads_device(d.data_ptr(), 9, i * n, n, L, stride, 1, genome_len=100_000_000)
    bs.append(d)
torch.cuda.synchronize()


def timed(make_engines):
    """-> (hash ms per submit, step ms per submit), best of --reps; every engine sees every batch"""
    best = None
    for _ in range(args.reps):
        es = make_engines()
        try:
            for e in es:
                e.set_profiling(True)
                e.submit_device(bs[0].data_ptr(), n, L, stride)  # warm-up: log mode probe, first apply
                e.finish()
            k0 = [e.kernel_time()[0] for e in es]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in bs[1:]:
                for e in es:
                    e.submit_device(d.data_ptr(), n, L, stride)
            for e in es:
                e.finish()
            dt = (time.perf_counter() - t0) * 1e3 / (len(bs) - 1)
            hk = sum(e.kernel_time()[0] - k for e, k in zip(es, k0)) / (len(bs) - 1)
        finally:
            for e in es:
                e.close()
        if best is None or dt < best[1]:
            best = (hk, dt)
    return best


g5 = "1" * 13 + "0" * 5 + "1" * 13
cases = [("k=31 -g 5 (Engine([31], gap=5))", lambda: [nt.Engine([31], gap=5, r_bits=r_bits, s_bits=s_bits)])]
if not args.gap_only:
    one = "1" * 10 + "0" * 5 + "1" * 16
    two = "1" * 7 + "000" + "1" * 8 + "000" + "1" * 10
    four = "1111" + "00" + "1111" + "00" + "1111" + "00" + "1111" + "00" + "1" * 7
    five = ("111" + "00") * 5 + "1" * 6
    k64 = "1" * 20 + "0" * 4 + "1" * 16 + "0" * 4 + "1" * 20
    assert len(one) == len(two) == len(four) == len(five) == 31 and len(k64) == 64
    seed = lambda ms: (lambda: [nt.Engine.from_seeds(ms, r_bits=r_bits, s_bits=s_bits)])  # noqa: E731
    cases += [
        ("k=31 plain (Engine([31]))", lambda: [nt.Engine([31], r_bits=r_bits, s_bits=s_bits)]),
        ("k=31 the -g 5 seed as a mask", seed([g5])),
        ("k=31 1 run, not symmetric", seed([one])),
        ("k=31 2 interior runs", seed([two])),
        ("k=31 4 interior runs", seed([four])),
        ("k=31 5 interior runs (closed-form XOR-out)", seed([five])),
        ("k=64 2 interior runs", seed([k64])),
        ("4 masks, one engine", seed([one, two, four, k64])),
        ("4 masks, 4 engines", lambda: [nt.Engine.from_seeds([m], r_bits=r_bits, s_bits=s_bits) for m in (one, two, four, k64)]),
    ]
print("%-46s %12s %12s" % ("case (10 M x 150 bp per submit)", "hash ms", "step ms"))
for name, make in cases:
    hk, dt = timed(make)
    print("%-46s %12.3f %12.3f" % (name, hk, dt), flush=True)
