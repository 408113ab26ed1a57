#!/usr/bin/env python3
"""tools/sig_gather_time.py — what gather costs on the device (profiles/signature.txt, "Gather"; include/ntcard_hip.h: ntc_signature_gather_device).
One query of the 6.5 M-pair size used elsewhere in that profile, with counts, against 64 and against 1024 synthetic references of mixed overlap: a
reference takes a share of 5 % .. 95 % of its entries from a window of the query — windows of different references overlap, so later picks explain less than
they have in common — and the rest from outside it.  Timed, wall clock round the synchronous call, lists already on the device:
  whole    every row down to --threshold hashes
  search   the same call with room for no row: the ascent check, both search passes, one pick that stops at once and the final reduction
  rounds   whole - search (of the medians): what the rounds behind the first pick add
against the same greedy on the host, tests/sig_gather_model.py in numpy (its lookup of every reference in the query, and its rounds), whose result the
device's has to equal.  Every device figure is the MEDIAN of --reps repeats behind one warm-up, with min .. max behind it; the host runs --host-reps times."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--query", type=int, default=6_534_307, help="entries of the query")
ap.add_argument("--refs", default="64,1024")
ap.add_argument("--threshold", type=int, default=1)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import sig_gather_model  # noqa: E402

fmt = lambda xs: "%.3f (%.3f .. %.3f)" % (float(np.median(xs)), min(xs), max(xs))


def lists(n_refs, rng, inside, outside):
    """n_refs references: sizes log-uniform, 50 000 .. 1 000 000 entries for 64 of them and 32 times smaller for 1024"""
    lo, hi = 50_000 * 64 // n_refs, 1_000_000 * 64 // n_refs
    refs = []
    for _ in range(n_refs):
        size = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        common = int(size * rng.uniform(0.05, 0.95))
        width = min(inside.size, 3 * common)
        w0 = int(rng.integers(0, inside.size - width + 1))
        o0 = int(rng.integers(0, outside.size - 3 * (size - common) + 1))
        part = inside[w0: w0 + width][rng.random(width) < 1 / 3]
        rest = outside[o0: o0 + 3 * (size - common)][rng.random(3 * (size - common)) < 1 / 3]
        refs.append(np.sort(np.concatenate([part, rest])))
    return refs


rng = np.random.default_rng(2026)
pool = np.unique(rng.integers(1, 2**63, size=int(2.2 * args.query), dtype=np.uint64))
is_query = np.zeros(pool.size, dtype=bool)
is_query[rng.permutation(pool.size)[:args.query]] = True
query, outside = pool[is_query], pool[~is_query]
counts = rng.integers(1, 50, size=query.size).astype(np.uint32)
del pool, is_query
cases = []
for n_refs in [int(x) for x in args.refs.split(",")]:
    refs = lists(n_refs, rng, query, outside)
    host = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        want = sig_gather_model.gather(query, counts, refs, threshold=args.threshold)
        host.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    hits = sum(sig_gather_model.positions(query, r).size for r in refs)
    lookup = (time.perf_counter() - t0) * 1e3
    cases.append((refs, want, host, lookup, hits))
    print("host, %d references of %d .. %d entries, %d hits in all: %d rows, %d of %d query entries unassigned; numpy greedy %s ms, of it the lookup of "
          "every reference in the query %.3f ms" % (n_refs, min(r.size for r in refs), max(r.size for r in refs), hits, want[0].size, want[1], query.size,
                                                    fmt(host), lookup), flush=True)

import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402

print("device: %s; median of %d repeats (min .. max) behind one warm-up; threshold %d" % (torch.cuda.get_device_name(0), args.reps, args.threshold), flush=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


dq = torch.from_numpy(query.view(np.int64)).cuda()
dc = torch.from_numpy(counts.view(np.int32)).cuda()
for refs, want, host, lookup, hits in cases:
    dl = [torch.from_numpy(r.view(np.int64)).cuda() for r in refs]
    ptrs, ns = [x.data_ptr() for x in dl], [x.numel() for x in dl]
    whole_call = lambda: nt.signature_gather_device(dq.data_ptr(), dc.data_ptr(), query.size, ptrs, ns, threshold=args.threshold)
    search_call = lambda: nt.signature_gather_device(dq.data_ptr(), dc.data_ptr(), query.size, ptrs, ns, threshold=args.threshold, max_rows=0)
    got = whole_call()
    assert sig_gather_model.same(got, want), "the device's rows differ from the model's"
    assert search_call()[1] == query.size
    whole = [wall(whole_call) for _ in range(args.reps)]
    search = [wall(search_call) for _ in range(args.reps)]
    rounds = float(np.median(whole) - np.median(search))
    n_rows = got[0].size
    print("%4d references, %8d hits, %4d rows: whole %s ms   search %s ms   rounds %.3f ms (%.1f us per round)   host %.1fx the whole call" %
          (len(refs), hits, n_rows, fmt(whole), fmt(search), rounds, 1e3 * rounds / max(n_rows, 1), float(np.median(host)) / float(np.median(whole))), flush=True)
    del dl
