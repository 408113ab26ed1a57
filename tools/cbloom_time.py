#!/usr/bin/env python3
"""The timing protocol of the counting Bloom filter tools (DESIGN.md §4 "Counting filters and solid k-mers"; results: profiles/cbloom.txt).

The batch of tools/bloom_time.py: genome-like reads from ntc_gen_reads_device (dist 1), packed so that stride == read_len, uniform offsets; k = 32, three
hashes; m from ntc_bloom_size at fpr 0.01 for the batch's distinct k-mers as the engine estimates them (F0) — counters here, bits for the plain filter it is
set against.  Timed, each the median of the in-process repeats between two events on the stream:
  insert      into zeroed counters (the memset is outside the events)
  again       the same batch into the counters the first insert left
  query       min_count 2, the same batch; profile: the same batch, one byte per position
  threshold   min_count 2 into a plain filter of m bits; next to it a plain device copy of the m counter bytes
  hist        the 256 bins; next to the same copy
  solid       min_count 2 into a zeroed plain filter of ntc_bloom_size(F0 - f_1) bits
and next to insert / query the plain filter's ntc_bloom_insert_device / ntc_bloom_query_device on the same batch and the same m (bits).
The calls are synchronous and upload the offsets (8 B per sequence) themselves: that copy is inside the events, as it is inside every caller's call.

  python tools/cbloom_time.py [--reads 10000000] [--read-len 150] [--repeats 9] [--hashes 3] [--m COUNTERS] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--fpr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--m", type=int, default=0, help="this many counters (and bits of the plain filter) instead of ntc_bloom_size's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ntcard_amd as nt
    from ntcard_amd import _abi

    if not torch.cuda.is_available():
        sys.exit("cbloom_time.py measures on the GPU: no HIP device")  # (no number comes from anywhere else)
    dev = torch.device("cuda:0")
    n, L, k, c = args.reads, args.read_len, args.k, args.min_count
    stride = (L + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    lib = _abi.lib()

    slots = torch.empty(n * stride + 16, dtype=torch.uint8, device=dev)
    nt.gen_reads_device(slots.data_ptr(), args.seed, 0, n, L, stride, 1, genome_len=100_000_000, stream=stream)
    bases = slots[: n * stride].view(n, stride)[:, :L].contiguous().view(-1)
    del slots
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    offp = offsets.ctypes.data_as(C.c_void_p)

    # F0 and f_1 .. of the batch: the engine's estimate over the same reads (bit-identical bases) in the tiled layout
    tiles = torch.empty(nt.tiled_bytes(n, L), dtype=torch.uint8, device=dev)
    nt.gen_reads_tiled_device(tiles.data_ptr(), args.seed, 0, n, L, 1, genome_len=100_000_000, stream=stream)
    r_bits, s_bits = 27, 7
    with nt.Engine([k], r_bits=r_bits, s_bits=s_bits, device=0, stream=stream, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_tiled_device(tiles.data_ptr(), n, L)
        _, ph, f1 = e.finish()
    F0, f = nt.estimate(ph[0], r_bits, s_bits, 1000)
    del tiles
    torch.cuda.empty_cache()
    n_solid = max(int(F0) - int(sum(f[1:c])), 1)

    m = args.m or nt.bloom_size(int(F0), args.fpr, args.hashes)
    cf = nt.CountingBloomFilter(m, args.hashes, k)
    pf = nt.BloomFilter(m, args.hashes, k)
    sf = nt.BloomFilter.for_distinct(n_solid, args.fpr, args.hashes, k)
    thr = nt.BloomFilter(m, args.hashes, k)
    copy_to = torch.empty_like(cf.filter)
    per_seq = torch.empty((2, n), dtype=torch.int32, device=dev)
    prof = torch.empty(n * L, dtype=torch.uint8, device=dev)
    hist = np.zeros(256, dtype=np.uint64)
    st = C.c_void_p(stream)

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1), out

    def plain_query():
        _abi.check(lib.ntc_bloom_query_device(0, st, pf.filter.data_ptr(), m, pf.n_hash, k, 0, bases.data_ptr(), offp, n, per_seq[0].data_ptr(), per_seq[1].data_ptr()))

    def query():
        _abi.check(lib.ntc_cbloom_query_device(0, st, cf.filter.data_ptr(), m, cf.n_hash, k, 0, bases.data_ptr(), offp, n, c, per_seq[0].data_ptr(), per_seq[1].data_ptr()))

    def profile():
        _abi.check(lib.ntc_cbloom_profile_device(0, st, cf.filter.data_ptr(), m, cf.n_hash, k, 0, bases.data_ptr(), offp, n, prof.data_ptr()))

    def threshold():
        _abi.check(lib.ntc_cbloom_threshold_device(0, st, cf.filter.data_ptr(), m, c, thr.filter.data_ptr()))

    def histogram():
        _abi.check(lib.ntc_cbloom_hist_device(0, st, cf.filter.data_ptr(), m, hist.ctypes.data_as(C.c_void_p)))

    names = ["plain insert, zeroed filter", "plain insert again", "plain query", "insert, zeroed counters", "insert again", f"query, min_count {c}", "profile",
             f"threshold at {c}", "hist", "copy of the m counter bytes", f"solid insert at {c}, zeroed filter"]
    t = {name: [] for name in names}
    cf.insert(bases, offsets)  # warm-up: code objects, the allocator
    pf.insert(bases, offsets)
    query(), plain_query(), profile(), threshold(), histogram()
    cf.solid(bases, offsets, c, sf)
    windows = passed = 0
    for _ in range(args.repeats):
        for x in (cf, pf, sf):
            x.filter.zero_()
        torch.cuda.synchronize()
        t[names[0]].append(timed(lambda: pf.insert(bases, offsets))[0])
        t[names[1]].append(timed(lambda: pf.insert(bases, offsets))[0])
        t[names[2]].append(timed(plain_query)[0])
        ms, windows = timed(lambda: cf.insert(bases, offsets))
        t[names[3]].append(ms)
        first = cf.filter.clone()
        t[names[4]].append(timed(lambda: cf.insert(bases, offsets))[0])
        cf.filter.copy_(first)  # the counters of ONE pass over the batch are what the rest reads
        del first
        torch.cuda.synchronize()
        t[names[5]].append(timed(query)[0])
        t[names[6]].append(timed(profile)[0])
        t[names[7]].append(timed(threshold)[0])
        t[names[8]].append(timed(histogram)[0])
        t[names[9]].append(timed(lambda: copy_to.copy_(cf.filter))[0])
        ms, passed = timed(lambda: cf.solid(bases, offsets, c, sf))
        t[names[10]].append(ms)
    hits = int(per_seq[1].sum(dtype=torch.int64))

    med = statistics.median
    lines = [
        f"reads {n} x {L} bp (genome-like, seed {args.seed}), k = {k}, hashes = {args.hashes}, fpr {args.fpr}",
        f"windows (F1) {int(f1[0])}   F0 (the engine's estimate) {int(F0)}   m {m} counters ({cf.filter.numel() / 2**20:.1f} MiB; the plain filter of m bits: {pf.filter.numel() / 2**20:.1f} MiB)",
        f"counters not 0: {m - int(hist[0])}   saturated: {int(hist[255])}   false 'count >= 1' rate {((m - int(hist[0])) / m) ** args.hashes:.5f}   "
        f"false 'count >= {c}' rate {(int(hist[c:].sum()) / m) ** args.hashes:.5f}",
        f"windows with count >= {c}: {hits} by the query, {passed} by the solid insert (of {windows}); the solid filter: {sf.m_bits} bits for {n_solid} k-mers (F0 minus the f_i below {c})",
        f"median of {args.repeats} (min .. max), ms; G k-mers/s = windows / median (copy, threshold, hist: GB/s of counter bytes)",
    ]
    for name in names:
        v = t[name]
        rate = f"{m / med(v) / 1e6:8.1f} GB/s" if name in (names[7], names[8], names[9]) else f"{windows / med(v) / 1e6:8.2f}"
        lines.append(f"  {name:36s} {med(v):10.3f}  ({min(v):.3f} .. {max(v):.3f})   {rate}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
