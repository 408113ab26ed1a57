#!/usr/bin/env python3
"""The timing protocol of the blocked Bloom filters next to the plain ones (DESIGN.md §4 "Blocked filters"; results: profiles/bbloom.txt).

The batch and the method are tools/bloom_time.py's: genome-like reads from ntc_gen_reads_device (dist 1), packed so that stride == read_len; k = 32, three
hashes; each figure the median of nine in-process repeats between two events on the stream.  Both filters are sized for fpr 0.01 from the engine's own F0
of the same reads: ntc_bloom_size for the plain filter, ntc_bbloom_size for the blocked one.  Rows, all from this one process:
  plain    insert into a zeroed filter / insert again (every bit found set: hashing and loads, no atomics) / query
  blocked  the same three
  solid    the second stage at min_count 2 from one counting filter of the batch (ntc_bloom_size(F0) counters), into a zeroed plain filter and into a
           zeroed blocked one, both sized for F0 - f_1 of the engine's estimate
  hist     ntc_bbloom_hist_device over the blocked filter, next to a device-to-device copy of the same bytes
and the realised false positive rate of both filters: (popcount / m_bits)^h, and for the blocked one the mean over its blocks of (set bits / 512)^h from the
block histogram — which is the rate a foreign k-mer meets — next to ntc_bbloom_fpr's prediction.

  python tools/bbloom_time.py [--reads 10000000] [--read-len 150] [--repeats 9] [--hashes 3] [--out FILE]
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ntcard_amd as nt
    from ntcard_amd import _abi

    if not torch.cuda.is_available():
        sys.exit("bbloom_time.py measures on the GPU: no HIP device")  # (no number comes from anywhere else)
    dev = torch.device("cuda:0")
    n, L, k, H = args.reads, args.read_len, args.k, args.hashes
    stride = (L + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream
    lib = _abi.lib()

    slots = torch.empty(n * stride + 16, dtype=torch.uint8, device=dev)
    nt.gen_reads_device(slots.data_ptr(), args.seed, 0, n, L, stride, 1, genome_len=100_000_000, stream=stream)
    bases = slots[: n * stride].view(n, stride)[:, :L].contiguous().view(-1)
    del slots
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    off_p = offsets.ctypes.data_as(C.c_void_p)

    # F0 and f_1: the engine's estimate for the same reads (bit-identical bases) in the tiled layout
    tiles = torch.empty(nt.tiled_bytes(n, L), dtype=torch.uint8, device=dev)
    nt.gen_reads_tiled_device(tiles.data_ptr(), args.seed, 0, n, L, 1, genome_len=100_000_000, stream=stream)
    r_bits, s_bits = 27, 7
    with nt.Engine([k], r_bits=r_bits, s_bits=s_bits, device=0, stream=stream, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_tiled_device(tiles.data_ptr(), n, L)
        _, ph, f1 = e.finish()
    F0, f = nt.estimate(ph[0], r_bits, s_bits, 1000)
    F0, n_solid = int(F0), max(int(F0) - int(f[1]), 1)
    del tiles
    torch.cuda.empty_cache()

    plain = nt.BloomFilter.for_distinct(F0, args.fpr, H, k)
    blocked = nt.BlockedBloomFilter.for_distinct(F0, args.fpr, H, k)
    out = torch.empty((2, n), dtype=torch.int32, device=dev)

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        res = fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1), res

    def query_of(f, call):  # timed at the C call: the result arrays stay on the device, outside the events
        def q():
            _abi.check(call(0, C.c_void_p(stream), f.filter.data_ptr(), f.m_bits, f.n_hash, f.k, 0, bases.data_ptr(), off_p, n, out[0].data_ptr(), out[1].data_ptr()))
        return q

    rows, windows = [], None
    for name, f, call in (("plain", plain, lib.ntc_bloom_query_device), ("blocked", blocked, lib.ntc_bbloom_query_device)):
        query = query_of(f, call)
        f.insert(bases, offsets)  # warm-up: code objects, the allocator
        query()
        ins, again, qry = [], [], []
        for _ in range(args.repeats):
            f.filter.zero_()
            torch.cuda.synchronize()
            t, windows = timed(lambda: f.insert(bases, offsets))
            ins.append(t)
            t, w2 = timed(lambda: f.insert(bases, offsets))
            again.append(t)
            assert w2 == windows
            t, _ = timed(query)
            qry.append(t)
            w, hits = int(out[0].sum(dtype=torch.int64)), int(out[1].sum(dtype=torch.int64))
            assert w == windows and hits == windows  # everything that was inserted is found
        rows += [(f"{name}: insert, zeroed filter", ins), (f"{name}: insert again (loads only)", again), (f"{name}: query", qry)]

    # the solid inserts: one counting filter of the batch, two destinations
    cbf = nt.CountingBloomFilter.for_distinct(F0, args.fpr, H, k)
    cbf.insert(bases, offsets)
    s_plain = nt.BloomFilter.for_distinct(n_solid, args.fpr, H, k)
    s_blocked = nt.BlockedBloomFilter.for_distinct(n_solid, args.fpr, H, k)
    passed = {}
    for name, dst, call in (("solid (min_count 2) into a plain filter", s_plain, lib.ntc_bloom_insert_solid_device),
                            ("solid (min_count 2) into a blocked filter", s_blocked, lib.ntc_bbloom_insert_solid_device)):
        cnt = C.c_uint64(0)

        def solid():
            _abi.check(call(0, C.c_void_p(stream), dst.filter.data_ptr(), dst.m_bits, dst.n_hash, cbf.filter.data_ptr(), cbf.m_bits, cbf.n_hash, 2, k, 0,
                            bases.data_ptr(), off_p, n, C.byref(cnt)))
        solid()  # warm-up
        ts = []
        for _ in range(args.repeats):
            dst.filter.zero_()
            torch.cuda.synchronize()
            t, _ = timed(solid)
            ts.append(t)
        passed[name] = int(cnt.value)
        rows.append((name, ts))
    assert len(set(passed.values())) == 1  # the same windows pass into either destination
    del cbf, s_plain, s_blocked
    torch.cuda.empty_cache()

    # the histogram next to a copy of the same bytes
    blocked.block_hist()
    copy = torch.empty_like(blocked.filter)
    hs, cp = [], []
    for _ in range(args.repeats):
        t, hist = timed(blocked.block_hist)
        hs.append(t)
        t, _ = timed(lambda: copy.copy_(blocked.filter))
        cp.append(t)
    rows += [("blocked: block histogram", hs), ("device copy of the blocked filter", cp)]

    pop_p, pop_b = plain.popcount(), blocked.popcount()
    v = np.arange(513, dtype=np.float64) / 512.0
    fpr_hist = float((hist.astype(np.float64) * v ** H).sum() / blocked.n_blocks)
    assert int((hist * np.arange(513, dtype=np.uint64)).sum()) == pop_b  # the histogram and the popcount count the same bits

    med = statistics.median
    lines = [
        f"reads {n} x {L} bp (genome-like, seed {args.seed}), k = {k}, hashes = {H}, fpr {args.fpr}",
        f"windows (F1) {int(f1[0])}   F0 (the engine's estimate) {F0}   F0 - f_1 (solid at 2) {n_solid}   windows that pass at min_count 2: {list(passed.values())[0]}",
        f"plain   m_bits {plain.m_bits} ({plain.filter.numel() / 2**20:.1f} MiB)   popcount {pop_p}   occupancy {pop_p / plain.m_bits:.4f}   "
        f"realised fpr (popcount / m)^h {(pop_p / plain.m_bits) ** H:.5f}",
        f"blocked m_bits {blocked.m_bits} ({blocked.filter.numel() / 2**20:.1f} MiB, {blocked.m_bits / plain.m_bits:.4f} of the plain)   popcount {pop_b}   "
        f"occupancy {pop_b / blocked.m_bits:.4f}   (popcount / m)^h {(pop_b / blocked.m_bits) ** H:.5f}   realised fpr from the block histogram {fpr_hist:.5f}   "
        f"ntc_bbloom_fpr(F0) {nt.bbloom_fpr(F0, blocked.m_bits, H):.5f}",
        f"median of {args.repeats} (min .. max), ms; G k-mers/s = windows / median",
    ]
    for name, t in rows:
        lines.append(f"  {name:44s} {med(t):10.3f}  ({min(t):.3f} .. {max(t):.3f})   {windows / med(t) / 1e6:8.2f}")
    by = {name: med(t) for name, t in rows}
    for what in ("insert, zeroed filter", "insert again (loads only)", "query"):
        lines.append(f"blocked / plain, {what}: {by['blocked: ' + what] / by['plain: ' + what]:.3f}")
    lines.append(f"blocked / plain, solid: {by['solid (min_count 2) into a blocked filter'] / by['solid (min_count 2) into a plain filter']:.3f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
