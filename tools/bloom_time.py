#!/usr/bin/env python3
"""The timing protocol of the Bloom filter tools (DESIGN.md §4 "Bloom filters"; results: profiles/bloom.txt).

One batch of genome-like reads from ntc_gen_reads_device (dist 1, the generator of bench.py), packed so that stride == read_len and the offsets are
uniform; k = 32, three hashes; m from ntc_bloom_size at fpr 0.01 for the batch's distinct k-mers, taken from this project's own estimate: the F0 of an
Engine that counted the same reads.  Timed, each the median of nine in-process repeats between two events on the stream:
  insert   into a zeroed filter (the memset is outside the events)
  again    the same batch into the filter the first insert left: every bit is found set, so the pass is hashing and loads, no atomics
  query    the same batch
and next to them the parent's K1h + K1f hash time for the same reads in the tiled layout (ntc_kernel_time + ntc_fixup_time): the cost of the walk alone.
The Bloom calls are synchronous and upload the offsets (8 B per sequence) themselves: that copy is inside the events, as it is inside every caller's call.

  python tools/bloom_time.py [--reads 10000000] [--read-len 150] [--repeats 9] [--hashes 3] [--m-bits BITS] [--out FILE]
"""
import argparse
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
    ap.add_argument("--m-bits", type=int, default=0, help="a filter of this size instead of ntc_bloom_size's: a tiny one stays in the caches, which leaves the walk's own time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ntcard_amd as nt

    if not torch.cuda.is_available():
        sys.exit("bloom_time.py measures on the GPU: no HIP device")  # (no number comes from anywhere else)
    dev = torch.device("cuda:0")
    n, L, k = args.reads, args.read_len, args.k
    stride = (L + 3) & ~3
    stream = torch.cuda.current_stream().cuda_stream

    # the reads: row slots from the generator, packed to stride == read_len (the generator wants stride % 4 == 0 and fills the rest of a slot with 'A')
    slots = torch.empty(n * stride + 16, dtype=torch.uint8, device=dev)
    nt.gen_reads_device(slots.data_ptr(), args.seed, 0, n, L, stride, 1, genome_len=100_000_000, stream=stream)
    bases = slots[: n * stride].view(n, stride)[:, :L].contiguous().view(-1)
    del slots
    offsets = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)

    # F0 and the walk's own time: the same reads (bit-identical bases) in the tiled layout through K1h + K1f
    tiles = torch.empty(nt.tiled_bytes(n, L), dtype=torch.uint8, device=dev)
    nt.gen_reads_tiled_device(tiles.data_ptr(), args.seed, 0, n, L, 1, genome_len=100_000_000, stream=stream)
    r_bits, s_bits = 27, 7
    hash_ms = []
    with nt.Engine([k], r_bits=r_bits, s_bits=s_bits, device=0, stream=stream, flags=nt.FLAG_REQUIRE_TILED) as e:
        e.submit_tiled_device(tiles.data_ptr(), n, L)  # warm-up
        e.sync()
        for _ in range(args.repeats):
            e.reset()
            e.set_profiling(True)
            e.submit_tiled_device(tiles.data_ptr(), n, L)
            e.sync()
            hash_ms.append(e.kernel_time()[0] + e.fixup_time())
        _, ph, f1 = e.finish()
    F0, _ = nt.estimate(ph[0], r_bits, s_bits, 1000)
    del tiles
    torch.cuda.empty_cache()

    f = nt.BloomFilter(args.m_bits, args.hashes, k) if args.m_bits else nt.BloomFilter.for_distinct(int(F0), args.fpr, args.hashes, k)

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1), out

    # the query is timed at the C call: the result arrays stay on the device, outside the events
    import ctypes as C
    from ntcard_amd import _abi
    out = torch.empty((2, n), dtype=torch.int32, device=dev)

    def query():
        _abi.check(_abi.lib().ntc_bloom_query_device(0, C.c_void_p(stream), f.filter.data_ptr(), f.m_bits, f.n_hash, f.k, 0, bases.data_ptr(),
                                                     offsets.ctypes.data_as(C.c_void_p), n, out[0].data_ptr(), out[1].data_ptr()))

    f.insert(bases, offsets)  # warm-up: code objects, the allocator
    query()
    ins, again, qry = [], [], []
    windows = hits = None
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
    pop = f.popcount()

    med = statistics.median
    lines = [
        f"reads {n} x {L} bp (genome-like, seed {args.seed}), k = {k}, hashes = {args.hashes}, fpr {args.fpr}",
        f"windows (F1) {int(f1[0])}   F0 (the engine's estimate) {int(F0)}   m_bits {f.m_bits} ({f.filter.numel() / 2**20:.1f} MiB)",
        f"popcount {pop}   occupancy {pop / f.m_bits:.4f}   implied fpr {(pop / f.m_bits) ** args.hashes:.5f}",
        f"median of {args.repeats} (min .. max), ms; G k-mers/s = windows / median",
    ]
    for name, v in (("K1h + K1f hash (parent)", hash_ms), ("insert, zeroed filter", ins), ("insert again (loads only)", again), ("query", qry)):
        lines.append(f"  {name:28s} {med(v):10.3f}  ({min(v):.3f} .. {max(v):.3f})   {windows / med(v) / 1e6:8.2f}")
    lines.append(f"insert - insert again = {med(ins) - med(again):.3f} ms: what the atomics of a first build cost over hashing + loads")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
