#!/usr/bin/env python3
"""tools/sig_algebra_time.py — what the set algebra and the spectrum of signatures cost on the device (profiles/signature.txt, "Set algebra and spectrum").
Sizes are those of tools/sig_sort_time.py: 407 213 and 6 534 307 pairs, signature-shaped hashes, counts that are mostly 1.
(1) ntc_signature_union_device of two and of sixteen lists whose entries add up to the size (drawn from a pool of 3/4 of it: many hashes are in several
    lists), against numpy on the host (np.unique of the concatenation, np.add.at), against the only route the parent commit has — ntc_signature_inject_device of every list
    into a signature engine, then ntc_signature_device — and against a device copy of the pairs the call gathers.
(2) ntc_signature_select_device of a signature of that size against one and against 64 references as long as itself: references that each hold a random
    half of it (a lane leaves at the first reference that lacks its hash) and references that hold all of it (every lane searches every reference), against
    np.isin per reference on the host — skipped above --host-work entries x references — and a device copy of A's pairs.
(3) ntc_signature_hist_device of that many counts, against np.bincount and a device copy of the counts.
Every device figure is wall clock round the synchronous call (scratch allocation, launches and waits included), the MEDIAN of --reps repeats behind one
warm-up, with min .. max behind it; host figures are the median of --host-reps without one."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--host-work", type=int, default=30_000_000, help="np.isin is timed up to this many entries x references")
ap.add_argument("--sizes", default="407213,6534307")
ap.add_argument("--only", default="1,2,3")
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ntcard_amd as nt  # noqa: E402
import sig_algebra_model as model  # noqa: E402

only = set(int(x) for x in args.only.split(","))
fmt = lambda xs: "%.3f (%.3f .. %.3f)" % (float(np.median(xs)), min(xs), max(xs))
print("device: %s; median of %d repeats (min .. max) behind one warm-up, ms; host: median of %d" % (torch.cuda.get_device_name(0), args.reps, args.host_reps), flush=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn):
    fn()
    return [wall(fn) for _ in range(args.reps)]


def host_timed(fn):
    return [wall(fn) for _ in range(args.host_reps)]


def sig_shaped(n, rng):
    """n distinct signature-shaped hashes (ntComp's two patterns at s = 7 in front, random bits behind), ascending uint64"""
    r = rng.integers(0, 2**64, size=n + n // 8, dtype=np.uint64)
    one = (r & np.uint64(2**56 - 1)) | np.uint64(1 << 56)
    two = (r & np.uint64(2**57 - 1)) | np.uint64(63 << 57)
    h = np.unique(np.where(rng.random(r.size) < 0.5, one, two))
    return np.sort(rng.choice(h, size=n, replace=False)) if h.size > n else h


def counts_like(n, rng):
    return np.minimum(rng.geometric(0.8, size=n), 2**31).astype(np.uint32)


def dev64(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def dev32(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


def copy_ms(tensors):
    outs = [torch.empty_like(t) for t in tensors]
    return timed(lambda: [o.copy_(t) for o, t in zip(outs, tensors)])


sizes = [int(x) for x in args.sizes.split(",")]
rng = np.random.default_rng(5)

if 1 in only:
    print("\n(1) union: lists whose entries add up to `pairs`; result = the distinct hashes")
    for total in sizes:
        for n_lists in (2, 16):
            each = total // n_lists
            pool = sig_shaped(each * n_lists * 3 // 4, rng)
            lists = [np.sort(rng.choice(pool, size=each + (total - each * n_lists if i == 0 else 0), replace=False)) for i in range(n_lists)]
            counts = [counts_like(h.size, rng) for h in lists]
            dl, dc = [dev64(h) for h in lists], [dev32(c) for c in counts]
            ptrs, cptrs, ns = [t.data_ptr() for t in dl], [t.data_ptr() for t in dc], [h.size for h in lists]
            want = model.union(lists, counts)
            h, c, n = nt.signature_union_device(ptrs, cptrs, ns)
            assert n == want[0].size and np.array_equal(h.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(c.cpu().numpy().view(np.uint32), want[1])
            dev = timed(lambda: nt.signature_union_device(ptrs, cptrs, ns))
            host = host_timed(lambda: model.union(lists, counts))
            with nt.Engine([32], r_bits=14, s_bits=7, signature=True) as e:
                def inject_route():
                    e.reset()
                    for p, cp, k in zip(ptrs, cptrs, ns):
                        e.signature_inject((p, k), counts=cp, device=True)
                    return e.signature_device()
                eh, ec, en = inject_route()
                assert en == n and bool((eh == h).all()) and bool((ec == c).all())
                route = timed(inject_route)
            cp = copy_ms(dl + dc)
            print("%9d pairs in %2d lists -> %9d   union %-26s inject + signature_device %-26s numpy %-30s copy of the pairs %s" %
                  (sum(ns), n_lists, n, fmt(dev), fmt(route), fmt(host), fmt(cp)), flush=True)
            del dl, dc, h, c, eh, ec

if 2 in only:
    print("\n(2) select, mode all: A of `pairs` entries with counts; references as long as A")
    for na in sizes:
        a = sig_shaped(na, rng)
        ca = counts_like(a.size, rng)
        others = sig_shaped(na // 2, rng)
        da, dca = dev64(a), dev32(ca)
        d_others = dev64(others)
        for n_refs in (1, 64):
            for what in ("half of A each", "all of A each"):
                if what.startswith("half"):  # (built on the device; these hashes are non-negative as int64, so torch's order is the unsigned one)
                    dr = [torch.sort(torch.cat([da[torch.rand(a.size, device="cuda") < 0.5], d_others]))[0] for _ in range(n_refs)]
                else:
                    dr = [da.clone() for _ in range(n_refs)]
                ptrs, ns = [t.data_ptr() for t in dr], [t.numel() for t in dr]
                call = lambda: nt.signature_select_device(da.data_ptr(), dca.data_ptr(), a.size, ptrs, ns, mode="all")
                h, c, n = call()
                if a.size * n_refs <= args.host_work:
                    refs = [t.cpu().numpy().view(np.uint64) for t in dr]
                    want = model.select(a, ca, refs, "all")
                    assert n == want[0].size and np.array_equal(h.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(c.cpu().numpy().view(np.uint32), want[1])
                    host = fmt(host_timed(lambda: model.select(a, ca, refs, "all")))
                else:
                    host = "not timed (above --host-work)"
                dev = timed(call)
                print("%9d pairs, %2d references, %-15s -> %9d   select %-26s numpy %-30s copy of A's pairs %s" %
                      (a.size, n_refs, what, n, fmt(dev), host, fmt(copy_ms([da, dca]))), flush=True)
                del dr

if 3 in only:
    print("\n(3) hist, cov_max 1000")
    for n in sizes:
        c = counts_like(n, rng)
        d = dev32(c)
        want = model.hist(c, 1000)
        got = nt.signature_hist_device(d.data_ptr(), n, cov_max=1000)
        assert np.array_equal(got[0], want[0]) and int(got[1]) == want[1]
        dev = timed(lambda: nt.signature_hist_device(d.data_ptr(), n, cov_max=1000))
        host = host_timed(lambda: model.hist(c, 1000))
        print("%9d counts   hist %-26s numpy %-30s copy of the counts %s" % (n, fmt(dev), fmt(host), fmt(copy_ms([d]))), flush=True)
