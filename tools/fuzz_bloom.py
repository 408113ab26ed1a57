#!/usr/bin/env python3
"""tools/fuzz_bloom.py [n_cases] [seed] [--dry] [--case CASE_SEED] — randomised differential sweep of the Bloom filters on the device (ntcard_amd/bloom.py:
BloomFilter, CountingBloomFilter, BlockedBloomFilter) against tests/bloom_model.py, cbloom_model.py and bbloom_model.py.

A case draws the kind; the action — insert every second sequence and query all, the counting filter's profile, its solid insert into a plain or into a
blocked filter, or insert and query of given h_0 values; k, weighted to 1, 2, 31 .. 33, 63 .. 65, 127 .. 129, 255 .. 257, 599 and 600; the strand; 1 .. 32
hashes; m from small primes, powers of two and their neighbours (a blocked filter: blocks); the address of the first base modulo 16 and the first offset;
and a layout of sequences: lengths around k, boundaries at multiples of 4096 +- 1, runs of empty sequences, 0 .. 5 % non-base bytes, lower case and U.  A
case stays below 40 000 positions.  Every case is a function of its CASE_SEED alone: the first mismatch prints the case's parameters, that seed among
them, exits 1 and starts nothing more on the device; `--case CASE_SEED` runs that case alone.

--dry lists the drawn cases, one JSON object per line with the sequences, positions and windows of each, without torch and without a device.
SHORT_RUN is the run the test suite makes (tests/test_fuzz_bloom_host.py: what it draws; tests/test_bloom_limits_gpu.py: the run itself)."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

import bbloom_model as bb
import bloom_model as bm
import cbloom_model as cm
import strand_model as sm

SHORT_RUN = (48, 22)  # (n_cases, seed) of the suite's run: every kind, action and strand, a k >= 599 and a k <= 2 (tests/test_fuzz_bloom_host.py)
MAX_POSITIONS = 40_000
KINDS = {"plain": "BloomFilter", "counting": "CountingBloomFilter", "blocked": "BlockedBloomFilter"}
ACTIONS = {"plain": ("insert_query", "hashes"), "blocked": ("insert_query", "hashes"),
           "counting": ("insert_query", "profile", "solid_plain", "solid_blocked", "hashes")}
STRANDS = ("canonical", "forward", "reverse")
SIZES = (1, 2, 3, 7, 8, 9, 31, 32, 33, 61, 64, 67, 509, 512, 521, 4093, 4096, 4099, 65521, 65536, 65537, (1 << 20) - 3, 1 << 20, (1 << 20) + 7)
BLOCKS = (1, 2, 3, 7, 8, 9, 31, 64, 127, 1000)
BASES = np.frombuffer(b"ACGTU", dtype=np.uint8)
NON_BASES = np.frombuffer(b"NnRYKM.-*", dtype=np.uint8)


def draw_k(r):
    return r.choice([1, 2, r.randint(31, 33), r.randint(63, 65), r.randint(127, 129), r.randint(255, 257), 599, 600, r.randint(3, 200)])


def draw_size(r, kind):
    return 512 * r.choice(BLOCKS) if kind == "blocked" else r.choice(SIZES)


def draw_lengths(r, k):
    """the lengths of the sequences, fewer than MAX_POSITIONS positions in all"""
    lens, total = [], 0
    for _ in range(r.choice([1, 3, 10, 40, 120])):
        how = r.random()
        if how < 0.3:
            n = max(0, k + r.randint(-2, 2))
        elif how < 0.5:  # up to a multiple of 4096, one less or one more: the next sequence starts on a seam of the block grid or beside it
            n = max(0, (-total) % 4096 + 4096 * r.choice([0, 0, 1]) + r.randint(-1, 1))
        elif how < 0.6:
            lens += [0] * r.choice([1, 5, 70, 300])
            continue
        elif how < 0.8:
            n = r.randint(0, 3 * k + 50)
        else:
            n = r.randint(100, 3000)
        if total + n >= MAX_POSITIONS:
            break
        lens.append(n)
        total += n
    if r.random() < 0.9 and total + 2 * k + 500 < MAX_POSITIONS:  # most cases hold a sequence that is certainly long enough for a window
        lens.insert(r.randint(0, len(lens)), k + r.randint(0, k + 500))
    return lens


def draw(case_seed):
    """the parameters of a case: a function of case_seed alone"""
    r = random.Random(case_seed)
    kind = r.choice(["plain", "counting", "counting", "blocked"])
    p = {"case_seed": case_seed, "kind": kind, "action": r.choice(ACTIONS[kind]), "k": draw_k(r), "strand": r.choice(STRANDS), "n_hash": r.randint(1, 32)}
    p["m"] = draw_size(r, kind)
    p["lead"], p["first"] = r.randint(0, 15), r.choice([0, 1, 5, 16, 33])
    p["min_count"] = r.choice([1, 1, 2, 3, 5, 255])
    p["repeat"] = r.choice([1, 1, 2])  # the counting filter of a profile or a solid insert sees the input that often
    if p["action"] in ("solid_plain", "solid_blocked"):
        p["into_m"] = draw_size(r, "blocked" if p["action"] == "solid_blocked" else "plain")
        p["into_n_hash"] = r.randint(1, 32)
    if p["action"] == "hashes":
        p["n_values"] = r.choice([1, 255, 256, 257, 5000])
    else:
        p["lens"] = draw_lengths(r, p["k"])
        p["p_bad"] = r.choice([0.0, 0.0, 0.0005, 0.005, 0.05])
        p["p_low"] = r.choice([0.0, 0.1, 0.5])
    return p


def sequences(p):
    """the case's sequences (a function of its seed and lengths)"""
    rng = np.random.default_rng(p["case_seed"])
    n = sum(p["lens"])
    flat = BASES[rng.integers(0, BASES.size, size=n)]
    flat = np.where(rng.random(n) < p["p_low"], flat | 0x20, flat).astype(np.uint8)
    if p["p_bad"]:
        flat = np.where(rng.random(n) < p["p_bad"], NON_BASES[rng.integers(0, NON_BASES.size, size=n)], flat).astype(np.uint8)
    cuts = np.concatenate([[0], np.cumsum(p["lens"])]).astype(np.int64)
    return [flat[cuts[i]: cuts[i + 1]].tobytes() for i in range(len(p["lens"]))]


def values(p):
    """the case's given h_0 values: (inserted, asked) — some inserted values more than once, the asked ones half inserted and half not"""
    rng = np.random.default_rng(p["case_seed"])
    h0 = rng.integers(0, 2**64, size=p["n_values"], dtype=np.uint64)
    half = h0.size // 2
    if half and rng.random() < 0.5:
        h0[half:] = h0[rng.integers(0, half, size=h0.size - half)]
    asked = np.concatenate([h0[: half + 1], rng.integers(0, 2**64, size=h0.size, dtype=np.uint64)])
    return h0, asked


def census(p):
    """-> (sequences, positions, windows) of a case, host only; given values count as one window each"""
    if p["action"] == "hashes":
        return 0, 0, p["n_values"]
    seqs = sequences(p)
    return len(seqs), sum(map(len, seqs)), int(sum(int(cm.window_starts(s, p["k"]).sum()) for s in seqs))


def put(seqs, lead, first):
    """the sequences behind one another on the device, the first base `first` bytes behind the tensor's start and at `lead` modulo 16 -> (tensor, offsets)"""
    import torch
    pad = (lead - first) % 16
    host = np.frombuffer(b"#" * (pad + first) + b"".join(seqs) + b"#", dtype=np.uint8).copy()
    d = torch.from_numpy(host).cuda()[pad:]
    assert (d.data_ptr() + first) % 16 == lead
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[0] = first
    offs[1:] = first + np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return d, offs


def image_model(kind, h0, n_hash, k, m, into=None):
    if kind == "blocked":
        return bb.image_of(h0, n_hash, k, m, into)
    if kind == "counting":
        return cm.counters_of(h0, n_hash, k, m, into)
    return bm.image_of(bm.positions(h0, n_hash, k, m), m, into)


def image_of(f):
    return f.counters() if hasattr(f, "counters") else f.bytes()


def run(p, nt):
    """one case on the device against the models -> what differs, or None"""
    kind, k, n_hash, m, strand, st = p["kind"], p["k"], p["n_hash"], p["m"], p["strand"], sm.STRANDS[p["strand"]]
    f = getattr(nt, KINDS[kind])(m, n_hash, k, strand)
    if p["action"] == "hashes":
        h0, asked = values(p)
        f.insert_hashes(h0)
        want = image_model(kind, h0, n_hash, k, m)
        if not np.array_equal(image_of(f), want):
            return "the image after insert_hashes"
        if kind == "counting":
            ok = np.array_equal(f.counts_of_hashes(asked), cm.counts(want, asked, n_hash, k))
        elif kind == "blocked":
            ok = np.array_equal(f.query_hashes(asked), bb.test_values(want, asked, n_hash, k, m))
        else:
            ok = np.array_equal(f.query_hashes(asked), bm.bits_set(want, bm.positions(asked, n_hash, k, m)).all(axis=1))
        return None if ok else "the answers for given values"
    seqs = sequences(p)
    d, offs = put(seqs, p["lead"], p["first"])
    if p["action"] == "insert_query":
        ins = seqs[::2] if len(seqs) > 1 else seqs
        v = cm.all_values(ins, k, st)
        di, oi = put(ins, p["lead"], p["first"])
        if f.insert(di, oi) != v.size:
            return "the windows inserted"
        want = image_model(kind, v, n_hash, k, m)
        if not np.array_equal(image_of(f), want):
            return "the image after insert"
        if kind == "counting":
            w, h = f.query(d, offs, p["min_count"])
            mw, mh = cm.query(want, seqs, k, st, n_hash, p["min_count"])
        else:
            w, h = f.query(d, offs)
            mw, mh = (bb if kind == "blocked" else bm).query(want, seqs, k, st, n_hash, m)
        return None if np.array_equal(w, mw) and np.array_equal(h, mh) else "the query's windows or hits"
    # the counting filter's own actions
    v = cm.all_values(seqs, k, st)
    cnt = None
    for _ in range(p["repeat"]):
        if f.insert(d, offs) != v.size:
            return "the windows inserted"
        cnt = cm.counters_of(v, n_hash, k, m, into=cnt)
    if not np.array_equal(f.counters(), cnt):
        return "the counters after insert"
    if p["action"] == "profile":
        return None if np.array_equal(f.profile(d, offs), cm.profile(cnt, seqs, k, st, n_hash)) else "the profile"
    solid = cm.solid_values(cnt, seqs, k, st, n_hash, p["min_count"])
    if p["action"] == "solid_plain":
        into = nt.BloomFilter(p["into_m"], p["into_n_hash"], k, strand)
        n = f.solid(d, offs, p["min_count"], into)
        want = image_model("plain", solid, p["into_n_hash"], k, p["into_m"])
    else:
        into = nt.BlockedBloomFilter(p["into_m"], p["into_n_hash"], k, strand)
        n = into.insert_solid(f, d, offs, p["min_count"])
        want = image_model("blocked", solid, p["into_n_hash"], k, p["into_m"])
    if n != solid.size:
        return "the windows that passed"
    return None if np.array_equal(into.bytes(), want) else "the image after the solid insert"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("n_cases", nargs="?", type=int, default=300)
    ap.add_argument("seed", nargs="?", type=int, default=1)
    ap.add_argument("--dry", action="store_true", help="list the drawn cases; no torch, no device")
    ap.add_argument("--case", type=int, default=None, help="run the case of this case_seed alone")
    a = ap.parse_args()
    master = random.Random(a.seed)
    seeds = [a.case] if a.case is not None else [master.getrandbits(48) for _ in range(a.n_cases)]
    if a.dry:
        for s in seeds:
            p = draw(s)
            p["n_seqs"], p["positions"], p["windows"] = census(p)
            p.pop("lens", None)
            print(json.dumps(p))
        return 0
    import torch
    torch.cuda.init()
    import ntcard_amd as nt
    for i, s in enumerate(seeds):
        p = draw(s)
        what = run(p, nt)
        if what:
            print(f"MISMATCH in {what}: case {i} {json.dumps(p)}\nrerun: tools/fuzz_bloom.py --case {s}", flush=True)
            return 1
        if i % 10 == 0:
            print("ok case", i, json.dumps({key: val for key, val in p.items() if key != "lens"}), flush=True)
    print(f"fuzz bloom OK: {len(seeds)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
