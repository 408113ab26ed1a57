"""k1h_strand_model.py — CPU-side harness of the ONE-STRAND K1h kernels (gen_k1h.Gen(..., strand=1 | 2)): the generated instruction list on the wave
emulator through k1h_model.run_k1h (whose Gen factory is replaced for the duration of a call), and a Python model of what K1f does for a strand launch.
Test infrastructure only.

The one-strand contract (gen_k1h.Gen.flags_and_push_one): one hit-log key per window whose strand value matches one of ntComp's patterns and whose read is
clean around it; candidates near a dirty piece are suspects (never marked as ties); the tie array is written and all zero.  K1f: F1 takes the windows with a
non-base byte back; a suspect counts, with K1h's own counter index, iff its window holds no non-base byte; when a suspect region overflowed, every window of
every dirty-affected block is re-derived from the bytes with the strand's value (fh or rh) instead of the smaller one.  Expected counters and F1 come from
strand_model.model_sketch, built from the oracle's fh / rh.
"""
import contextlib

import numpy as np

import k1h_model as km
import strand_model as sm
from support import ALPHA, gap_mask, key_of, random_reads, tile_array

gen_k1h = km.gen_k1h


@contextlib.contextmanager
def strand_gen(strand):
    """k1h_model.run_k1h builds its program with gen_k1h.Gen(k, sb, gap): for the duration of the block that is the one-strand generator"""
    real = gen_k1h.Gen

    def factory(k, sb_class=7, gap=0):
        return real(k, sb_class, gap, strand=strand)
    gen_k1h.Gen = factory
    try:
        yield
    finally:
        gen_k1h.Gen = real


def run_k1h(strand, *args, **kw):
    with strand_gen(strand):
        return km.run_k1h(*args, **kw)


def k1f_strand_model(reads, read_len, k, r_bits, s_bits, strand, res, gap=0):
    """-> (keys, f1_sub) of K1f behind a one-strand K1h launch (res: run_k1h's result)"""
    dirty, tie, sus, overflow = res["dirty"], res["tie"], res["sus"], res["sus_overflow"]
    assert not tie.any(), "a one-strand kernel leaves the tie array all zero"
    phi = (k - 1) % 16
    NB = ((read_len - 1 + 16 - phi) >> 4) + 1
    Cn = (read_len + 15) // 16
    keys, f1_sub = [], 0
    for r, seq in enumerate(reads):
        t, lane, m = r // 2048, (r % 2048) % 64, (r % 2048) // 64
        for b in range(NB):
            aff = any(0 <= c < Cn and (int(dirty[t, c, lane]) >> m) & 1 for c in (b - 2, b - 1, b))
            if not aff:
                continue  # (a window with a non-base byte lies in a dirty-affected block: asserted through F1 below)
            for e in range(max(16 * b - 16 + phi, k - 1), min(16 * b + phi - 1, len(seq) - 1) + 1):
                ok, fv, rv = km.window_hashes(seq[e - k + 1: e + 1], k, gap)
                if not ok:
                    f1_sub += 1
                elif overflow:  # slow path: every window of a dirty-affected block, the strand's own value
                    kk = key_of(fv if strand == sm.FORWARD else rv, r_bits, s_bits)
                    if kk is not None:
                        keys.append(kk)
    if not overflow:
        for x, t, rw, mark in sus:
            r, w = int(t) * 2048 + (int(rw) & 2047), int(rw) >> 11
            assert not int(mark) & 4, "a one-strand kernel queues no tie items"
            tl, lane, m = r // 2048, (r % 2048) % 64, (r % 2048) // 64
            c0 = w // 16
            for j in range(3):
                if c0 + j < Cn and 16 * j < (w % 16) + k:
                    assert (int(mark) >> (4 + j)) & 1 == (int(dirty[tl, c0 + j, lane]) >> m) & 1, (r, w, j, int(mark))
            ok, fv, rv = km.window_hashes(reads[r][w: w + k], k, gap)
            if not ok:
                continue  # a non-base byte inside the window: nothing (ntHashIterator.hpp:59-86)
            kk = key_of(fv if strand == sm.FORWARD else rv, r_bits, s_bits)
            assert kk is not None or s_bits > 7, (r, w)
            assert (int(mark) & 2 != 0) == (kk is None), (r, w, int(mark))
            if kk is not None:
                assert int(x) == kk, (r, w, int(x), kk)  # K1f's fast path counts K1h's own index
                keys.append(kk)
    return keys, f1_sub


def check(strand, reads, arr, n, read_len, k, r_bits, s_bits, gap, n_waves, tails=None, **kw):
    """run the strand kernel + the K1f model over the reads and compare with strand_model.model_sketch"""
    res = run_k1h(strand, tile_array(arr), n, read_len, k, r_bits=r_bits, n_waves=n_waves, s_bits=s_bits, gap=gap, tails=tails, **kw)
    fk, f1_sub = k1f_strand_model(reads, read_len, k, r_bits, s_bits, strand, res, gap=gap)
    got = np.bincount(np.concatenate([res["keys"], np.array(fk, dtype=np.uint32)]).astype(np.int64), minlength=2 << r_bits).astype(np.uint32) + res["sketch"]
    tc, f1 = sm.model_sketch(reads, [gap_mask(k, gap)], strand, r_bits, s_bits)
    assert res["f1"] - f1_sub == int(f1[0])
    assert np.array_equal(got, tc[0].reshape(-1).astype(np.uint32))
    return res


def run(strand, n, L, k, p_bad=0.0, r_bits=14, n_waves=2, seed=1, s_bits=7, gap=0, **kw):
    arr = random_reads(np.random.default_rng(seed), n, L, p_bad)
    return check(strand, [arr[i].tobytes() for i in range(n)], arr, n, L, k, r_bits, s_bits, gap, n_waves, **kw)


def run_ragged(strand, n, C, k, p_bad=0.0, r_bits=14, n_waves=2, seed=1, s_bits=7, gap=0, **kw):
    """a ragged batch: reads of 16 C - 15 .. 16 C bases, every tile sorted longest first, tails[tile][d] = its reads with more than d bases in their last piece"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(16 * C - 15, 16 * C + 1, size=n)
    ntl = (n + 2047) // 2048
    reads, tails = [], np.zeros((ntl, 16), dtype=np.uint32)
    arr = np.full((n, 16 * C), ord("A"), dtype=np.uint8)
    for t in range(ntl):
        ls = np.sort(lens[t * 2048:(t + 1) * 2048])[::-1]
        for d in range(16):
            tails[t, d] = int(np.count_nonzero(ls - 16 * (C - 1) > d))
        for j, ln in enumerate(ls):
            row = ALPHA[rng.integers(0, 4, size=ln)]
            if p_bad:
                row = np.where(rng.random(ln) < p_bad, ALPHA[rng.integers(4, len(ALPHA), size=ln)], row).astype(np.uint8)
            arr[t * 2048 + j, :ln] = row
            reads.append(row.tobytes())
    return check(strand, reads, arr, n, 16 * C, k, r_bits, s_bits, gap, n_waves, tails=tails, **kw)
