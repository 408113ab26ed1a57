"""Inputs and models of the limit tests (tests/test_tiled_limits_gpu.py, tests/test_long_limits_gpu.py): numpy only, so that tests/test_limits_host.py can
pin them without a GPU.

  directed_batch        a batch of equal-length reads whose first nine are the directed ones (DIRECTED), the rest random with a few non-base bytes
  assert_directed       ... and the proof that they are there
  forward_sketch        one-strand (forward) t_Counter and F1 of equal-length reads, vectorised (tests/strand_model.py takes one ctypes call per window)
  k1h_blocks            sketch_k1h_blocks of ntc_sketch_k1h.hip
  cut_search_steps      the 64-way table search of cut_tiles_kernel (ntc_long.hip), step for step
"""
import numpy as np

import orc
import strand_model as sm
from support import ALPHA, random_reads, tile_array  # noqa: F401  (re-exported: lm.tile_array, lm.random_reads)

P_BAD = 5e-4  # non-base bytes of the random reads
N = ord("N")
DIRECTED = ("clean", "N at 0", "N at L - 1", "N at L - k", "N at L - k - 1", "N around the last chunk's first byte", "slot byte 1 at L - 20",
            "N run of 40 across 32768", "lower case and U")


def run_centre(L):
    """where the N run of 40 lies: across position 32768 where the read has one, else across the chunk boundary in its middle"""
    return 32768 if L > 32768 else (L // 2) & ~15


def directed_batch(rng, n, L, k):
    """(n, L) reads; n >= 70: rows 0 .. 8 are DIRECTED (no other non-base byte in them); k: the window length the positions refer to"""
    arr = random_reads(rng, n, L, P_BAD)
    if n < 70:
        return arr
    assert L >= 1009 and k <= 32
    arr[:9] = ALPHA[rng.integers(0, 4, size=(9, L))]
    arr[1, 0] = N
    arr[2, L - 1] = N
    arr[3, L - k] = N
    arr[4, L - k - 1] = N
    p = 16 * ((L + 15) // 16 - 1)  # the last chunk's first byte
    arr[5, p - 1] = N
    if p + 1 < L:
        arr[5, p + 1] = N
    arr[6, L - 20] = 1  # a base (T) to the reference's seed table, no letter to K1h: K1f's slow path, at the highest chunk index
    s = min(run_centre(L) - 20, L - 40)
    arr[7, s:s + 40] = N
    arr[8] = np.frombuffer(b"acgtuACGTU", dtype=np.uint8)[rng.integers(0, 10, size=L)]
    return arr


def assert_directed(arr, k):
    n, L = arr.shape
    assert n >= 70
    base = np.zeros(256, dtype=bool)
    base[np.frombuffer(b"ACGTacgtUu", dtype=np.uint8)] = True
    bad = ~base[arr[:9]]
    assert not bad[0].any() and not bad[8].any()
    assert np.isin(arr[0], np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    assert np.isin(arr[8], np.frombuffer(b"acgtu", dtype=np.uint8)).sum() > L // 4 and (arr[8] == ord("U")).any()
    for row, pos in ((1, [0]), (2, [L - 1]), (3, [L - k]), (4, [L - k - 1])):
        assert np.flatnonzero(bad[row]).tolist() == pos and arr[row, pos[0]] == N, DIRECTED[row]
    p = 16 * ((L + 15) // 16 - 1)
    assert np.flatnonzero(bad[5]).tolist() == [q for q in (p - 1, p + 1) if q < L] and p - 1 >= 0 and p < L
    assert np.flatnonzero(bad[6]).tolist() == [L - 20] and arr[6, L - 20] == 1
    run = np.flatnonzero(bad[7])
    assert run.size == 40 and run[-1] - run[0] == 39 and (arr[7, run] == N).all()
    c = run_centre(L)
    assert run[0] < c <= run[-1] and c % 16 == 0 and (c == 32768 or L <= 32768)


def k1h_blocks(k, L):
    """blocks of 16 window ends per read (ntc_sketch_k1h.hip: sketch_k1h_blocks)"""
    return ((L - 1 + 16 - ((k - 1) & 15)) >> 4) + 1


_seed = None


def _seeds():
    global _seed
    if _seed is None:
        L = orc.lib()
        _seed = np.array([L.orc_seed(b) for b in range(256)], dtype=np.uint64)
    return _seed


def forward_values(arr, k):
    """the forward ntHash fh = XOR_i srol^(k-1-i) seed(c_i) (nthash.hpp:220-239) of every window of k bases of every read of arr (n, L) that holds no
    non-base byte (ntHashIterator.hpp:59-86), as one array"""
    L = orc.lib()
    seed = _seeds()
    n, ln = arr.shape
    W = ln - k + 1
    if W <= 0:
        return np.zeros(0, dtype=np.uint64)
    fh = np.zeros((n, W), dtype=np.uint64)
    for i in range(k):
        tab = np.array([L.orc_srol(int(s), k - 1 - i) for s in seed], dtype=np.uint64)
        fh ^= tab[arr[:, i:i + W]]
    bad = np.zeros((n, ln + 1), dtype=np.int64)
    np.cumsum(seed[arr] == 0, axis=1, out=bad[:, 1:])
    return fh[(bad[:, k:] - bad[:, :-k]) == 0]


def forward_sketch(arr, k, r_bits, s_bits):
    """-> (t_Counter [1][2][1 << r_bits] uint16, F1 [1]) of a forward-strand engine over the reads of arr: ntComp (ntcard.cpp:132-145) over forward_values"""
    h = forward_values(arr, k)
    return sm.sketch_of([(h, h)], sm.FORWARD, r_bits, s_bits)


def cut_search_steps(n_seqs, target):
    """steps of cut_tiles_kernel's 64-way search (ntc_long.hip:50-55) over a table of n_seqs entries for the entry `target`"""
    lo, hi, steps = 0, n_seqs, 0
    while hi - lo > 1:
        stride = (hi - lo + 63) // 64
        n_le = sum(1 for lane in range(64) if lo + lane * stride < hi and lo + lane * stride <= target)
        lo, hi = lo + (n_le - 1) * stride, min(lo + n_le * stride, hi)
        steps += 1
    assert lo == target
    return steps
