"""`.hist` -> `ntbloom count --hist` -> `ntbloom solid --hist` -> `ntbloom query` on reads the test writes (ntcard_amd/csrc/ntbloom_cli.cpp): the counting
filter is sized from the F0 line, the solid filter from F0 - sum_{i<C} f_i, the `.cbf` bytes behind the header are the counters of tests/cbloom_model.py,
`solid.bf` is byte for byte the model's image of the k-mers counted at least C times, and the query rows are what the models count."""
import os
import random

import numpy as np
import pytest

import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from support import NTBLOOM, fastq, rows_of, rseq_acgt, run_cli

pytestmark = pytest.mark.gpu
K, H, C_MIN = 32, 3, 2


def run(args, cwd):
    r = run_cli(NTBLOOM, args, cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """reads of 100 bases from a genome of 4000 at about sevenfold coverage, one base in 60 wrong: true k-mers come often, wrong ones once"""
    d = tmp_path_factory.mktemp("cbloom_cli")
    rng = random.Random(5)
    genome = rseq_acgt(rng, 4000)
    reads = []
    for _ in range(280):
        at = rng.randrange(len(genome) - 100)
        r = bytearray(genome[at: at + 100])
        for i in range(100):
            if rng.random() < 1 / 60:
                r[i] = rng.choice(b"ACGT")
        reads.append(bytes(r))
    reads += [b"ACGTN" * 10, b"", genome[:31]]
    other = [rseq_acgt(rng, rng.randint(20, 200)) for _ in range(60)] + [genome[100:400], reads[3], b""]
    (d / "reads.fq").write_bytes(fastq(reads, b"r"))
    (d / "other.fq").write_bytes(fastq(other, b"o"))
    # the `.hist` file of these reads, exact: F1 windows, F0 distinct k-mers, f_i of them seen i times
    v = cm.all_values(reads, K, sm.CANONICAL)
    _, true = np.unique(v, return_counts=True)
    f = np.bincount(true, minlength=12)
    (d / f"s_k{K}.hist").write_text(f"F1\t{v.size}\nF0\t{true.size}\n" + "".join(f"{i}\t{int(f[i])}\n" for i in range(1, 11)))
    return d, reads, other, int(true.size), f


def test_hist_to_counts_to_the_solid_filter_to_query(work):
    d, reads, other, f0, f = work
    import ntcard_amd as nt
    from ntcard_amd import bloom
    hist = f"s_k{K}.hist"
    assert f[1] > f0 // 4 and f0 - f[1] > 1000  # errors and solid k-mers both
    # count
    run(["count", "-k", K, "--hist", hist, "--fpr", "0.01", "-o", "s.cbf", "reads.fq"], d)
    assert not os.path.exists(d / "s.cbf.part")
    m = nt.bloom_size(f0, 0.01, H)
    hd, counters = bloom.read_counting_file(d / "s.cbf")
    want, n_win = cm.counters(reads, K, sm.CANONICAL, H, m)
    assert hd == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": m, "n_inserted": n_win}
    assert np.array_equal(counters, want)
    lines = dict(line.split("\t") for line in run(["info", "s.cbf"], d).stdout.decode().splitlines())
    assert lines["counters"] == str(m) and lines["nonzero"] == str(int((want != 0).sum())) and lines["saturated"] == str(int((want == 255).sum()))
    assert float(lines["fpr"]) == pytest.approx(((want != 0).sum() / m) ** H, rel=1e-4)
    # solid: the second stage, sized from F0 - f_1
    run(["solid", "--min-count", C_MIN, "--hist", hist, "--fpr", "0.01", "-o", "solid.bf", "s.cbf", "reads.fq"], d)
    assert not os.path.exists(d / "solid.bf.part")
    m2 = nt.bloom_size(f0 - int(f[1]), 0.01, H)
    assert m2 < m
    passing = cm.solid_values(want, reads, K, sm.CANONICAL, H, C_MIN)
    hd2, image = bloom.read_file(d / "solid.bf")
    assert hd2 == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": m2, "n_inserted": int(passing.size)}
    img = bm.image_of(bm.positions(passing, H, K, m2), m2)
    assert np.array_equal(image, img)  # byte for byte the model's
    # ... query solid.bf other.fq
    rows = rows_of(run(["query", "solid.bf", "other.fq"], d).stdout)
    mw, mh = bm.query(img, other, K, sm.CANONICAL, H, m2)
    assert [r[0] for r in rows] == [f"o{i}" for i in range(len(other))]
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mh.tolist()
    assert int(mh[-3]) > 200 and int(mh[:60].sum()) < int(mw[:60].sum()) // 10  # the genome's k-mers are solid, random ones are not
    # -H and another C reach the second stage
    run(["solid", "--min-count", "3", "--hist", hist, "--fpr", "0.05", "-H", "5", "-o", "solid3.bf", "s.cbf", "reads.fq"], d)
    m3 = nt.bloom_size(f0 - int(f[1]) - int(f[2]), 0.05, 5)
    p3 = cm.solid_values(want, reads, K, sm.CANONICAL, H, 3)
    hd3, image3 = bloom.read_file(d / "solid3.bf")
    assert hd3 == {"k": K, "n_hash": 5, "strand": "canonical", "m_bits": m3, "n_inserted": int(p3.size)}
    assert np.array_equal(image3, bm.image_of(bm.positions(p3, 5, K, m3), m3))


def test_query_min_count_and_threshold(work):
    d, reads, other, f0, f = work
    from ntcard_amd import bloom
    m = 20011  # small: collisions, so false "count >= c" answers occur and the model must count the same ones
    run(["count", "-k", K, "-m", m, "-o", "small.cbf", "reads.fq"], d)
    want, n_win = cm.counters(reads, K, sm.CANONICAL, H, m)
    hd, counters = bloom.read_counting_file(d / "small.cbf")
    assert hd["m_bits"] == m and hd["n_inserted"] == n_win and np.array_equal(counters, want)
    for c in (None, 1, 2, 5, 255):
        args = ["query"] + ([] if c is None else ["--min-count", c]) + ["small.cbf", "other.fq"]
        rows = rows_of(run(args, d).stdout)
        mw, mh = cm.query(want, other, K, sm.CANONICAL, H, c or 1)
        assert [r[0] for r in rows] == [f"o{i}" for i in range(len(other))]
        assert [int(r[1]) for r in rows] == [len(s) for s in other]
        assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mh.tolist(), c
        for r, w, h in zip(rows, mw, mh):
            assert float(r[4]) == pytest.approx(h / w if w else 0.0, abs=1e-6)
    # solid without input files thresholds the counters: as many bits as counters, the counting filter's hash count
    run(["solid", "--min-count", C_MIN, "-o", "thr.bf", "small.cbf"], d)
    hd2, image = bloom.read_file(d / "thr.bf")
    assert hd2 == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": m, "n_inserted": n_win}
    assert np.array_equal(image, cm.threshold(want, C_MIN))
    rows = rows_of(run(["query", "thr.bf", "other.fq"], d).stdout)
    mw, mh = cm.query(want, other, K, sm.CANONICAL, H, C_MIN)  # a k-mer is in the thresholded filter iff its count is >= C
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mh.tolist()


def test_solid_refuses_a_hist_too_short(work):
    import ctypes as C
    from ntcard_amd import _abi
    d, *_ = work
    hd = _abi.NtcBloomHeader(k=K, n_hash=H, strand=0, reserved=0, m_bits=64, n_inserted=0)
    assert _abi.lib().ntc_cbloom_write(str(d / "empty.cbf").encode(), C.byref(hd), np.zeros(64, dtype=np.uint8).ctypes.data_as(C.c_void_p)) == 0
    (d / "short.hist").write_text("F1\t1000\nF0\t600\n1\t400\n2\t100\n")
    r = run_cli(NTBLOOM, ["solid", "--min-count", "4", "--hist", "short.hist", "--fpr", "0.01", "-o", "no.bf", "empty.cbf", "reads.fq"], cwd=d, timeout=120)
    assert r.returncode != 0 and b"stop below --min-count - 1: short.hist" in r.stderr
    assert not os.path.exists(d / "no.bf") and not os.path.exists(d / "no.bf.part")
