"""`ntcard` -> `.hist` -> `ntbloom build --hist` -> `info` -> `query` on the test reads (ntcard_amd/csrc/ntbloom_cli.cpp): the filter is sized from the
F0 line ntcard wrote, the `.bf` bytes behind the header are the image of tests/bloom_model.py, and a query prints per record what the model counts —
from FASTQ, from wrapped FASTA and through the decompressor's pipe."""
import os
import random
import shutil

import numpy as np
import pytest

import bloom_model as bm
import strand_model as sm
from support import GOLD, NTBLOOM, NTCARD, fastq, rows_of, rseq, run_cli, small_reads

pytestmark = pytest.mark.gpu
K, H = 32, 3


def run(binary, args, cwd):
    r = run_cli(binary, args, cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def fasta(seqs, prefix=b"c"):  # wrapped at 60 columns: the k-mers cross the line breaks
    return b"".join(b">%s%d some text\n" % (prefix, i) + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)) for i, s in enumerate(seqs))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("bloom_cli")
    reads = small_reads()
    (d / "reads.fq").write_bytes(fastq(reads, b"r"))
    (d / "reads.fa").write_bytes(fasta(reads, b"r"))
    shutil.copy(os.path.join(GOLD, "reads_small.fq.gz"), d / "reads.fq.gz")
    rng = random.Random(77)
    other = [rseq(rng, rng.randint(20, 300), pn=0.01) for _ in range(300)] + [b"", reads[5], reads[6][:31]]
    (d / "other.fa").write_bytes(fasta(other))
    run(NTCARD, ["-k", str(K), "-p", "s", "reads.fq"], d)
    return d, reads, other


def hist_f0(path):
    lines = dict(line.split("\t") for line in open(path).read().splitlines()[:2])
    return int(lines["F0"])


def test_hist_to_filter_to_query(work):
    d, reads, other = work
    f0 = hist_f0(d / f"s_k{K}.hist")
    assert f0 > 50_000
    import ntcard_amd as nt
    m = nt.bloom_size(f0, 0.01, H)
    run(NTBLOOM, ["build", "-k", K, "--hist", f"s_k{K}.hist", "--fpr", "0.01", "-o", "s.bf", "reads.fq"], d)
    assert not os.path.exists(d / "s.bf.part")
    from ntcard_amd import bloom
    hd, image = bloom.read_file(d / "s.bf")
    vals = np.concatenate(bm.h0_values(reads, K, sm.CANONICAL))
    assert hd == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": m, "n_inserted": int(vals.size)}
    want = bm.image_of(bm.positions(vals, H, K, m), m)
    assert np.array_equal(image, want)  # the bytes behind the header are the model's image
    # info
    r = run(NTBLOOM, ["info", "s.bf"], d)
    lines = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    pop = bm.popcount(want)
    assert lines["bits"] == str(m) and lines["hashes"] == str(H) and lines["k"] == str(K) and lines["popcount"] == str(pop)
    assert float(lines["occupancy"]) == pytest.approx(pop / m, abs=1e-6) and float(lines["fpr"]) == pytest.approx((pop / m) ** H, rel=1e-4)
    # sized from ntcard's own F0, the filter comes out near the rate it was sized for.  How near: F0 is an estimate from about 1,400 sampled distinct k-mers
    # (91 k distinct at sBits 7), a standard error of 2.7 %; allow it 10 %.  d ln fpr / d ln n = h x e^-x / (1 - e^-x) = 2.65 at x = h n / m = 0.2426
    # (h = 3, fpr 0.01), so the rate stays below 0.01 * 1.1^2.65 = 0.0129
    assert (pop / m) ** H < 0.0129
    # query: the reads themselves are all found ...
    rows = rows_of(run(NTBLOOM, ["query", "s.bf", "reads.fq"], d).stdout)
    mw, mh = bm.query(want, reads, K, sm.CANONICAL, H, m)
    assert [r[0] for r in rows] == [f"r{i}" for i in range(len(reads))]
    assert [int(r[1]) for r in rows] == [len(s) for s in reads]
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mw.tolist() and np.array_equal(mh, mw)
    # ... and other records give what the model's membership test gives, names cut at the first blank
    rows = rows_of(run(NTBLOOM, ["query", "s.bf", "other.fa"], d).stdout)
    mw, mh = bm.query(want, other, K, sm.CANONICAL, H, m)
    assert [r[0] for r in rows] == [f"c{i}" for i in range(len(other))]
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mh.tolist()
    assert int(mh[-2]) == int(mw[-2]) > 0 and int(mw[-1]) == 0 and int(mh[:300].sum()) < int(mw[:300].sum()) // 10
    for r, w, h in zip(rows, mw, mh):
        assert float(r[4]) == pytest.approx(h / w if w else 0.0, abs=1e-6)


def test_fasta_gz_strands_and_sizes_give_the_models_bytes(work):
    d, reads, _ = work
    from ntcard_amd import bloom
    run(NTBLOOM, ["build", "-k", K, "-m", "1048583", "-o", "fq.bf", "reads.fq"], d)
    ref = (d / "fq.bf").read_bytes()
    vals = np.concatenate(bm.h0_values(reads, K, sm.CANONICAL))
    assert ref[40:] == bm.image_of(bm.positions(vals, H, K, 1048583), 1048583).tobytes()
    run(NTBLOOM, ["build", "-k", K, "-m", "1048583", "-o", "fa.bf", "reads.fa"], d)
    assert (d / "fa.bf").read_bytes() == ref
    if shutil.which("gunzip"):
        run(NTBLOOM, ["build", "-k", K, "-m", "1048583", "-o", "gz.bf", "reads.fq.gz"], d)
        assert (d / "gz.bf").read_bytes() == ref
    # two files are one input; -H and --strand reach the kernels; --distinct sizes like --hist
    half = len(reads) // 2
    (d / "a.fq").write_bytes(fastq(reads[:half]))
    (d / "b.fa").write_bytes(fasta(reads[half:]))
    run(NTBLOOM, ["build", "-k", "21", "-H", "5", "--strand=reverse", "--distinct", "300000", "--fpr", "0.05", "-o", "r.bf", "a.fq", "b.fa"], d)
    hd, image = bloom.read_file(d / "r.bf")
    import ntcard_amd as nt
    m = nt.bloom_size(300000, 0.05, 5)
    vals = np.concatenate(bm.h0_values(reads, 21, sm.REVERSE))
    assert hd == {"k": 21, "n_hash": 5, "strand": "reverse", "m_bits": m, "n_inserted": int(vals.size)}
    assert np.array_equal(image, bm.image_of(bm.positions(vals, 5, 21, m), m))
