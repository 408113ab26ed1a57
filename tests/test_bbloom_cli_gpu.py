"""`ntcard` -> `.hist` -> `ntbloom build --blocked --hist` -> `query` -> `info` on the test reads, and `count` -> `solid --blocked`
(ntcard_amd/csrc/ntbloom_cli.cpp): the filter is sized by ntc_bbloom_size from the F0 line ntcard wrote, the file's bytes behind the header are the image
of tests/bbloom_model.py, and a query prints per record what the model counts."""
import os
import random

import numpy as np
import pytest

import bbloom_model as bb
import bloom_model as bm
import cbloom_model as cm
import strand_model as sm
from support import NTBLOOM, NTCARD, fastq, rows_of, rseq, run_cli, small_reads

pytestmark = pytest.mark.gpu
K, H = 32, 3


def run(binary, args, cwd):
    r = run_cli(binary, args, cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("bbloom_cli")
    reads = small_reads()
    (d / "reads.fq").write_bytes(fastq(reads, b"r"))
    rng = random.Random(78)
    other = [rseq(rng, rng.randint(20, 300), pn=0.01) for _ in range(300)] + [b"", reads[5], reads[6][:31]]
    (d / "other.fq").write_bytes(fastq(other, b"c"))
    run(NTCARD, ["-k", str(K), "-p", "s", "reads.fq"], d)
    return d, reads, other


def hist_lines(path):
    return dict(line.split("\t") for line in open(path).read().splitlines())


def test_hist_to_blocked_filter_to_query_to_info(work):
    d, reads, other = work
    import ntcard_amd as nt
    from ntcard_amd import bloom
    f0 = int(hist_lines(d / f"s_k{K}.hist")["F0"])
    m = nt.bbloom_size(f0, 0.01, H)
    assert m % 512 == 0 and m > nt.bloom_size(f0, 0.01, H)
    run(NTBLOOM, ["build", "--blocked", "-k", K, "--hist", f"s_k{K}.hist", "--fpr", "0.01", "-o", "s.bbf", "reads.fq"], d)
    assert not os.path.exists(d / "s.bbf.part")
    hd, image = bloom.read_blocked_file(d / "s.bbf")
    vals = np.concatenate(bm.h0_values(reads, K, sm.CANONICAL))
    assert hd == {"k": K, "n_hash": H, "strand": "canonical", "m_bits": m, "n_inserted": int(vals.size), "block_bits": 512}
    want = bb.image_of(vals, H, K, m)
    assert (d / "s.bbf").read_bytes()[:8] == b"NTCBB1\0\0" and np.array_equal(image, want)  # the bytes behind the header are the model's image
    # query: the reads themselves are all found ...
    rows = rows_of(run(NTBLOOM, ["query", "s.bbf", "reads.fq"], d).stdout)
    mw, mh = bb.query(want, reads, K, sm.CANONICAL, H, m)
    assert [r[0] for r in rows] == [f"r{i}" for i in range(len(reads))]
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mw.tolist() and np.array_equal(mh, mw)
    # ... and other records give what the model's membership test gives
    rows = rows_of(run(NTBLOOM, ["query", "s.bbf", "other.fq"], d).stdout)
    mw, mh = bb.query(want, other, K, sm.CANONICAL, H, m)
    assert [r[0] for r in rows] == [f"c{i}" for i in range(len(other))]
    assert [int(r[2]) for r in rows] == mw.tolist() and [int(r[3]) for r in rows] == mh.tolist()
    assert int(mh[-2]) == int(mw[-2]) > 0 and int(mw[-1]) == 0 and int(mh[:300].sum()) < int(mw[:300].sum()) // 10
    # --min-count goes with a counting filter only
    r = run_cli(NTBLOOM, ["query", "--min-count", "2", "s.bbf", "reads.fq"], cwd=d)
    assert r.returncode != 0 and b"--min-count goes with a counting filter" in r.stderr
    # info: the header, the block size, the popcount and the rate from the blocks' histogram
    lines = dict(line.split("\t") for line in run(NTBLOOM, ["info", "s.bbf"], d).stdout.decode().splitlines())
    pop = bm.popcount(want)
    assert lines["bits"] == str(m) and lines["hashes"] == str(H) and lines["k"] == str(K) and lines["block"] == "512" and lines["blocks"] == str(m // 512)
    assert lines["popcount"] == str(pop) and float(lines["occupancy"]) == pytest.approx(pop / m, abs=1e-6)
    assert float(lines["fpr"]) == pytest.approx(bb.realised_fpr(want, H), rel=1e-4)
    # -m, -H and --strand reach the blocked kernels too
    run(NTBLOOM, ["build", "--blocked", "-k", "21", "-H", "5", "--strand=reverse", "-m", str(300 * 512), "-o", "r.bbf", "reads.fq"], d)
    hd, image = bloom.read_blocked_file(d / "r.bbf")
    vals = np.concatenate(bm.h0_values(reads, 21, sm.REVERSE))
    assert (hd["k"], hd["n_hash"], hd["strand"], hd["m_bits"], hd["n_inserted"]) == (21, 5, "reverse", 300 * 512, int(vals.size))
    assert np.array_equal(image, bb.image_of(vals, 5, 21, 300 * 512))


def test_count_to_blocked_solid_filter(work):
    d, reads, _ = work
    import ntcard_amd as nt
    from ntcard_amd import bloom
    lines = hist_lines(d / f"s_k{K}.hist")
    n_solid = int(lines["F0"]) - int(lines["1"])
    assert n_solid > 0
    (d / "twice.fq").write_bytes(fastq(reads + reads[:200], b"t"))  # the k-mers of 200 reads occur twice
    run(NTBLOOM, ["count", "-k", K, "--hist", f"s_k{K}.hist", "--fpr", "0.01", "-o", "s.cbf", "twice.fq"], d)
    run(NTBLOOM, ["solid", "--blocked", "--min-count", "2", "--hist", f"s_k{K}.hist", "--fpr", "0.01", "-o", "solid.bbf", "s.cbf", "twice.fq"], d)
    hd, image = bloom.read_blocked_file(d / "solid.bbf")
    m = nt.bbloom_size(n_solid, 0.01, H)
    c_m = nt.bloom_size(int(lines["F0"]), 0.01, H)
    seqs = reads + reads[:200]
    cnt, _ = cm.counters(seqs, K, sm.CANONICAL, H, c_m)
    solid = cm.solid_values(cnt, seqs, K, sm.CANONICAL, H, 2)
    assert (hd["m_bits"], hd["n_hash"], hd["k"], hd["n_inserted"], hd["block_bits"]) == (m, H, K, int(solid.size), 512) and solid.size > 0
    assert np.array_equal(image, bb.image_of(solid, H, K, m))
