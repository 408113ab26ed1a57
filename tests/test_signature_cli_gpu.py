"""`ntcard --signature` and bin/ntsig (include/ntcard_hip.h: NTC_FLAG_SIGNATURE): the .sig file beside a .hist holds exactly the model's pairs
(tests/sig_model.py), the .hist and the messages are those of a run without the option, and ntsig compares two runs."""
import os

import numpy as np
import pytest

import sig_model
import ntcard_amd as nt
from support import GOLD, NTCARD, NTSIG, run_cli, small_reads

FASTQ = os.path.join(GOLD, "reads_small.fq.gz")


def run(cmd, cwd):
    return run_cli(cmd[0], cmd[1:], cwd=cwd, timeout=600)


def without_runtime(text):
    return [line for line in text.splitlines() if not line.startswith(b"Runtime(sec)")]


def test_help_mentions_the_option(tmp_path):
    r = run([NTCARD, "--help"], tmp_path)
    assert r.returncode == 0 and b"--signature" in r.stderr


def test_the_option_needs_a_prefix(tmp_path):
    r = run([NTCARD, "--signature", "-k", "32", "-o", "x.tsv", FASTQ], tmp_path)
    assert r.returncode != 0 and b"--signature" in r.stderr and not (tmp_path / "x.tsv").exists()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sig_cli")
    reads = small_reads()
    assert len(reads) == 5000
    (d / "half.fq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads[:2500])))
    out = {}
    out["with"] = run([NTCARD, "--signature", "-k", "32,20", "-p", "with", FASTQ], d)
    out["plain"] = run([NTCARD, "-k", "32,20", "-p", "plain", FASTQ], d)
    out["half"] = run([NTCARD, "--signature", "-k", "32,20", "-p", "half", "half.fq"], d)
    out["fwd"] = run([NTCARD, "--signature", "--strand=forward", "-k", "32", "-p", "fwd", FASTQ], d)
    return d, reads, out


@pytest.mark.gpu
def test_sig_files_hold_the_model(runs):
    d, reads, out = runs
    for r in out.values():
        assert r.returncode == 0, r.stderr
    for k in (32, 20):
        wh, wc = sig_model.model(reads, k, "canonical", 7)
        assert wh.size > 1000 and int(wc.max()) > 1
        hd, h, c = nt.signature_read(d / f"with_k{k}.sig")
        assert hd == dict(k=k, gap=0, strand=0, hpc=0, s_bits=7, mask="1" * k, n=wh.size)
        assert np.array_equal(h, wh) and np.array_equal(c.astype(np.int64), wc)
    hd, h, c = nt.signature_read(d / "fwd_k32.sig")
    wh, wc = sig_model.model(reads, 32, "forward", 7)
    assert hd["strand"] == 1 and np.array_equal(h, wh) and np.array_equal(c.astype(np.int64), wc)


@pytest.mark.gpu
def test_hist_and_messages_are_those_of_a_run_without_the_option(runs):
    d, _, out = runs
    for k in (32, 20):
        a, b = (d / f"with_k{k}.hist").read_bytes(), (d / f"plain_k{k}.hist").read_bytes()
        assert a == b and len(a) > 100
    assert out["with"].stdout == out["plain"].stdout
    assert without_runtime(out["with"].stderr) == without_runtime(out["plain"].stderr)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("plain")) == ["plain_k20.hist", "plain_k32.hist"]
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("with")) == ["with_k20.hist", "with_k20.sig", "with_k32.hist", "with_k32.sig"]


@pytest.mark.gpu
def test_ntsig_compares_two_runs(runs):
    d, reads, _ = runs
    r = run([NTSIG, "compare", "with_k32.sig", "with_k32.sig"], d)
    assert r.returncode == 0 and b"jaccard\t1.000000" in r.stdout, r.stderr
    full, half = sig_model.model(reads, 32, "canonical", 7)[0], sig_model.model(reads[:2500], 32, "canonical", 7)[0]
    common = np.intersect1d(full, half).size
    assert 0 < common == half.size < full.size
    r = run([NTSIG, "compare", "with_k32.sig", "half_k32.sig"], d)
    assert r.returncode == 0, r.stderr
    f = dict(line.split("\t") for line in r.stdout.decode().splitlines())
    assert int(f["common"]) == common and f["containment_a_in_b"] == "%.6f" % (common / full.size) and f["containment_b_in_a"] == "1.000000"
    assert f["jaccard"] == "%.6f" % (common / (full.size + half.size - common))
    for other, field in (("with_k20.sig", "k"), ("fwd_k32.sig", "strand")):
        r = run([NTSIG, "compare", "with_k32.sig", other], d)
        assert r.returncode != 0 and ("(%s differs)" % field).encode() in r.stderr
