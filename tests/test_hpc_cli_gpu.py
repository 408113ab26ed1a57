"""`ntcard --hpc` and `nthll --hpc` (include/ntcard_hip.h: NTC_FLAG_HPC): a run with the option over raw files gives byte for byte what a run without it
gives over the same records compressed beforehand by the pure-Python model (tests/hpc_model.py)."""
import random

import pytest

import hpc_model as hm
from support import NTCARD, NTHLL, run_cli


def run(cmd, cwd):
    return run_cli(cmd[0], cmd[1:], cwd=cwd, timeout=600)


@pytest.mark.parametrize("binary", [NTCARD, NTHLL])
def test_help_mentions_the_option(binary, tmp_path):
    r = run([binary, "--help"], tmp_path)
    assert r.returncode == 0 and b"--hpc" in r.stderr


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpc_cli")
    rng = random.Random(9)
    contigs = [hm.runs_seq(rng, n, p_other=0.0) for n in (5000, 1234, 61, 60, 59, 33, 20000)]
    contigs[0] = contigs[0][:700] + b"NNNN" + contigs[0][700:1500] + b"RR" + contigs[0][1500:]
    reads = [hm.runs_seq(rng, rng.randrange(40, 151), p_other=0.0) for _ in range(1500)]
    reads[3] = b"N" + reads[3][1:]

    def fasta(seqs):  # wrapped at 60 columns: runs cross the line breaks
        return b"".join(b">c%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)) for i, s in enumerate(seqs))

    def fastq(seqs):
        return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))

    (d / "raw.fa").write_bytes(fasta(contigs))
    (d / "raw.fq").write_bytes(fastq(reads))
    (d / "hpc.fa").write_bytes(fasta(hm.model(contigs)))
    (d / "hpc.fq").write_bytes(fastq(hm.model(reads)))  # (qualities trimmed to the compressed length)
    assert sum(len(c) for c in hm.model(contigs)) < 0.8 * sum(len(c) for c in contigs)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--strand=forward"]])
def test_ntcard_hist_files_are_identical(files, extra):
    tag = "s" if extra else "c"
    r = run([NTCARD, "--hpc", "-k", "21,32", "-p", f"with_{tag}"] + extra + ["raw.fa", "raw.fq"], files)
    assert r.returncode == 0, r.stderr
    r = run([NTCARD, "-k", "21,32", "-p", f"pre_{tag}"] + extra + ["hpc.fa", "hpc.fq"], files)
    assert r.returncode == 0, r.stderr
    r = run([NTCARD, "-k", "21,32", "-p", f"raw_{tag}"] + extra + ["raw.fa", "raw.fq"], files)
    assert r.returncode == 0, r.stderr
    for k in (21, 32):
        a, b, c = ((files / f"{p}_{tag}_k{k}.hist").read_bytes() for p in ("with", "pre", "raw"))
        assert a == b and len(a) > 100
        assert a != c  # (the option does something on these files)


@pytest.mark.gpu
def test_ntcard_gap_and_seed(files):
    for opts, name in ((["-k", "32", "-g", "8"], "_k32.hist"), (["--seed=1110111,11111111"], "_seed1_k7.hist")):
        r = run([NTCARD, "--hpc", "-p", "gw"] + opts + ["raw.fa", "raw.fq"], files)
        assert r.returncode == 0, r.stderr
        r = run([NTCARD, "-p", "gp"] + opts + ["hpc.fa", "hpc.fq"], files)
        assert r.returncode == 0, r.stderr
        assert (files / ("gw" + name)).read_bytes() == (files / ("gp" + name)).read_bytes()


@pytest.mark.gpu
def test_nthll_result_line_is_identical(files):
    a = run([NTHLL, "--hpc", "-k", "21,32", "raw.fa", "raw.fq"], files)
    b = run([NTHLL, "-k", "21,32", "hpc.fa", "hpc.fq"], files)
    c = run([NTHLL, "-k", "21,32", "raw.fa", "raw.fq"], files)
    assert a.returncode == 0 and b.returncode == 0 and c.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and a.stdout.count(b"F0, Exp# of distnt kmers") == 2
    assert a.stdout != c.stdout
