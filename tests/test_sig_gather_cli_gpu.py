"""`ntsig gather` on the GPU (ntcard_amd/csrc/ntsig_cli.cpp): the TSV equals, as text, the rows of tests/sig_gather_model.py with the fractions recomputed here."""
import numpy as np
import pytest

import sig_gather_model
from support import NTSIG, run_cli

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEADER = dict(k=32, gap=0, strand=0, hpc=0, s_bits=7, mask="1" * 32)
COLUMNS = ["rank", "reference", "common", "unique", "f_orig_query", "f_unique_query", "f_unique_weighted", "f_match", "avg_abund"]


def frac(num, den):
    return "%.6f" % (num / den if den else 0.0)


def expected(files, q, counts, refs, **kw):
    rows, rest, rest_w = sig_gather_model.gather(q, counts, refs, **kw)
    total = int(counts.astype(np.uint64).sum())
    lines = [COLUMNS]
    for rank, r in enumerate(rows, 1):
        ref, common, unique, weight = int(r["ref"]), int(r["common"]), int(r["unique"]), int(r["unique_weight"])
        lines.append([str(rank), files[ref], str(common), str(unique), frac(common, q.size), frac(unique, q.size), frac(weight, total), frac(unique, refs[ref].size),
                      frac(weight, unique)])
    lines.append(["unassigned", "-", "-", str(rest), "-", frac(rest, q.size), frac(rest_w, total), "-", frac(rest_w, rest)])
    return lines, rows


def test_gather_prints_the_models_rows(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a HIP device (run on the MI355X box)"
    import ntcard_amd as nt
    rng = np.random.default_rng(61)
    pool = np.unique(rng.integers(1, 2**64, size=12_000, dtype=np.uint64))
    q = pool[:8000]
    counts = rng.integers(1, 40, size=q.size).astype(np.uint32)
    lists = {"a.sig": pool[500:3500], "inside_a.sig": pool[1000:2000], "b.sig": pool[3000:9000], "small.sig": pool[490:510], "empty.sig": pool[:0],
             "other.sig": pool[9000:11_000]}
    nt.signature_write(tmp_path / "q.sig", HEADER, q, counts)
    files = []
    for name, h in lists.items():
        nt.signature_write(tmp_path / name, HEADER, h, np.ones(h.size, np.uint32))
        files.append(str(tmp_path / name))
    refs = list(lists.values())

    def run(*flags):
        r = run_cli(NTSIG, ["gather", *flags, tmp_path / "q.sig", *files], timeout=120)
        assert r.returncode == 0, r.stderr
        return [line.split("\t") for line in r.stdout.decode().splitlines()]

    want, rows = expected(files, q, counts, refs)
    assert run() == want
    assert [files[i].rsplit("/", 1)[1] for i in rows["ref"]] == ["b.sig", "a.sig", "small.sig"] and want[-1][0] == "unassigned" and want[-1][3] == "490"
    assert want[2][4] != want[2][5] and want[1][8] not in ("0.000000", "1.000000")  # a's common and unique differ; the weights are counts
    want, rows = expected(files, q, counts, refs, threshold=11)
    assert run("--threshold", "11") == want and rows.size == 2 and want[-1][3] == "500"
    want, rows = expected(files, q, counts, refs, threshold=10)
    assert run("--threshold", "10") == want and rows.size == 3


def test_gather_of_an_empty_query(tmp_path):
    import ntcard_amd as nt
    pool = np.arange(1, 101, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 8)
    nt.signature_write(tmp_path / "q.sig", HEADER, pool[:0], np.ones(0, np.uint32))
    nt.signature_write(tmp_path / "a.sig", HEADER, pool, np.ones(100, np.uint32))
    r = run_cli(NTSIG, ["gather", tmp_path / "q.sig", tmp_path / "a.sig"], timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == ["\t".join(COLUMNS), "unassigned\t-\t-\t0\t-\t0.000000\t0.000000\t-\t0.000000"]
