"""`ntsig merge | intersect | subtract | filter | hist` on the GPU (ntcard_amd/csrc/ntsig_cli.cpp): OUT, read back with the library's reader, carries A's
header with the new n and the pairs of tests/sig_algebra_model.py; the hist TSV equals the model's spectrum, the >COV row and the shifted column included."""
import os

import numpy as np
import pytest

import sig_algebra_model as model
from support import NTSIG, run_cli

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEADER = dict(k=24, gap=0, strand=1, hpc=1, s_bits=9, mask="1" * 10 + "0" * 4 + "1" * 10)
U32_MAX = 2**32 - 1


@pytest.fixture(scope="module")
def sigs(tmp_path_factory):
    """a.sig, b.sig, c.sig and empty.sig: overlapping parts of one pool, with counts that saturate when added"""
    assert torch.cuda.is_available(), "GPU tests need a HIP device (run on the MI355X box)"
    import ntcard_amd as nt
    d = tmp_path_factory.mktemp("sigs")
    rng = np.random.default_rng(95)
    pool = np.unique(np.concatenate([rng.integers(0, 2**64, size=9000, dtype=np.uint64), np.array([0, 2**64 - 1], dtype=np.uint64)]))
    parts = {"a.sig": pool[:6000], "b.sig": pool[2000:8000:2], "c.sig": pool[3000:], "empty.sig": pool[:0]}
    out = {}
    for name, h in parts.items():
        c = rng.choice(np.array([1, 1, 1, 2, 3, 40, 1001, 2**31, U32_MAX], dtype=np.uint32), size=h.size)
        nt.signature_write(d / name, HEADER, h, c)
        out[name] = (str(d / name), h, c)
    return nt, d, out


def run_to_file(nt, d, command, *args):
    out = d / ("out_%s.sig" % command)
    r = run_cli(NTSIG, [command, "-o", out, *args], timeout=120)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert not os.path.exists(str(out) + ".part")
    header, h, c = nt.signature_read(out)
    assert header == dict(HEADER, n=h.size)
    return h, c


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.uint64 and got[1].dtype == np.uint32


def test_merge_writes_the_union(sigs):
    nt, d, s = sigs
    (fa, ha, ca), (fb, hb, cb), (fc, hc, cc), (fe, he, ce) = s["a.sig"], s["b.sig"], s["c.sig"], s["empty.sig"]
    want = model.union([ha, hb, hc, he], [ca, cb, cc, ce])
    assert (want[1] == U32_MAX).sum() > 100 and want[0][0] == 0 and want[0][-1] == 2**64 - 1
    assert same(run_to_file(nt, d, "merge", fa, fb, fc, fe), want)
    assert same(run_to_file(nt, d, "merge", fa), (ha, ca)) and same(run_to_file(nt, d, "merge", fe, fe), (he, ce))


def test_intersect_and_subtract_write_the_selection(sigs):
    nt, d, s = sigs
    (fa, ha, ca), (fb, hb, cb), (fc, hc, cc), (fe, he, ce) = s["a.sig"], s["b.sig"], s["c.sig"], s["empty.sig"]
    want = model.select(ha, ca, [hb, hc], "all")
    assert 0 < want[0].size < hb.size
    assert same(run_to_file(nt, d, "intersect", fa, fb, fc), want)
    want = model.select(ha, ca, [hb, hc], "none")
    assert want[0].size == 2000 + 500
    assert same(run_to_file(nt, d, "subtract", fa, fb, fc), want)
    assert same(run_to_file(nt, d, "intersect", fa, fe), (he, ce)) and same(run_to_file(nt, d, "subtract", fa, fe), (ha, ca))
    assert same(run_to_file(nt, d, "subtract", fa, fa), (he, ce))


def test_filter_writes_the_pairs_inside_the_bounds(sigs):
    nt, d, s = sigs
    fa, ha, ca = s["a.sig"]
    for flags, lo, hi in (((), 0, 0), (("--min-count", "2"), 2, 0), (("--max-count", "40"), 0, 40), (("--min-count", "2", "--max-count", "1001"), 2, 1001),
                          (("--min-count", "4294967295"), U32_MAX, 0), (("--min-count", "41", "--max-count", "1000"), 41, 1000)):
        want = model.select(ha, ca, [], "all", lo, hi)
        assert same(run_to_file(nt, d, "filter", *flags, fa), want), flags
    assert model.select(ha, ca, [], "all", 41, 1000)[0].size == 0 and 0 < model.select(ha, ca, [], "all", U32_MAX, 0)[0].size < ha.size // 4


def test_an_out_that_cannot_be_written_leaves_nothing_behind(sigs):
    nt, d, s = sigs
    fa = s["a.sig"][0]
    out = d / "no_such_directory" / "out.sig"
    r = run_cli(NTSIG, ["merge", "-o", out, fa, fa], timeout=120)
    assert r.returncode != 0 and r.stdout == b"" and b"cannot write" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(out) + ".part")
    target = d / "a_directory.sig"
    os.mkdir(target)
    r = run_cli(NTSIG, ["filter", "-o", target, fa], timeout=120)
    assert r.returncode != 0 and b"cannot write" in r.stderr and os.path.isdir(target) and not os.path.exists(str(target) + ".part")


@pytest.mark.parametrize("cov", [None, 2, 1001, 65535])
def test_hist_prints_the_models_spectrum(sigs, cov):
    nt, d, s = sigs
    fa, ha, ca = s["a.sig"]
    r = run_cli(NTSIG, ["hist", *(("-c", str(cov)) if cov else ()), fa], timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    cov = cov or 1000
    hist, weight = model.hist(ca, cov)
    shift = HEADER["s_bits"] - 1
    want = [["n", str(ha.size)], ["weight", str(weight)], ["sBits", str(HEADER["s_bits"])]]
    want += [[str(v), str(int(hist[v])), str(int(hist[v]) << shift)] for v in range(1, cov + 1)]
    want.append([">%d" % cov, str(int(hist[cov + 1])), str(int(hist[cov + 1]) << shift)])
    assert [line.split("\t") for line in r.stdout.decode().splitlines()] == want
    assert int(hist[1]) > 1000 and int(hist[cov + 1]) > 0 and weight > U32_MAX


def test_hist_of_an_empty_signature(sigs):
    nt, d, s = sigs
    r = run_cli(NTSIG, ["hist", "-c", "3", s["empty.sig"][0]], timeout=120)
    assert r.returncode == 0 and r.stdout.decode().splitlines() == ["n\t0", "weight\t0", "sBits\t9", "1\t0\t0", "2\t0\t0", "3\t0\t0", ">3\t0\t0"]
