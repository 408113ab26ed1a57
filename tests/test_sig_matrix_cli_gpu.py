"""`ntsig matrix` on the GPU (ntcard_amd/csrc/ntsig_cli.cpp): the TSV of all pairs, every off-diagonal value equal — as text — to what `ntsig compare` prints
for that pair."""
import os

import numpy as np
import pytest

from support import NTSIG, run_cli

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HEADER = dict(k=32, gap=0, strand=0, hpc=0, s_bits=7, mask="1" * 32)


def ntsig(*args):
    return run_cli(NTSIG, args, timeout=120)


@pytest.mark.parametrize("containment", [False, True])
def test_matrix_agrees_with_compare(tmp_path, containment):
    assert torch.cuda.is_available(), "GPU tests need a HIP device (run on the MI355X box)"
    import ntcard_amd as nt
    pool = np.unique(np.random.default_rng(51).integers(1, 2**64, size=12000, dtype=np.uint64))
    lists = {"a.sig": pool[:6000], "b.sig": pool[4500:11000], "empty.sig": pool[:0]}
    files = []
    for name, h in lists.items():
        nt.signature_write(tmp_path / name, HEADER, h, np.ones(h.size, np.uint32))
        files.append(str(tmp_path / name))
    r = ntsig("matrix", *(["--containment"] if containment else []), *files)
    assert r.returncode == 0, r.stderr
    rows = [line.split("\t") for line in r.stdout.decode().splitlines()]
    assert rows[0] == [""] + files and [row[0] for row in rows[1:]] == files and all(len(row) == 4 for row in rows)
    key = "containment_a_in_b" if containment else "jaccard"
    for i in range(3):
        for j in range(3):
            if i == j:
                assert rows[1 + i][1 + j] == ("1.000000" if lists[os.path.basename(files[i])].size else "0.000000")
                continue
            c = ntsig("compare", files[i], files[j])
            assert c.returncode == 0, c.stderr
            fields = dict(line.split("\t") for line in c.stdout.decode().splitlines())
            assert rows[1 + i][1 + j] == fields[key], (i, j)
    assert rows[1][2] not in ("0.000000", "1.000000")  # a and b overlap in part
