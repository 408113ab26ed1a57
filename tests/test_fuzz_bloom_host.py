"""Host tests of tools/fuzz_bloom.py through its dry mode: what the short run of the suite (fuzz_bloom.SHORT_RUN, run on the device by
tests/test_bloom_limits_gpu.py) draws — every kind, action and strand, both ends of the k range, few cases without a window — without torch and without a
device; and that a case is a function of its seed alone, which is what makes the line printed at a mismatch enough to run that case again."""
import json
import os
import subprocess
import sys

import pytest

from support import ROOT

TOOL = os.path.join(ROOT, "tools", "fuzz_bloom.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_bloom  # noqa: E402


def dry(*args):
    """the tool's --dry output as a list of dicts; in the child `import torch` fails, so a dry mode that wanted it would not get this far"""
    code = "import runpy, sys; sys.modules['torch'] = None; sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')"
    r = subprocess.run([sys.executable, "-c", code, TOOL, *map(str, args), "--dry"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(line) for line in r.stdout.decode().splitlines()]


@pytest.fixture(scope="module")
def short_run():
    return dry(*fuzz_bloom.SHORT_RUN)


def test_short_run_draws_every_kind_action_strand_and_both_ends_of_k(short_run):
    n_cases, _ = fuzz_bloom.SHORT_RUN
    assert len(short_run) == n_cases  # the sweep skips no case
    assert {p["kind"] for p in short_run} == set(fuzz_bloom.KINDS)
    assert {(p["kind"], p["action"]) for p in short_run} == {(kind, a) for kind, actions in fuzz_bloom.ACTIONS.items() for a in actions}
    assert {a for actions in fuzz_bloom.ACTIONS.values() for a in actions} == {"insert_query", "profile", "solid_plain", "solid_blocked", "hashes"}
    assert {p["strand"] for p in short_run} == {"canonical", "forward", "reverse"}
    ks = [p["k"] for p in short_run]
    assert max(ks) >= 599 and min(ks) <= 2 and all(1 <= k <= 600 for k in ks)
    walked = [p for p in short_run if p["action"] != "hashes"]
    assert any(p["k"] >= 599 and p["windows"] > 4096 for p in walked)  # the walk itself at the top of the k range, over more than one block
    assert all(1 <= p["n_hash"] <= 32 and 0 <= p["lead"] <= 15 for p in short_run)
    assert {p["m"] % 512 for p in short_run if p["kind"] == "blocked"} == {0}


def test_short_run_has_few_cases_without_a_window_and_none_too_large(short_run):
    n_cases, _ = fuzz_bloom.SHORT_RUN
    assert 10 * sum(1 for p in short_run if p["windows"] == 0) <= n_cases
    assert all(p["positions"] < fuzz_bloom.MAX_POSITIONS for p in short_run)
    assert any(p["n_seqs"] > 70 for p in short_run) and any(p.get("p_bad") for p in short_run) and any(p.get("p_low") for p in short_run)


def test_a_case_is_a_function_of_its_seed(short_run):
    for p in (short_run[0], short_run[-1]):
        assert dry("--case", p["case_seed"]) == [p]
    seqs = [fuzz_bloom.sequences(fuzz_bloom.draw(short_run[3]["case_seed"])) for _ in range(2)] if short_run[3]["action"] != "hashes" else [0, 0]
    assert seqs[0] == seqs[1]


def test_sequences_hold_what_the_layout_promises():
    """lower case, U and non-base bytes occur, the lengths are the drawn ones"""
    p = next(p for p in map(fuzz_bloom.draw, range(200)) if p["action"] != "hashes" and p["p_bad"] and p["p_low"] and sum(p["lens"]) > 5000)
    seqs = fuzz_bloom.sequences(p)
    assert [len(s) for s in seqs] == p["lens"]
    text = b"".join(seqs)
    assert any(c in text for c in b"acgt") and b"U" in text and any(c in text for c in b"NnRYKM.-*")
    assert set(text) <= set(b"ACGTUacgtuNnRYKM.-*")
