"""GPU tests of the general kernel K1, one test id per case of tests/k1_cases.py (tests/test_k1_cases_host.py shows what the cases cover).  Every case is
run once and compared EXACTLY with its reference — t_Counter and F1; signature pairs and counts; nthll registers and F1; dumped values and counts — and
ntc_k1_variant_stats must show that the launches were the ones the case is there for: the rows of K1's table, launch for launch the regimes, the waves
per block of the hf_shape port, and with the launched shape the paths the host file counted on."""
import functools

import numpy as np
import pytest

import k1_cases as kc
from gpu_support import dev, nt  # noqa: F401
from support import to_slots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STRAND = {"canonical": 0, "forward": 1, "reverse": 2}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stats(nt):
    return {s["row"]: s for s in nt.k1_variant_stats()}


@functools.lru_cache(maxsize=None)
def row_slots(reads_key, stride, n_slots):
    """the read set in row slots, repeated up to n_slots (a replicated case: whole copies and the head of one more), uploaded once"""
    reads = kc.read_set(*reads_key)
    base = to_slots(reads, stride, tail=0)
    m, extra = divmod(n_slots, len(reads))
    return dev(np.concatenate([np.tile(base, m), base[:extra * stride], np.full(16, ord("A"), dtype=np.uint8)]))


@functools.lru_cache(maxsize=None)
def tiles(reads_key, n_slots):
    """the read set in the tiled layout (whole tiles), repeated up to n_slots"""
    import ntcard_amd
    reads = kc.read_set(*reads_key)
    base = ntcard_amd.tile_reads(list(reads), reads_key[1])
    if n_slots == len(reads):
        return dev(base)
    assert len(reads) % kc.TILE == 0
    m, extra = divmod(n_slots, len(reads))
    one = base.size // (len(reads) // kc.TILE)
    return dev(np.concatenate([np.tile(base, m), base[:-(-extra // kc.TILE) * one]]))


@functools.lru_cache(maxsize=None)
def ragged_tiles(reads_key):
    import ntcard_amd
    t, tails, _ = ntcard_amd.tile_reads_ragged(list(kc.read_set(*reads_key)), (reads_key[1] + 15) // 16)
    return dev(t), dev(tails)


def submit(e, case, n_slots):
    L = kc.read_len(case)
    if case.submit == "rows":
        e.submit_device(row_slots(case.reads, case.stride, n_slots).data_ptr(), n_slots, L, case.stride)
    elif case.submit == "tiles":
        e.submit_tiled_device(tiles(case.reads, n_slots).data_ptr(), n_slots, L)
    elif case.submit == "tiles_ragged":
        t, tails = ragged_tiles(case.reads)
        e.submit_tiled_ragged_device(t.data_ptr(), n_slots, (L + 15) // 16, tails.data_ptr())
    else:
        e.submit_reads(list(kc.read_set(*case.reads)))


def run_and_compare(nt, case, n_slots):
    ks = case.ks
    if case.kind == "dump":
        n, L = n_slots, kc.read_len(case)
        maxw = max(L - ks[0] + 1, 1)
        dh = torch.zeros(n * maxw, dtype=torch.int64, device="cuda")
        dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        nt.hash_dump_strand_device(row_slots(case.reads, case.stride, n).data_ptr(), n, L, case.stride, case.masks[0], STRAND[case.strand], maxw,
                                   dh.data_ptr(), dc.data_ptr())
        torch.cuda.synchronize()
        hh, cc = dh.cpu().numpy().view(np.uint64).reshape(n, maxw), dc.cpu().numpy()
        want = kc.expected_dump(case)
        assert np.array_equal(cc, [len(w) for w in want]), case.name
        for i, w in enumerate(want):
            assert np.array_equal(hh[i, :len(w)], w), (case.name, i)
        return
    if case.kind == "hll":
        kw = dict(n_bits=case.n_bits, strand=case.strand)
        e = nt.HllEngine.from_seeds(list(case.masks), **kw) if case.gap < 0 else nt.HllEngine(ks, **kw)
        with e:
            for _ in range(2 if case.rep else 1):  # (run_hll's sub-batches double with the reads seen: the second submit is one launch)
                submit(e, case, n_slots)
            regs, f1 = e.finish()
        wregs, wf1 = kc.expected_hll(case, n_slots)
        assert np.array_equal(f1, wf1), (case.name, f1, wf1)
        assert np.array_equal(regs, wregs), (case.name, int((regs != wregs).sum()))
        return
    kw = dict(r_bits=kc.R_BITS, s_bits=case.s_bits, strand=case.strand, signature=case.kind == "sig", log_entries=case.log_entries,
              flags=nt.FLAG_ALWAYS_LOG if case.update == "log" else nt.FLAG_DIRECT_ATOMICS)
    e = nt.Engine.from_seeds(list(case.masks), **kw) if case.gap < 0 else nt.Engine(ks, gap=max(case.gap, 0), **kw)
    with e:
        submit(e, case, n_slots)
        tc, _, f1 = e.finish(counters=True)
        sigs = [e.signature(i) for i in range(len(ks))] if case.kind == "sig" else []
    wtc, wf1 = kc.expected_sketch(case, n_slots)
    assert np.array_equal(f1, wf1), (case.name, f1, wf1)
    assert np.array_equal(tc, wtc), (case.name, int((tc != wtc).sum()))
    for i, (h, c) in enumerate(sigs):
        wh, wc = kc.expected_signature(case, i, n_slots)
        assert np.array_equal(h, wh), (case.name, i, h.size, wh.size)
        assert np.array_equal(c, wc), (case.name, i, int((c != wc).sum()))


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_case(nt, name):
    case = kc.BY_NAME[name]
    plan = kc.launches(case, cus())
    before = stats(nt)
    run_and_compare(nt, case, kc.batch_of(case, cus())[0])
    after = stats(nt)
    # the launches were the planned ones: per row of the table their number, and launch for launch the regimes
    want = {}
    for x in plan:
        w = want.setdefault(x["row"], dict(launches=0, **{r: 0 for r in kc.REGIMES}))
        w["launches"] += 1
        for r in x["regimes"]:
            w[r] += 1
    for row in after:
        got = dict(launches=after[row]["launches"] - before[row]["launches"], **{r: after[row]["regime"][r] - before[row]["regime"][r] for r in kc.REGIMES})
        assert got == want.get(row, dict(launches=0, **{r: 0 for r in kc.REGIMES})), (name, row, got)
    last = plan[-1]
    s = after[last["row"]]
    assert (s["last_wpb"], s["last_grid"], s["last_stride"], s["last_n_slots"]) == (last["wpb"], last["grid"], last["stride"], last["n_slots"]), (name, s)
    assert kc.claims(case, cus()) >= kc.claims(case), name  # (what the host file counted on with the MI355X's CUs holds on this device)
    # with the launched shape the kernel reaches every path the host file counted on for this case
    assert kc.paths(case, s["last_grid"], s["last_wpb"], cus()) >= kc.paths(case), name
