"""GPU tests of spaced seeds given as masks (include/ntcard_hip.h: ntc_create_seeded, ntc_hash_dump_seed_device; `ntcard --seed`):
hashes against the oracle's stHashIterator / NTMSM64 restatement with the mask's don't-care positions, sketches against that
restatement pushed through ntComp (ntcard.cpp:132-145), equivalences with plain k and with -g, every submit path, the CLI."""
import os
import random

import numpy as np
import pytest

import orc
from gpu_support import nt  # noqa: F401
from support import GOLD, NTCARD, mask_with, masks_for, rseq, run_cli, sketch_from_values, small_reads, to_slots

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def seed_hash(seq, mask):
    """-> (hashes u64[n], pos u32[n]): every valid window of the read under the mask (orc_sthash_read, NTMSM64 with m = m2 = 1)"""
    L = orc.lib()
    dc = np.array([i for i, c in enumerate(mask) if c == "0"] or [0], dtype=np.uint32)
    n_dc = mask.count("0")
    cap = max(len(seq), 1)
    h = np.zeros(cap, dtype=np.uint64)
    pos = np.zeros(cap, dtype=np.uint32)
    n = L.orc_sthash_read(seq, len(seq), len(mask), orc._ptr(dc), n_dc, orc._ptr(h), orc._ptr(pos), cap)
    return h[:n].copy(), pos[:n].copy()


def oracle_sketch(reads, masks, r_bits, s_bits):
    """t_Counter [n][2][1 << r_bits] (uint16, as the engine reports it) and F1 [n]: the oracle's hashes through ntComp"""
    return sketch_from_values([np.concatenate([seed_hash(r, m)[0] for r in reads] or [np.zeros(0, dtype=np.uint64)]) for m in masks], r_bits, s_bits)


SPANS = [1, 12, 31, 32, 33, 64, 97, 200]


@pytest.mark.parametrize("k", SPANS)
def test_hash_dump_matches_oracle(nt, k):
    rng = random.Random(7 * k)
    for L in sorted({max(1, k - 1), k, k + 5, 150, 151}):
        # equal-length waves (rolling form) and a partial last wave (ragged: closed-form XOR-out); reads with N make most waves DIRTY
        n = 64 * 3 + 37
        reads = [rseq(rng, L, pn=rng.choice([0.0, 0.0, 0.02])) for _ in range(n)]
        stride = (L + 3) & ~3
        d = torch.from_numpy(to_slots(reads, stride)).cuda()
        maxw = max(L - k + 1, 1)
        for m in masks_for(k):
            dh = torch.zeros(n * maxw, dtype=torch.int64, device="cuda")
            dc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            nt.hash_dump_seed_device(d.data_ptr(), n, L, stride, m, maxw, dh.data_ptr(), dc.data_ptr())
            torch.cuda.synchronize()
            hh = dh.cpu().numpy().view(np.uint64).reshape(n, maxw)
            cc = dc.cpu().numpy()
            for i, r in enumerate(reads):
                oh, _ = seed_hash(r, m)
                assert cc[i] == len(oh), (k, L, m, i)
                assert np.array_equal(hh[i, :len(oh)], oh), (k, L, m, i)


MIXED5 = ["1110011100111", "0111111111111111111111111111110", "1" * 24 + "0" * 4, "10" * 16 + "1", "1" * 20 + "0" * 9 + "1" * 35]


@pytest.mark.parametrize("masks", [["1110110111"], [mask_with(31, [0, 1, 14, 15, 16, 29, 30])], [("01" * 20)[:39] + "1"], MIXED5])
def test_sketch_matches_oracle_host_reads(nt, masks):
    """host submit: ragged reads (closed-form XOR-out), equal-length batches (rolling form), long sequences cut into overlapping chunks"""
    rng = random.Random(len(masks) * 31 + len(masks[0]))
    ragged = [rseq(rng, rng.choice([5, 30, 64, 100, 150, 151]), pn=rng.choice([0.0, 0.0, 0.01])) for _ in range(3000)]
    equal = [rseq(rng, 150, pn=rng.choice([0.0, 0.0, 0.005])) for _ in range(3000)]
    long = [rseq(rng, n, pn=0.001) for n in (5000, 20000)]
    reads = ragged + equal + long
    r_bits, s_bits = 16, 3
    with nt.Engine.from_seeds(masks, r_bits=r_bits, s_bits=s_bits) as e:
        e.submit_reads(ragged)
        e.submit_reads(equal)
        e.submit_reads(long)
        tc, ph, f1 = e.finish(counters=True)
    oc, of1 = oracle_sketch(reads, masks, r_bits, s_bits)
    assert np.array_equal(f1, of1)
    assert np.array_equal(tc, oc)
    if len(masks) > 1:  # every plane of a list equals an engine of that mask alone
        for mi, m in enumerate(masks):
            with nt.Engine.from_seeds([m], r_bits=r_bits, s_bits=s_bits) as e:
                e.submit_reads(reads)
                tc1, _, f11 = e.finish(counters=True)
            assert f11[0] == f1[mi] and np.array_equal(tc1[0], tc[mi])


def test_sketch_matches_oracle_row_slots_and_tiles(nt):
    """device-resident row slots, tiled batches (K1h for the plain and -g planes, row slots for the rest) and ragged tiled batches"""
    rng = random.Random(5)
    masks = ["1" * 32, "111110011111", "1110011100111", "0" + "1" * 30 + "0", "1" * 13 + "0" * 5 + "1" * 13]
    r_bits, s_bits = 16, 7  # (sBits >= 7: K1h takes the plain and the (12, 2) planes of tiled batches)
    n, L = 5000, 150
    reads = [rseq(rng, L, pn=rng.choice([0.0, 0.0, 0.003])) for _ in range(n)]
    oc, of1 = oracle_sketch(reads, masks, r_bits, s_bits)
    stride = 152
    d = torch.from_numpy(to_slots(reads, stride)).cuda()
    with nt.Engine.from_seeds(masks, r_bits=r_bits, s_bits=s_bits) as e:
        e.submit_device(d.data_ptr(), n, L, stride)
        tc, _, f1 = e.finish(counters=True)
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
    tiles = torch.from_numpy(nt.tile_reads(reads, L)).cuda()
    with nt.Engine.from_seeds(masks, r_bits=r_bits, s_bits=s_bits) as e:
        e.submit_tiled_device(tiles.data_ptr(), n, L)
        tc, _, f1 = e.finish(counters=True)
    assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
    # ragged tiled batches (reads of 145..160 bases, 10 chunks)
    rr = [rseq(rng, rng.randint(145, 160), pn=rng.choice([0.0, 0.0, 0.003])) for _ in range(n)]
    orr, ofr = oracle_sketch(rr, masks, r_bits, s_bits)
    t, tails, _ = nt.tile_reads_ragged(rr, 10)
    dt, dtl = torch.from_numpy(t).cuda(), torch.from_numpy(tails).cuda()
    for sel in (masks, masks[2:4]):  # with K1h planes, and a list no plane of which is K1h's
        idx = [masks.index(m) for m in sel]
        with nt.Engine.from_seeds(sel, r_bits=r_bits, s_bits=s_bits) as e:
            e.submit_tiled_ragged_device(dt.data_ptr(), n, 10, dtl.data_ptr())
            tc, _, f1 = e.finish(counters=True)
        assert np.array_equal(f1, ofr[idx]) and np.array_equal(tc, orr[idx])


def test_all_ones_mask_is_plain_k(nt):
    rng = random.Random(11)
    reads = [rseq(rng, rng.choice([40, 150]), pn=0.005) for _ in range(4000)]
    for k in (12, 32, 45):
        with nt.Engine([k], r_bits=18, s_bits=5) as e:
            e.submit_reads(reads)
            tc0, ph0, f10 = e.finish(counters=True)
        with nt.Engine.from_seeds(["1" * k], r_bits=18, s_bits=5) as e:
            e.submit_reads(reads)
            tc1, ph1, f11 = e.finish(counters=True)
        assert np.array_equal(f10, f11) and np.array_equal(tc0, tc1) and np.array_equal(ph0, ph1)


def test_symmetric_masks_are_the_gap_seeds(nt):
    reads = small_reads()
    n, L = 4096, 150
    rng = random.Random(2)
    eq = [rseq(rng, L) for _ in range(n)]
    tiles = torch.from_numpy(nt.tile_reads(eq, L)).cuda()
    # 111110011111 is -k 12 -g 2 and reaches K1h (NTC_FLAG_REQUIRE_TILED); 1^13 0^5 1^13 is -k 31 -g 5 (K1)
    for mask, k, gap, flags in (("111110011111", 12, 2, nt.FLAG_REQUIRE_TILED), ("1" * 13 + "0" * 5 + "1" * 13, 31, 5, 0)):
        with nt.Engine([k], gap=gap, r_bits=20, s_bits=7) as e:
            e.submit_reads(reads)
            e.submit_tiled_device(tiles.data_ptr(), n, L)
            tc0, ph0, f10 = e.finish(counters=True)
        with nt.Engine.from_seeds([mask], r_bits=20, s_bits=7, flags=flags) as e:
            e.submit_reads(reads)
            e.submit_tiled_device(tiles.data_ptr(), n, L)
            tc1, ph1, f11 = e.finish(counters=True)
        assert np.array_equal(f10, f11) and np.array_equal(tc0, tc1) and np.array_equal(ph0, ph1), mask


def test_require_tiled_refuses_a_general_mask(nt):
    n, L = 2048, 150
    rng = random.Random(3)
    tiles = torch.from_numpy(nt.tile_reads([rseq(rng, L) for _ in range(n)], L)).cuda()
    with nt.Engine.from_seeds(["1" * 32, "1110011100111"], r_bits=18, s_bits=7, flags=nt.FLAG_REQUIRE_TILED) as e:
        with pytest.raises(nt.NtcError, match="REQUIRE_TILED"):
            e.submit_tiled_device(tiles.data_ptr(), n, L)
        tc, _, f1 = e.finish(counters=True)
    assert not f1.any() and not tc.any()


def test_merge_devices_compares_seed_lists(nt):
    rng = random.Random(4)
    reads = [rseq(rng, 150) for _ in range(3000)]
    masks = ["1110011100111", "1" * 21]
    oc, of1 = oracle_sketch(reads, masks, 16, 5)
    es = [nt.Engine.from_seeds(masks, r_bits=16, s_bits=5) for _ in range(3)]
    try:
        for i, e in enumerate(es):
            e.submit_reads(reads[i::3])
        nt.merge_devices(es)
        tc, _, f1 = es[0].finish(counters=True)
        assert np.array_equal(f1, of1) and np.array_equal(tc, oc)
        with nt.Engine.from_seeds(["1110011100111", "1" * 10 + "0" + "1" * 10], r_bits=16, s_bits=5) as other:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], other])
        with nt.Engine([13, 21], r_bits=16, s_bits=5) as plain:
            with pytest.raises(nt.NtcError, match="not configured like"):
                nt.merge_devices([es[0], plain])
    finally:
        for e in es:
            e.close()


def test_cli_seed_reproduces_the_reference_gap_output(tmp_path):
    """the one check anchored directly on the reference binary: `ntcard -k 12 -g 2` (tests/golden/ref_k12_g2__out_k12.hist)"""
    src = os.path.join(GOLD, "reads_small.fq.gz")
    r = run_cli(NTCARD, ["--seed", "111110011111", "-p", "x", src], cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "x_seed1_k12.hist").read_bytes() == open(os.path.join(GOLD, "ref_k12_g2__out_k12.hist"), "rb").read()


def test_cli_seed_compact_output_matches_the_oracle(tmp_path):
    masks = ["1110011100111", "0111111111111111111111111111110", "1" * 20]
    src = os.path.join(GOLD, "reads_small.fq.gz")
    r = run_cli(NTCARD, ["--seed=" + ",".join(masks), "-c", "50", "-o", "out.tsv", src], cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = (tmp_path / "out.tsv").read_text().splitlines()
    assert rows[0] == "seed\tf\tn" and len(rows) == 1 + 3 * 50
    reads = small_reads()
    oc, of1 = oracle_sketch(reads, masks, 27, 7)
    err = r.stderr.decode()
    for mi in range(3):
        F0, f = orc.comp_est_p(orc.value_hist(oc[mi], 27), 27, 7, 50)
        assert "seed=%d\tF1\t%d\n" % (mi + 1, of1[mi]) in err
        assert "seed=%d\tF0\t%d\n" % (mi + 1, int(F0)) in err
        assert rows[1 + 50 * mi: 1 + 50 * (mi + 1)] == ["%d\t%d\t%d" % (mi + 1, i, int(f[i])) for i in range(1, 51)]
