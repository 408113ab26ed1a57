"""tests/engine_seq_model.py pinned without a GPU: the named batches are what the sequences need, the directed sequences reach every cell of the
(operation x pending class) table that the rules allow, the random ones are legal and reproducible, the tracker says what the header says at the
points the header names, and the accumulated expected state equals the oracle over the concatenated batches."""
import numpy as np
import pytest

import engine_seq_model as m
import orc

COVER = m.FORM[m.COVER_FORM]
CLASS_NAMES = sorted({m.class_name(*c) for c in m.CLASSES})


def walk(form, seq):
    """(operation, class before it) for every operation of the sequence"""
    t, out = m.Tracker(form), []
    for op in seq:
        out.append((op[0], t.klass()))
        t.step(op)
    return out


def test_named_batches():
    sizes = sorted(n for n, *_ in m.EQUAL.values())
    assert {2048, 2049, 4096} <= set(sizes) and any(5000 <= n <= 6200 for n in sizes) and sizes[-1] <= 6200
    assert {L for _, L, *_ in m.EQUAL.values()} == {40, 64, 97, 150}
    base = np.zeros(256, dtype=bool)
    base[list(b"ACGTUacgtu")] = True
    for name in m.EQUAL:
        a = m.equal_array(name)
        assert a.shape == m.EQUAL[name][:2]
        bad = float((~base[a]).mean())
        if name == "clean2048":
            assert bad == 0.0 and not np.isin(a, list(b"acgtu")).any()
        elif name == "slot2048":
            assert {1, 3, 4, 5, 7} <= set(np.unique(a).tolist())
        else:
            assert 0.0005 < bad < 0.004 and np.isin(a, list(b"N")).any() and np.isin(a, list(b"acgt")).any() and np.isin(a, list(b"RYKMSW")).any(), name
    for name, (_, bins) in m.RAGGED.items():
        assert 2 <= len(bins) <= 3
        for i, (chunks, n) in enumerate(bins):
            lens = {len(r) for r in m.reads_of(m.bin_name(name, i))}
            assert n >= 1024 and min(lens) == 16 * chunks - 15 and max(lens) == 16 * chunks and len(lens) == 16
        assert sorted(m.reads_of(name)) == sorted(r for i in range(len(bins)) for r in m.reads_of(m.bin_name(name, i)))
    lens = [len(r) for r in m.reads_of("long")]
    assert 4900 < lens[0] < 5100 and all(n < 1008 for n in lens[1:]) and any(n < 32 for n in lens) and len(lens) > 3
    # partial last tiles and exact multiples of a tile both occur
    assert any(n % 2048 == 0 for n in sizes) and any(n % 2048 for n in sizes)


def test_every_allowed_cell_of_the_table_is_reached(capsys):
    """the directed sequences on the all-tiled deferring engine: every (operation, class) cell but the unreachable ones, which no sequence reaches either"""
    seqs = m.sequences()
    directed = {n: s for n, s in seqs.items() if not n.startswith(("random_", "nodefer_"))}
    hit = {}
    for name, seq in directed.items():
        assert m.check_legal(COVER, seq) is None, name
        for cell in walk(COVER, seq):
            hit.setdefault(cell, name)
    for name, seq in seqs.items():
        if name.startswith("nodefer_"):
            continue
        for cell in walk(COVER, seq):
            assert cell[1] in CLASS_NAMES, (name, cell)       # a launch that waits for K1f has booked the log: F > 0 without G does not exist
            assert cell not in m.UNREACHABLE, (name, cell)
    assert len(CLASS_NAMES) == 24 and len(m.OPS) == 19
    # the cells each coverage chain was built for are the ones the tracker sees there
    for name, marks in m.cover_cells().items():
        cells = walk(COVER, seqs[name])
        for at, opname, klass in marks:
            assert cells[at] == (opname, klass), (name, at)
    with capsys.disabled():
        print("\n(operation x pending class) on %s: x reached, - unreachable" % COVER.name)
        print("%-15s" % "" + " ".join("".join(c).ljust(9) for c in CLASS_NAMES))
        for op in m.OPS:
            print("%-15s" % op + " ".join(("x" if (op, c) in hit else "-" if (op, c) in m.UNREACHABLE else "MISSING").ljust(9) for c in CLASS_NAMES))
        for cell, why in sorted(m.UNREACHABLE.items())[:1]:
            print("unreachable: external_add in every class with Z:", why)
    missing = [(op, c) for op in m.OPS for c in CLASS_NAMES if (op, c) not in hit and (op, c) not in m.UNREACHABLE]
    assert not missing, missing
    assert all(op == "external_add" and c[3] == "Z" for op, c in m.UNREACHABLE) and len(m.UNREACHABLE) == 12


def test_specific_sequences_are_there():
    s = m.sequences()
    for name in ("ninth_batch", "seventeen_batches", "nested_flush_host", "nested_flush_bins", "nested_flush_long", "sets_grow", "reset_with_deferred",
                 "exposed_reset", "merge_counters_ZG", "export_with_deferred", "export_with_suspects", "finish_twice", "sync_scribble_all"):
        assert name in s
    assert [op[0] for op in s["exposed_reset"]] == ["device_state", "external_add", "reset", "external_add", "tiled", "finish"]
    assert sum(op[0] == "tiled" for op in s["seventeen_batches"]) == 17
    # the nested flush: a route that recycles its staging while batches wait (D > 0) and launches await K1f (F > 0)
    for name, kind in (("nested_flush_host", "host"), ("nested_flush_bins", "bins"), ("nested_flush_long", "long_device")):
        assert any(op == kind and c[0] != "D0" and c[1] != "F0" for op, c in walk(COVER, s[name])), name
    # merge_counters in each of Z x G
    assert {(c[2], c[3]) for op, c in walk(COVER, s["merge_counters_ZG"]) if op == "merge_counters"} == {("g", "Z"), ("G", "Z"), ("g", "z"), ("G", "z")}
    # the sets grow while launches wait
    t, grew = m.Tracker(COVER), False
    for op in s["sets_grow"]:
        before = (t.set_cap, t.F)
        t.step(op)
        grew |= t.set_cap > before[0] > 0 and before[1] > 0
    assert grew
    assert any(op == "export_replace" and c[0] != "D0" for op, c in walk(COVER, s["export_with_deferred"]))
    # an export behind an exposed reset must be refused, one on a fresh engine must succeed
    t = m.Tracker(COVER)
    for op in s["exposed_reset_export"]:
        t.step(op)
        assert op[0] != "export_replace" or t.export_expected == "state"
    t = m.Tracker(COVER)
    for op in s["export_with_deferred"]:
        t.step(op)
        assert op[0] != "export_replace" or t.export_expected == "ok"


def test_the_tracker_says_what_the_header_says():
    """NTC_FLAG_DEFER_REDO: up to 8 tiled batches are hashed by one launch, started when the eighth arrives or when a flush, sync, finish, reset,
    ntc_merge_devices or ntc_device_state needs the counters; K1f behind up to 8 launches; ntc_merge_counters adds without starting them"""
    t = m.Tracker(COVER)
    for i in range(7):
        t.step(("tiled", m.T))
        assert (len(t.D), t.F, t.enq, t.G) == (i + 1, 0, 0, False)
    t.step(("tiled", m.T))
    assert (len(t.D), t.F, t.enq, t.G, t.Z) == (0, 8, 8, True, True)
    t.step(("tiled", m.T))
    assert (len(t.D), t.F, t.enq) == (1, 8, 8)
    t.step(("merge_counters", ("b2049",)))
    assert (len(t.D), t.F, t.enq, t.Z) == (1, 8, 8, False)
    for op in (("flush",), ("sync",), ("finish",), ("reset",), ("device_state",), ("merge_devices", ((("tiled", m.T),),))):
        u = m.Tracker(COVER)
        u.step(("tiled", m.T))
        u.step(("tiled", m.T))
        u.step(op)
        assert (len(u.D), u.F) == (0, 0), op
        assert u.enq == (0 if op[0] == "reset" else 2) and u.applies == (1 if op[0] in ("flush", "finish", "device_state", "merge_devices") else 0), op
    # the sk_exposed rule: once the counters are handed out, a reset does not make the next apply a writing one
    u = m.Tracker(COVER)
    u.step(("reset",))
    assert u.Z
    u.step(("device_state",))
    u.step(("reset",))
    assert u.X and not u.Z
    # legality: a deferring engine holds a device batch until sync / finish; an engine without the flag gives it back in stream order
    u = m.Tracker(COVER)
    u.step(("tiled", m.T))
    assert u.why_illegal(("scribble", (m.T,))) and u.why_illegal(("external_add", (1,), (1,)))
    u.step(("flush",))
    assert u.why_illegal(("scribble", (m.T,)))
    u.step(("sync",))
    assert u.why_illegal(("scribble", (m.T,))) is None
    v = m.Tracker(m.FORM["k32_tiled"])
    v.step(("tiled", m.T))
    assert v.why_illegal(("scribble", (m.T,))) is None and (len(v.D), v.F, v.enq) == (0, 0, 1)
    # a k list: three launches per batch over the eight sets
    w = m.Tracker(m.FORM["klist_tiled_defer"])
    w.step(("bins", (m.T,) * 8))
    assert w.F == 8 and w.k1f_runs == 2 and w.enq == 1
    # without a log nothing is ever pending, and the export must be refused
    x = m.Tracker(m.FORM["k32_direct_defer"])
    x.step(("tiled", m.T))
    x.step(("finish",))
    assert not x.G and x.applies == 0 and x.export_expect() == "state"
    assert m.Tracker(COVER).export_expect() == "ok"


@pytest.mark.parametrize("seed", m.RANDOM_SEEDS)
def test_random_sequences_are_legal_and_reproducible(seed):
    seq = m.random_sequence(seed)
    assert seq == m.random_sequence(seed) == m.sequences()["random_%d" % seed] and 12 <= len(seq) <= 20
    assert m.check_legal(COVER, seq) is None and m.seq_reads(seq) <= m.READ_CAP
    for f in m.FORMS:
        why = m.check_legal(f, seq)
        assert why is None or "ragged tiled batch needs" in why or "takes the bytes 1, 3, 4, 5, 7" in why, (f, why)


def test_scribble_without_a_wait_on_the_engine_without_the_flag():
    """the nodefer_* sequences: every scribble follows the submit of its batch with nothing in between, every device route is among them, they are legal on the
    form created without NTC_FLAG_DEFER_REDO and on no other"""
    s = {n: q for n, q in m.sequences().items() if n.startswith("nodefer_")}
    assert len(s) == 3
    routes = set()
    for name, seq in s.items():
        for f in m.FORMS:
            why = m.check_legal(f, seq)
            assert (why is None) == (f.name == m.NODEFER_FORM) and (why is None or "stays unchanged" in why or "non-bases" in why), (name, f, why)
        for prev, op in zip(seq, seq[1:]):
            if op[0] == "scribble":
                assert prev[0] in m.SUBMITS and set(op[1]) <= set(m.op_batches(prev)), (name, prev, op)
                routes.add(prev[0])
        assert any(op[0] in m.SUBMITS for op in seq[max(i for i, op in enumerate(seq) if op[0] == "scribble"):])  # more batches behind the last scribble
    assert routes == {"tiled", "ragged", "bins", "slots", "long_device"}
    # no other sequence scribbles a device batch without a wait: that is why these exist
    for name, seq in m.sequences().items():
        if name not in s:
            assert m.check_legal(COVER, seq) is None, name


def test_where_the_pins_stop(capsys):
    """per directed and random sequence on the cover form: the operation from which the tracker stops pinning the counts (it resumes at a reset)"""
    lines = []
    for name, seq in sorted(m.sequences().items()):
        if name.startswith(("cover_", "nodefer_")):
            continue
        t = m.Tracker(COVER)
        for i, op in enumerate(seq):
            was = t.pin_enq
            t.step(op)
            if was and not t.pin_enq:
                lines.append("%s: unpinned from operation %d (%s)" % (name, i, op[0]))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert any(l.startswith("nested_flush_long") for l in lines) and any(l.startswith("every_route") for l in lines)
    assert not any(l.startswith(("ninth_batch", "seventeen_batches", "reset_with_deferred", "merge_counters_ZG", "finish_twice", "nested_flush_host")) for l in lines)


def test_illegal_sequences_are_refused():
    for f, seq, word in ((COVER, (("tiled", m.T), ("scribble", (m.T,))), "unchanged"), (COVER, (("external_add", (1,), (1,)),), "ntc_device_state"),
                         (m.FORM["k64_defer"], (("ragged", "rag:0"),), "ragged"), (COVER, (("scribble", ("b2049",)),), "never submitted"),
                         (COVER, (("tiled", "rag:0"),), "equal-length"), (COVER, (("bins", (m.T,) * 9),), "up to 8"),
                         (COVER, (("slots", "slot2048"),), "non-bases"), (m.FORM["k32_64_defer"], (("tiled", "slot2048"),), "non-bases")):
        why = m.check_legal(f, seq)
        assert why and word in why, (seq, why)


def test_which_sequences_run_on_which_form(capsys):
    """every sequence is legal on every form but for three stated reasons; the cases the GPU module runs: three placements each, both ways of running"""
    rows, reasons = [], set()
    for f in m.FORMS:
        bad = [m.check_legal(f, s) for s in m.sequences().values()]
        bad = [w.split(": ", 1)[1] for w in bad if w]
        reasons |= set(bad)
        cases = 3 * sum(1 for n, q in m.sequences().items() if m.check_legal(f, q) is None)
        rows.append((f.name, len(m.sequences()) - len(bad), len(bad), cases))
    with capsys.disabled():
        print()
        for name, ok, no, cases in rows:
            print("%-22s %3d sequences run, %2d illegal, %3d cases over the placements" % (name, ok, no, cases))
        print("%d cases;" % sum(r[3] for r in rows), "reasons:", sorted(reasons))
    assert all(no == (0 if name == m.NODEFER_FORM else 3) for name, ok, no, _ in rows if m.FORM[name].ts_all) and len(reasons) == 3


def oracle_whole(form, seq):
    """the oracle over the concatenated batches since the last reset, plus the stated images"""
    reads, tc_extra, f1_extra = [], 0, 0
    klist, gap, _, r_bits, s_bits = form.cfg
    zero = np.zeros((len(klist), 2, 1 << r_bits), dtype=np.uint16)
    tc_extra, f1_extra = zero.copy(), np.zeros(len(klist), dtype=np.uint64)

    def whole(rs):
        return orc.sketch_reads(rs, list(klist), gap, r_bits, s_bits) if rs else (zero.copy(), np.zeros(len(klist), dtype=np.uint64))

    for op in seq:
        if op[0] in m.SUBMITS:
            for b in m.op_batches(op):
                reads += list(m.reads_of(b))
        elif op[0] == "reset":
            reads, tc_extra, f1_extra = [], zero.copy(), np.zeros(len(klist), dtype=np.uint64)
        elif op[0] == "merge_counters":
            tc, f1 = whole([r for b in op[1] for r in m.reads_of(b)])
            tc_extra += tc
            f1_extra += f1
        elif op[0] == "external_add":
            for i, v in zip(op[1], op[2]):
                tc_extra.reshape(-1)[i] += np.uint16(v & 0xffff)
        elif op[0] == "merge_devices":
            for s in op[1]:
                tc, f1 = oracle_whole(form, s)
                tc_extra += tc
                f1_extra += f1
    tc, f1 = whole(reads)
    return tc + tc_extra, f1 + f1_extra


WHOLE = [n for i, n in enumerate(sorted(m.sequences())) if not n.startswith("cover_") or i % 8 == 0]


@pytest.mark.parametrize("name", WHOLE)
def test_model_equals_the_oracle_as_a_whole(name):
    seq = m.sequences()[name]
    form = m.FORM["klist_tiled_defer"] if name in ("every_route", "random_101") else COVER
    ex, at_finish = m.run_expected(form, seq)
    tc, f1 = oracle_whole(form, seq)
    assert np.array_equal(ex.f1, f1) and np.array_equal(ex.tc, tc), name
    assert len(at_finish) == sum(op[0] == "finish" for op in seq)
    if not any(op[0] in ("external_add", "merge_devices") for op in seq):
        assert np.array_equal((ex.wide & 0xffff).astype(np.uint16), ex.tc)


def test_strand_and_gap_increments_are_the_oracles():
    """the one-strand form's increments come from tests/strand_model.py: the canonical pick of the same path is the oracle's; the gapped form is the oracle's -g"""
    cfg = ((32,), 0, "canonical", 14, m.S_BITS)
    tc, f1 = m.increment("b2049", cfg)
    import strand_model as sm
    key = (sm.CANONICAL, 14, m.S_BITS)
    got = sm.array_sketches(sm.pad_reads(m.reads_of("b2049")), "1" * 32, [key])[key]
    assert np.array_equal(got[0], tc) and np.array_equal(got[1], f1)
    fwd = m.increment("b2049", ((32,), 0, "forward", 14, m.S_BITS))
    assert np.array_equal(fwd[1], f1) and not np.array_equal(fwd[0], tc)
    g = m.increment("rag:0", ((12,), 2, "canonical", 14, m.S_BITS))
    assert g[1][0] > 0 and g[0].any()
