"""The engine as a state machine on the device: every sequence of tests/engine_seq_model.py on every engine form where it is legal, in three placements —
the null stream with engine-owned buffers, a caller stream (ntc_config::stream), and a caller stream with caller-owned sketch and F1 (ext_sketch /
ext_f1).  After every finish, and after the last operation, t_Counter, the value histograms and F1 equal the model exactly; the caller's buffers are
read directly behind every flush and finish.  With profiling on, ntc_kernel_time's launch count and ntc_apply_time's applies pin the model's
pending-state tracker after every operation (which waits for the stream each time); with profiling off nothing waits between the operations, and the
results must be the same.

All test-side device work — uploads, scribbles, external adds — runs on the engine's stream and is never waited for by the host: a missing stream
dependency inside the engine shows as a wrong count.  A scribble overwrites a batch's device buffer with OTHER reads (another seed), so a batch read after
the engine gave it back counts wrong; host batches are overwritten the moment the submit returns.

Every sequence runs on every form where it is legal, in all three placements, with and without profiling.  The nodefer_* sequences are legal only on the
form created without NTC_FLAG_DEFER_REDO: there every device route is followed by a scribble of its batch with no call in between."""
import functools
import os

import numpy as np
import pytest

import engine_seq_model as m
import hll_model
import sig_model
import support
from devview import DevArray
from gpu_support import nt, upload  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PLACEMENTS = ("null", "stream", "stream_ext")
ERR_STATE = -4


# ---- host images of the named batches per layout, pristine and "other reads" (alt), pinned once ----
def _alt_equal(name):
    n, L, seed, p_bad, alpha = m.EQUAL[name]
    return support.random_reads(np.random.default_rng(seed + 1000), n, L, 0.003)


def _alt_bin(name):
    chunks, n = m.bin_chunks(name), m.n_reads(name)
    rng = np.random.default_rng(sum(name.encode()) + 5000)
    lens = rng.integers(16 * chunks - 15, 16 * chunks + 1, size=n)
    full = support.random_reads(rng, n, 16 * chunks, 0.003)
    return [full[j, :lens[j]].tobytes() for j in range(n)]


def slot_stride(L):
    return (L + 3) & ~3


@functools.lru_cache(maxsize=None)
def host_image(name, layout, alt=False):
    """-> tuple of pinned host tensors: (tiles,) / (slots,) / (tiles, tails) / (bytes,)"""
    if layout == "tiles":
        arrs = (support.tile_array(_alt_equal(name) if alt else m.equal_array(name)),)
    elif layout == "slots":
        a = _alt_equal(name) if alt else m.equal_array(name)
        arrs = (support.to_slots([a[i].tobytes() for i in range(a.shape[0])], slot_stride(a.shape[1])),)
    elif layout == "ragged":
        tiles, tails = support.tile_ragged(_alt_bin(name) if alt else list(m.reads_of(name)), m.bin_chunks(name))
        arrs = (tiles, tails.view(np.int32).reshape(-1))
    else:  # "long": three bytes in front (offsets of any alignment), one behind
        seqs = m.reads_of(name)
        body = b"".join(seqs)
        if alt:
            body = support.random_reads(np.random.default_rng(77), 1, len(body), 0.003)[0].tobytes()
        arrs = (np.frombuffer(b"###" + body + b"#", dtype=np.uint8).copy(),)
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in arrs)


@functools.lru_cache(maxsize=None)
def sig_increment(name, k):
    h, c = sig_model.model(m.reads_of(name), k)
    return h, c


class Run:
    """one engine of a form in a placement, its device buffers and its model (expected state and tracker)"""

    def __init__(self, nt, form, placement, profiling, device=0):
        self.nt, self.form, self.placement, self.profile, self.device = nt, form, placement, profiling, device
        self.ex, self.t = m.Expected(form.cfg), m.Tracker(form, profiling)
        self.bufs, self.keep, self.sibs, self.view = {}, [], [], None
        self.cp = None  # the sequence's precomputed checkpoints (engine_seq_model.checkpoints); None: the expected state is accumulated as the run goes (siblings)
        self.finishes = 0
        with torch.cuda.device(device):
            self.stream = torch.cuda.Stream() if placement != "null" else None
            self.ext = self.ext_f1 = None
            if placement == "stream_ext":
                with self.on_stream():  # garbage in front of create: the contents are the engine's from ntc_create on, which zeroes them
                    self.ext = torch.full((len(form.klist) * (2 << form.r_bits),), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
                    self.ext_f1 = torch.full((len(form.klist),), 0x5a5a5a5a5a, dtype=torch.int64, device="cuda")
            self.e = nt.Engine(form.klist, gap=form.gap, r_bits=form.r_bits, s_bits=m.S_BITS, device=device,
                               stream=self.stream.cuda_stream if self.stream is not None else None, ext_sketch=self.ext, ext_f1=self.ext_f1, flags=form.flags,
                               log_entries=form.log_entries, strand=form.strand, strand_tiled=form.strand_tiled, signature=form.signature)
            if profiling:
                self.e.set_profiling(True)

    def on_stream(self):
        return torch.cuda.stream(self.stream if self.stream is not None else torch.cuda.default_stream(self.device))

    def restart(self):
        """a used engine for the next sequence: ntc_reset makes it the engine ntc_create made, but for the sizes of its scratch (the tracker keeps those)"""
        self.e.reset()
        self.e.set_profiling(self.profile)
        old = self.t
        self.ex, self.t = m.Expected(self.form.cfg), m.Tracker(self.form, self.profile)
        self.t.set_cap, self.t.sets_sus = old.set_cap, old.sets_sus
        self.finishes, self.view = 0, None
        self.keep.clear()  # (the reset has waited for the stream)
        self.check_ext("a used engine, reset", zero=True)
        for s in self.sibs:
            s.restart()

    def close(self):
        for s in self.sibs:
            s.close()
        self.e.close()  # (waits for the stream: nothing reads the buffers any more)
        self.bufs.clear()
        self.keep.clear()

    # -- device buffers --
    def buf(self, name, layout):
        """the batch on the device in that layout: uploaded on the engine's stream at first use, restored there after a scribble"""
        key = (name, layout)
        src = host_image(name, layout)
        st = self.stream if self.stream is not None else torch.cuda.default_stream(self.device)
        with torch.cuda.device(self.device):
            if key not in self.bufs:
                self.bufs[key] = [[upload(p, st)[0] for p in src], False]
            ts, dirty = self.bufs[key]
            if dirty:
                for t_, p in zip(ts, src):
                    upload(p, st, into=t_)
                self.bufs[key][1] = False
        assert ts[0].data_ptr() % 16 == 0
        return ts

    def scribble(self, names):
        with torch.cuda.device(self.device), self.on_stream():
            for (name, layout), entry in self.bufs.items():
                if name in names:
                    for t_, p in zip(entry[0], host_image(name, layout, True)):
                        upload(p, torch.cuda.current_stream(), into=t_)
                    entry[1] = True

    def bin_args(self, b):
        if b in m.EQUAL:
            return (self.buf(b, "tiles")[0].data_ptr(), m.EQUAL[b][0], m.EQUAL[b][1], 0)
        tiles, tails = self.buf(b, "ragged")
        return (tiles.data_ptr(), m.n_reads(b), 16 * m.bin_chunks(b), tails.data_ptr())

    # -- the checks --
    def check_finish(self, what):
        tc, ph, f1 = self.e.finish(counters=True)
        self.finishes += 1
        off = int((tc != self.ex.tc).sum())
        assert np.array_equal(f1, self.ex.f1), (what, "F1", f1.tolist(), self.ex.f1.tolist(), "counters off", off)
        assert off == 0, (what, "counters off", off, "engine sum", int(tc.sum(dtype=np.int64)), "model sum", int(self.ex.tc.sum(dtype=np.int64)))
        for ki in range(len(self.form.klist)):
            assert np.array_equal(ph[ki], self.ex.hist(ki)), (what, "value histogram", ki)
        self.check_ext(what)

    def check_ext(self, what, zero=False):
        """the caller's buffers, read directly: the counters before the wrap, F1"""
        if self.ext is None:
            return
        self.stream.synchronize()
        sk = self.ext.cpu().numpy().view(np.uint32).reshape(self.ex.tc.shape)
        f1 = self.ext_f1.cpu().numpy().view(np.uint64)
        want = np.zeros_like(self.ex.wide) if zero else self.ex.wide
        assert np.array_equal(f1, np.zeros_like(self.ex.f1) if zero else self.ex.f1), (what, "ext_f1", f1.tolist())
        assert np.array_equal(sk, want), (what, "ext_sketch off", int((sk != want).sum()))
        assert np.array_equal((sk & 0xffff).astype(np.uint16), self.ex.tc)

    def check_pins(self, what):
        t = self.t
        if not self.form.tracked:
            return
        if t.pin_applies:
            assert self.e.apply_time()[1] == t.applies, (what, "applies", self.e.apply_time()[1], "tracker", t.applies)
        if self.profile and t.pin_enq:
            got = self.e.kernel_time()[1]
            assert got == t.enq, (what, "submits enqueued", got, "tracker", t.enq, "submits", t.submits, "D", len(t.D))
            if not t.ever_off:  # the submits so far minus the waiting ones
                assert got == t.submits - len(t.D), (what, got, t.submits, len(t.D))

    # -- one operation --
    def step(self, op, what, at=None):
        """at: the operation's index in the sequence whose checkpoints self.cp holds"""
        e, kind = self.e, op[0]
        self.at = at
        if kind == "tiled":
            n, L = m.EQUAL[op[1]][:2]
            e.submit_tiled_device(self.buf(op[1], "tiles")[0].data_ptr(), n, L)
        elif kind == "ragged":
            tiles, tails = self.buf(op[1], "ragged")
            e.submit_tiled_ragged_device(tiles.data_ptr(), m.n_reads(op[1]), m.bin_chunks(op[1]), tails.data_ptr())
        elif kind == "bins":
            e.submit_tiled_bins_device([self.bin_args(b) for b in op[1]])
        elif kind == "slots":
            n, L = m.EQUAL[op[1]][:2]
            e.submit_device(self.buf(op[1], "slots")[0].data_ptr(), n, L, slot_stride(L))
        elif kind == "host":
            a = m.equal_array(op[1]).reshape(-1).copy()
            n, L = m.EQUAL[op[1]][:2]
            e.submit(a, np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
            a[:] = ord("C")  # free on return
        elif kind == "spans":
            buf, starts, lens = spans_image(op[1])
            buf = buf.copy()
            e.submit_spans(buf, starts, lens)
            buf[:] = ord("G")
        elif kind == "long_device":
            d, = self.buf(op[1], "long")
            e.submit_long_device(d.data_ptr(), support.offsets_of(m.reads_of(op[1]), 3))
        elif kind == "flush":
            e.flush()
        elif kind == "sync":
            e.sync()
        elif kind == "reset":
            e.reset()
        elif kind == "merge_counters":
            img = m.Expected(self.form.cfg)
            for b in op[1]:
                img.add(*m.increment(b, self.form.cfg))
            e.merge_counters(img.tc, img.f1)
        elif kind == "device_state":
            sk, n, f1p = e.device_state()
            assert n == len(self.form.klist) * (2 << self.form.r_bits) and (self.ext is None or (sk == self.ext.data_ptr() and f1p == self.ext_f1.data_ptr()))
            with torch.cuda.device(self.device):
                self.view = torch.as_tensor(DevArray(sk, n), device="cuda")
        elif kind == "external_add":
            with torch.cuda.device(self.device), self.on_stream():
                idx = torch.tensor(list(op[1]), dtype=torch.int64, device="cuda")
                val = torch.tensor(list(op[2]), dtype=torch.int32, device="cuda")
                self.view.index_add_(0, idx, val)
        elif kind == "export_replace":
            self.t.step(op, checked=True)  # (first: what the call must answer follows from the work it starts)
            expect_export = self.t.export_expected
            try:
                counts = e.log_export(op[1])
                offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
                with torch.cuda.device(self.device), self.on_stream():
                    keys = torch.empty(max(1, sum(counts)), dtype=torch.int32, device="cuda")
                self.keep.append(keys)
                assert e.log_export(op[1], keys.data_ptr(), offs) == counts
                e.log_replace(keys.data_ptr(), sum(counts))
                self.t.replaced(sum(counts))
                assert expect_export in ("ok", "either"), (what, "the export must be refused", expect_export)
            except self.nt.NtcError as err:
                assert err.code == ERR_STATE and expect_export in ("state", "either"), (what, str(err), expect_export)
        elif kind == "merge_devices":
            ndev = torch.cuda.device_count()
            sibs = []
            for i, seq in enumerate(op[1]):
                if i == len(self.sibs):  # (a sibling is used again by the next merge of the sequence: the merge has reset it, and it may keep counting)
                    self.sibs.append(Run(self.nt, self.form, self.placement, self.profile, device=(self.device + 1 + i) % ndev if self.spread else self.device))
                s = self.sibs[i]
                sibs.append(s)
                for j, o in enumerate(seq):
                    s.step(o, what + (" sibling", i, j))
            self.nt.merge_devices([e] + [s.e for s in sibs])
            if self.cp is None:
                self.ex.apply(op, [s.ex for s in sibs])
            else:
                self.ex = self.cp[0][self.at] or self.ex
                for s in sibs:
                    s.ex.zero()
            self.t.step(op, checked=True)
            for s in sibs:
                s.t.step(("reset",))
                s.check_finish(what + (" sibling after the merge",))
                s.t.step(("finish",))
            self.check_pins(what)
            return
        elif kind == "profiling":
            if self.profile:
                e.set_profiling(bool(op[1]))
        elif kind == "read_timers":
            ms, n = e.kernel_time()
            assert ms >= 0.0 and e.apply_time()[0] >= 0.0 and e.fixup_time() >= 0.0
        elif kind == "scribble":
            self.scribble(set(op[1]))
        if self.cp is None:
            self.ex.apply(op)
        else:
            self.ex = self.cp[0][self.at] or self.ex
        if not (kind == "profiling" and not self.profile) and kind != "export_replace":
            self.t.step(op, checked=True)
        if kind == "finish":
            self.check_finish(what)
        elif kind == "flush":
            self.check_ext(what)
        elif kind == "reset":
            self.check_ext(what, zero=True)
        self.check_pins(what)

    spread = False


_CP = {}


def checkpoints_of(form_name, name, seq):
    """the runs of one (form, sequence) follow one another: the last one's checkpoints are kept"""
    key = (form_name, name, seq)
    if key not in _CP:
        _CP.clear()
        _CP[key] = m.checkpoints(m.FORM[form_name], seq)
    return _CP[key]


@functools.lru_cache(maxsize=None)
def spans_image(name):
    return support.spans_of(list(m.reads_of(name)))


# Engines are kept between the sequences of a (form, placement, way of running) and reset: creating one allocates some fifty device buffers, and the suite runs
# thousands of sequences.  An engine whose counters were handed out (X outlives a reset) is closed behind its sequence, and the sequences about the sizes of
# the engine's scratch start on a new one, so new engines are run as well.  What a case meets therefore depends on the cases before it (a selection with -k,
# a failure that closed an engine): only in the sizes of the engine's scratch, which the tracker carries along (Run.restart) and which no result depends on.
# Every case must pass on a new engine too — NTC_SEQ_FRESH=1 in the environment runs them all that way, which is how to reproduce a failure alone.
POOL = {}
FRESH = ("sets_grow", "ninth_batch", "seventeen_batches")


@pytest.fixture(scope="module", autouse=True)
def engine_pool():
    yield
    for r in POOL.values():
        r.close()
    POOL.clear()


def run_sequence(nt, form, placement, profiling, seq, name, spread=False):
    key = (form.name, placement, profiling)
    fresh = spread or name in FRESH or os.environ.get("NTC_SEQ_FRESH") == "1"
    r = None if fresh else POOL.pop(key, None)
    if r is None:
        r = Run(nt, form, placement, profiling)
    else:
        r.restart()
    r.spread = spread
    r.cp = checkpoints_of(form.name, name, seq)
    done = False
    try:
        for i, op in enumerate(seq):
            r.step(op, (name, form.name, placement, "profiling" if profiling else "unwaited", i, op[0]), i)
        r.ex = r.cp[1]
        r.check_finish((name, form.name, placement, "the final finish"))
        if form.signature:
            hs = [sig_increment(b, form.klist[0]) for b in r.ex.sig]
            if hs:
                allh, inv = np.unique(np.concatenate([h for h, _ in hs]), return_inverse=True)
                want_c = np.bincount(inv, weights=np.concatenate([c for _, c in hs]).astype(np.float64), minlength=allh.size).astype(np.int64)
            else:
                allh, want_c = np.zeros(0, np.uint64), np.zeros(0, np.int64)
            h, c = r.e.signature(0)
            assert np.array_equal(h, allh) and np.array_equal(c.astype(np.int64), want_c), (name, "signature", h.size, allh.size)
        done = True
        return r.finishes
    finally:
        if done and not fresh and not r.t.X:
            POOL[key] = r
        else:
            r.close()


MODES = (True, False)  # profiling on: the pins, a wait per operation; off: nothing waited for

CASES = [(f.name, n) for f in m.FORMS for n, s in sorted(m.sequences().items()) if m.check_legal(f, s) is None]  # (x three placements x two ways of running each)


@pytest.mark.parametrize("form,name", CASES)
def test_sequence(nt, form, name):
    seq = m.sequences()[name]
    for placement in PLACEMENTS:
        for profiling in MODES:
            assert run_sequence(nt, m.FORM[form], placement, profiling, seq, name) >= 1


def test_the_case_list_is_whole():
    """every (form, placement, sequence) runs unless the model says why it cannot: the K1-only form's ragged tiled batches, and the batch of table-slot bytes
    on the forms of which some plane is the general kernel's"""
    skipped = [(f.name, n, m.check_legal(f, s)) for f in m.FORMS for n, s in m.sequences().items() if m.check_legal(f, s)]
    print(len(CASES) * len(PLACEMENTS), "(form, placement, sequence) cases, each with and without profiling;", len(skipped) * len(PLACEMENTS), "illegal:",
          sorted({(f, w.split(": ", 1)[1]) for f, _, w in skipped}))
    assert len(CASES) + len(skipped) == len(m.FORMS) * len(m.sequences())
    for f, n, w in skipped:
        assert ("ragged tiled batch needs" in w and f == "k64_defer") or ("takes the bytes 1, 3, 4, 5, 7" in w and not m.FORM[f].ts_all) or \
               ("stays unchanged" in w and n.startswith("nodefer_") and m.FORM[f].defer), (f, n, w)


def test_shared_helpers():
    """gpu_support.upload copies on the stream it is given, into a new or an existing tensor, without a host wait; devview.DevArray aliases device memory"""
    st = torch.cuda.Stream()
    a = np.arange(1 << 20, dtype=np.int32)
    t, pinned = upload(a, st)
    assert pinned.is_pinned() and t.is_cuda and t.dtype == torch.int32
    with torch.cuda.stream(st):
        twice = t * 2  # (ordered behind the copy by the stream alone)
    st.synchronize()
    assert np.array_equal(twice.cpu().numpy(), a * 2)
    t2, p2 = upload(a[::-1].copy(), st, into=t)
    assert t2 is t
    view = torch.as_tensor(DevArray(t.data_ptr(), 16), device="cuda")
    st.synchronize()
    assert view.tolist() == a[::-1][:16].tolist()
    view[3] = -7
    torch.cuda.synchronize()
    assert int(t[3]) == -7 and upload(p2, st)[1] is p2


# ---- ntc_merge_devices: two or three engines, each on a stream of its own, each with pending work of another class ----
MERGES = {
    "two": (("tiled", m.T), ("tiled", "b2049"), ("merge_devices", ((("bins", (m.T, m.T)), ("tiled", "c4096")),)), ("tiled", m.T), m.FIN),
    "three": (("bins", (m.T, "rag:0")), ("merge_devices", ((("tiled", "b2049"), ("flush",), ("tiled", "tiny2048")), (("tiled", "d5000"), ("sync",), ("host", "c4096")))),
              m.FIN, ("tiled", "e6200"), ("merge_devices", ((("tiled", "clean2048"),), (("tiled", m.T),) * 8)), m.FIN),
}


@pytest.mark.parametrize("form", ["k32_tiled_defer", "klist_tiled_defer", "k32_64_defer", "k32_sig_defer"])
@pytest.mark.parametrize("which", sorted(MERGES))
def test_merge_devices_with_pending_work(nt, form, which):
    assert m.check_legal(m.FORM[form], MERGES[which]) is None
    for spread in ([False, True] if torch.cuda.device_count() > 1 else [False]):
        for profiling in (True, False):
            run_sequence(nt, m.FORM[form], "stream_ext" if not spread else "stream", profiling, MERGES[which], which, spread=spread)


# ---- nthll on a caller stream ----
@functools.lru_cache(maxsize=None)
def hll_reads(seed, n=300, L=64):
    a = support.random_reads(np.random.default_rng(seed), n, L, 0.003)
    return tuple(a[i].tobytes() for i in range(n))


@functools.lru_cache(maxsize=None)
def hll_planes(seed, masks, n_bits):
    return hll_model.model(list(hll_reads(seed)), list(masks), 0, n_bits)


@pytest.mark.parametrize("masks,seeded", [(("1" * 32,), False), (("1110011100111", "1" * 24), True)])
def test_nthll_sequence_on_a_caller_stream(nt, masks, seeded):
    """slots, tiled, merge_devices, slots, finish, reset, slots, finish against tests/hll_model.py: registers are maxima, F1 adds"""
    n_bits, L = 10, 64
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    mk = (lambda st: nt.HllEngine.from_seeds(list(masks), n_bits=n_bits, stream=st.cuda_stream)) if seeded else (lambda st: nt.HllEngine(32, n_bits=n_bits, stream=st.cuda_stream))
    keep = []

    def slots(e, st, seed):
        t, p = upload(support.to_slots(list(hll_reads(seed)), L), st)
        keep.append((t, p))
        e.submit_device(t.data_ptr(), len(hll_reads(seed)), L, L)

    def tiled(e, st, seed):
        a = np.frombuffer(b"".join(hll_reads(seed)), dtype=np.uint8).reshape(-1, L)
        t, p = upload(support.tile_array(a), st)
        keep.append((t, p))
        e.submit_tiled_device(t.data_ptr(), a.shape[0], L)

    def want(seeds):
        regs = np.maximum.reduce([hll_planes(s, masks, n_bits)[0] for s in seeds])
        return regs, sum(hll_planes(s, masks, n_bits)[1] for s in seeds)

    def same(got, seeds, what):
        regs, f1 = want(seeds)
        assert np.array_equal(np.asarray(got[1]).reshape(-1), f1), (what, got[1], f1)
        assert np.array_equal(np.asarray(got[0]).reshape(regs.shape), regs), what

    a, b = mk(s0), mk(s1)
    try:
        slots(a, s0, 1)
        tiled(a, s0, 2)
        tiled(b, s1, 3)
        slots(b, s1, 4)
        nt.merge_devices([a, b])
        slots(a, s0, 5)
        same(a.finish(), (1, 2, 3, 4, 5), "after the merge")
        regs_b, f1_b = b.finish()
        assert not np.asarray(regs_b).any() and not np.asarray(f1_b).any()
        a.reset()
        slots(a, s0, 2)
        same(a.finish(), (2,), "after the reset")
    finally:
        a.close()
        b.close()
