"""Model of the engine as a state machine (include/ntcard_hip.h, ntcard_amd/csrc/ntc_engine.hpp): sequences of operations as data, the state they
must leave, which of them are legal, and what work is pending after each.  Host only: numpy and the oracle, no torch, no GPU.
tests/test_engine_seq_host.py pins this module (coverage of the operation x pending-class table, the model against the oracle as a whole);
tests/test_engine_seq_gpu.py runs every sequence on the engine.

An operation is a tuple:
    ("tiled", batch) ("ragged", bin) ("bins", (batch | bin, ...)) ("slots", batch) ("host", batch) ("spans", ragged set) ("long_device", long set)
    ("flush",) ("sync",) ("finish",) ("reset",)
    ("merge_counters", (batch, ...))        the t_Counter image and F1 of those batches are added
    ("device_state",) ("external_add", indices, values)      the second is legal only after the first
    ("export_replace", n_parts)             every part of the pending log exported and handed back as the pending log: a no-op on the result
    ("merge_devices", (sequence, ...))      one sibling engine per sequence, each run before the merge
    ("profiling", on) ("read_timers",)
    ("scribble", (batch, ...))              the device buffers of earlier batches are overwritten with other valid reads
"""
import functools
import random

import numpy as np

import orc
import strand_model as sm
import support

# ---- flags (include/ntcard_hip.h) ----
ALWAYS_LOG, PARTITION_ALWAYS, REQUIRE_TILED, DEFER_REDO, DIRECT_ATOMICS = 8, 16, 64, 128, 2
STRAND_FORWARD, STRAND_TILED = 512, 4096
S_BITS = 7

SUBMITS = ("tiled", "ragged", "bins", "slots", "host", "spans", "long_device")
OPS = SUBMITS + ("flush", "sync", "finish", "reset", "merge_counters", "device_state", "external_add", "export_replace", "merge_devices", "profiling",
                 "read_timers", "scribble")


# ---- named batches, each built from a seed ----
# equal-length batches: name -> (reads, read length, seed, rate of bad bytes, alphabet of the bad draw)
_BAD = b"ACGTNnacgtRYKMSW"
EQUAL = {
    "a2048": (2048, 150, 11, 0.003, _BAD),
    "b2049": (2049, 97, 12, 0.003, _BAD),
    "c4096": (4096, 64, 13, 0.003, _BAD),
    "d5000": (5000, 150, 14, 0.003, _BAD),
    "e6200": (6200, 40, 15, 0.003, _BAD),
    "slot2048": (2048, 97, 16, 0.004, b"ACGT\x01\x03\x04\x05\x07"),  # the table-slot bytes: K1f's slow path
    "clean2048": (2048, 64, 17, 0.0, _BAD),                        # no bad byte at all
    "big6144": (6144, 150, 18, 0.003, _BAD),                        # more tiles and longer reads than the small ones: the hand-over sets grow
    "tiny2048": (2048, 40, 19, 0.003, _BAD),
}
RAGGED = {"rag": (20, ((6, 1024), (7, 1100), (10, 1500)))}  # name -> (seed, ((chunks of the bin, reads), ...)): bins of at least 1024 reads
LONG = {"long": (21, (5003, 700, 33, 31, 150, 1007))}        # name -> (seed, lengths): one sequence of five pieces, the others shorter than a piece


def bin_name(name, i):
    return "%s:%d" % (name, i)


RAGGED_BINS = [bin_name(n, i) for n, (_, bins) in RAGGED.items() for i in range(len(bins))]


@functools.lru_cache(maxsize=None)
def equal_array(name):
    """(n, L) uint8, read-only"""
    n, L, seed, p_bad, alpha = EQUAL[name]
    a = support.random_reads(np.random.default_rng(seed), n, L, p_bad, np.frombuffer(alpha, dtype=np.uint8))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """the reads of any named batch, bin, ragged set or long set: a tuple of bytes"""
    if name in EQUAL:
        a = equal_array(name)
        return tuple(a[i].tobytes() for i in range(a.shape[0]))
    if name in LONG:
        seed, lens = LONG[name]
        rng = random.Random(seed)
        return tuple(support.rseq(rng, n, pn=0.003) for n in lens)
    if ":" in name:
        base, i = name.split(":")
        seed, bins = RAGGED[base]
        chunks, n = bins[int(i)]
        rng = np.random.default_rng(seed * 100 + int(i))
        lens = rng.integers(16 * chunks - 15, 16 * chunks + 1, size=n)
        full = support.random_reads(rng, n, 16 * chunks, 0.003, np.frombuffer(_BAD, dtype=np.uint8))
        return tuple(full[j, :lens[j]].tobytes() for j in range(n))
    # a ragged set: its bins interleaved, as a parser would deliver them
    parts = [reads_of(bin_name(name, i)) for i in range(len(RAGGED[name][1]))]
    out = [r for p in parts for r in p]
    random.Random(RAGGED[name][0]).shuffle(out)
    return tuple(out)


def n_reads(name):
    return EQUAL[name][0] if name in EQUAL else len(reads_of(name))


def bin_chunks(name):
    base, i = name.split(":")
    return RAGGED[base][1][int(i)][0]


def op_batches(op):
    """the named batches an operation submits (merge_counters: those of its image)"""
    if op[0] in ("tiled", "ragged", "slots", "host", "spans", "long_device"):
        return (op[1],)
    if op[0] in ("bins", "merge_counters"):
        return tuple(op[1])
    return ()


def op_reads(op):
    return sum(n_reads(b) for b in op_batches(op)) if op[0] in SUBMITS else 0


def seq_reads(seq):
    return sum(op_reads(op) + (sum(seq_reads(s) for s in op[1]) if op[0] == "merge_devices" else 0) for op in seq)


# ---- engine forms (tests/test_engine_seq_gpu.py creates them; r_bits 14 .. 16, s_bits 7) ----
class Form:
    def __init__(self, name, klist, flags, gap=0, r_bits=14, strand=None, strand_tiled=False, log_entries=0, signature=False, what=""):
        self.name, self.klist, self.flags, self.gap, self.r_bits, self.strand = name, list(klist), flags, gap, r_bits, strand
        self.strand_tiled, self.log_entries, self.signature, self.what = strand_tiled, log_entries, signature, what
        self.defer = bool(flags & DEFER_REDO)
        self.require_tiled = bool(flags & REQUIRE_TILED)
        self.has_log = not flags & DIRECT_ATOMICS
        tiled_k = [12 <= k <= 32 for k in self.klist]
        # every plane the tiled kernels' (include/ntcard_hip.h: ntc_submit_tiled_device, NTC_FLAG_STRAND_TILED, NTC_FLAG_SIGNATURE)
        self.ts_all = all(tiled_k) and not signature and (strand is None or strand_tiled) and (gap == 0 or (self.klist[0], gap) in ((12, 2), (32, 8)))
        self.ts_ok = any(tiled_k) and not signature and (strand is None or self.ts_all)
        # the tracker below is the all-tiled engine's; on the other forms only the results are compared
        self.tracked = self.ts_all
        # ntc_log_export_device succeeds only while the sketch holds the reset's zeros and no kernel has incremented it directly: a small log runs out of
        # regions, an adaptive engine may switch to atomics — there the model cannot say which, and accepts the refusal as well
        self.export_certain = self.ts_all and self.has_log and not log_entries

    @property
    def cfg(self):
        return (tuple(self.klist), self.gap, self.strand or "canonical", self.r_bits, S_BITS)

    def log_cap(self):
        """entries of the hit log (include/ntcard_hip.h: ntc_config::log_entries: four per counter by default, at least 2^18)"""
        counters = len(self.klist) * (2 << self.r_bits)
        cap = self.log_entries or min(1 << 30, max(1 << 18, 4 * counters))
        cap = max(cap, 1 << 14)
        region = min(32768, max(256, cap // 8192))
        return max(1, cap // region) * region

    def __repr__(self):
        return self.name


FORMS = [
    Form("k32_tiled_defer", [32], REQUIRE_TILED | DEFER_REDO, what="all-tiled, deferring"),
    Form("k32_tiled", [32], REQUIRE_TILED, r_bits=15, what="all-tiled, K1f at once"),
    Form("klist_tiled_defer", [21, 25, 31], REQUIRE_TILED | DEFER_REDO, r_bits=16, what="3 launches per batch over 8 sets"),
    Form("k32_64_defer", [32, 64], DEFER_REDO, what="K1's share from the same tiles; ts_all is false, so nothing defers"),
    Form("k32_forward_defer", [32], DEFER_REDO, strand="forward", strand_tiled=True, what="one-strand pair"),
    Form("gap12_2_defer", [12], REQUIRE_TILED | DEFER_REDO, gap=2, what="gapped K1h"),
    Form("k32_smalllog_defer", [32], ALWAYS_LOG | PARTITION_ALWAYS | DEFER_REDO, log_entries=1 << 18, what="applies forced in mid-sequence by the log's booking"),
    Form("k32_direct_defer", [32], DIRECT_ATOMICS | DEFER_REDO, what="no log: export_replace must fail"),
    Form("k64_defer", [64], DEFER_REDO, what="K1 only: the flag must change nothing"),
    Form("k32_sig_defer", [32], DEFER_REDO, signature=True, what="signature inserts in sync / finish, tiled batches re-laid out"),
]
FORM = {f.name: f for f in FORMS}


# ---- the increments: what one named batch adds, computed once per configuration and never changed ----
@functools.lru_cache(maxsize=None)
def increment(name, cfg):
    """-> (t_Counter uint16 [nk][2][1 << r_bits], F1 uint64 [nk]) of one named batch under cfg = (klist, gap, strand, r_bits, s_bits)"""
    klist, gap, strand, r_bits, s_bits = cfg
    reads = reads_of(name)
    if strand == "canonical":
        tc, f1 = orc.sketch_reads(list(reads), list(klist), gap, r_bits, s_bits)
    else:
        arr = sm.pad_reads(reads)
        key = (sm.STRANDS[strand], r_bits, s_bits)
        per = [sm.array_sketches(arr, sm.gap_mask(k, gap), [key])[key] for k in klist]
        tc, f1 = np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per])
    tc.setflags(write=False)
    f1.setflags(write=False)
    return tc, f1


class Expected:
    """the accumulating expected state of one engine: uint16 counters with wrapping adds, uint64 F1; `wide`: the counters before the wrap, as the device's
    uint32 words hold them (after ntc_merge_devices engine 0 holds the sums mod 2^16, and so does `wide`)"""

    def __init__(self, cfg):
        self.cfg = cfg
        nk, r_bits = len(cfg[0]), cfg[3]
        self.tc = np.zeros((nk, 2, 1 << r_bits), dtype=np.uint16)
        self.f1 = np.zeros(nk, dtype=np.uint64)
        self.wide = np.zeros(self.tc.shape, dtype=np.uint32)
        self.sig = []  # the named batches whose sampled values the signature holds (NTC_FLAG_SIGNATURE)

    def add(self, tc, f1=None):
        self.tc += tc  # (uint16: wraps)
        self.wide += tc
        if f1 is not None:
            self.f1 += f1

    def zero(self):
        self.tc[:] = 0
        self.f1[:] = 0
        self.wide[:] = 0
        self.sig = []

    def apply(self, op, others=()):
        """others: the Expected of the sibling engines of a merge_devices, already run"""
        kind = op[0]
        if kind in SUBMITS:
            for b in op_batches(op):
                self.add(*increment(b, self.cfg))
                self.sig.append(b)
        elif kind == "reset":
            self.zero()
        elif kind == "merge_counters":
            for b in op[1]:
                self.add(*increment(b, self.cfg))
        elif kind == "external_add":
            flat, wide = self.tc.reshape(-1), self.wide.reshape(-1)
            for i, v in zip(op[1], op[2]):
                flat[i] += np.uint16(v & 0xffff)
                wide[i] += np.uint32(v)
        elif kind == "merge_devices":
            for o in others:
                self.add(o.tc, o.f1)
                self.sig += o.sig
                o.zero()
            self.wide = self.tc.astype(np.uint32)  # (engine 0's counters afterwards hold their value mod 2^16)
        # everything else leaves the state alone: flush, sync, finish, device_state, export_replace, profiling, read_timers, a legal scribble

    def hist(self, ki):
        return orc.value_hist(self.tc[ki], self.cfg[3])


class Snap:
    """the expected state at one point of a sequence, frozen: what a check compares with (the histograms are computed when first asked for)"""

    def __init__(self, ex):
        self.cfg, self.tc, self.f1, self.wide, self.sig = ex.cfg, ex.tc.copy(), ex.f1.copy(), ex.wide.copy(), tuple(ex.sig)
        self._hist = {}

    def hist(self, ki):
        if ki not in self._hist:
            self._hist[ki] = orc.value_hist(self.tc[ki], self.cfg[3])
        return self._hist[ki]


def checkpoints(form, seq):
    """-> ([per operation: the Snap behind a finish, flush or reset, else None], the Snap behind the last operation): computed once per (form, sequence) and
    shared by the runs of that sequence in every placement, with and without profiling"""
    ex, out = Expected(form.cfg), []
    for op in seq:
        ex.apply(op, [run_expected(form, s)[0] for s in op[1]] if op[0] == "merge_devices" else ())
        out.append(Snap(ex) if op[0] in ("finish", "flush", "reset") else None)
    return out, Snap(ex)


def run_expected(form, seq):
    """the state after the whole sequence, and the state at every finish"""
    ex, at_finish = Expected(form.cfg), []
    for op in seq:
        others = [run_expected(form, s)[0] for s in op[1]] if op[0] == "merge_devices" else ()
        ex.apply(op, others)
        if op[0] == "finish":
            at_finish.append((ex.tc.copy(), ex.f1.copy()))
    return ex, at_finish


# ---- legality and the pending-state tracker ----
K1F_SETS = 8   # hand-over sets: K1h launches that may wait for K1f (include/ntcard_hip.h: NTC_FLAG_DEFER_REDO)
DEFER_MAX = 8  # tiled batches hashed by one launch: the eighth starts it


class Illegal(Exception):
    pass


class Tracker:
    """What is pending inside an engine after each operation, read from include/ntcard_hip.h and ntc_engine.hpp:
        D  tiled batches waiting for their hash launch (NTC_FLAG_DEFER_REDO: "up to 8 tiled batches ... started when the eighth arrives or when ntc_flush /
           ntc_sync / ntc_finish / ntc_reset / ntc_merge_devices / ntc_device_state needs the counters"), 0 .. 7
        F  K1h launches (one per batch and k) waiting for K1f ("the fix-up kernels K1f behind up to 8 launches"), 0 .. 8
        G  the hit log is pending ("applied to the sketch when it fills up and whenever the counters are needed")
        Z  the sketch still holds the reset's zeros: the first apply writes (ntc_engine.hpp: sk_host_dirty)
        X  ntc_device_state has handed the counters out ("after that call even a reset must make the next apply add")
    and two counts the engine reports: enq, the submits whose hash launch is enqueued while profiling (ntc_kernel_time), and applies (ntc_apply_time).
    "Fills up" is the one rule the header leaves open; the tracker takes ntc_engine.hpp's log_est — "host-side upper estimate of the entries logged since
    the last apply": per launch and k, reads x windows x 1.15 x 2^(1 - sBits), plus 64 regions' slack of 4096 — against 85 % of the capacity.  Where it
    cannot restate the estimate (row slots with a slot table, the long-sequence cut) it stops pinning the counts until the next reset (pin_applies,
    pin_enq); likewise from a launch that finds launches awaiting K1f AND batches waiting (F > 0, D > 0, outside a flush): whether a hand-over set must
    grow there — which runs K1f and with it the waiting batches — depends on sizes no header states (unsure).  tests/test_engine_seq_host.py
    (test_where_the_pins_stop) prints, per directed and random sequence, the operation from which it runs unpinned on the cover form — nested_flush_long and
    every_route from their long_device, the random sequences that hold a long_device or meet F > 0 with D > 0 — and asserts that the sequences about the
    eighth batch, resets, merges and host batches never do.  The estimate's constants (1.15, 64 x 4096, 85 %) and the rule for the sets'
    suspect lists restate ntc_launch.hip, not the header: a retuning there moves these pins without any change of contract, and this is the place to follow it.  It is the tracker of an engine whose every plane is the tiled kernels' (Form.tracked); it also decides legality for every form."""

    def __init__(self, form, profiling=True):
        self.form = form
        self.D = []          # the deferred batches: (reads, read length)
        self.F = 0
        self.G = self.X = False
        self.Z = True
        self.profiling = profiling
        self.enq = self.applies = 0
        self.submits = 0     # device or host submits since the reset that count in ntc_kernel_time once enqueued
        self.pin_enq = self.pin_applies = form.tracked
        self.log_est = 0.0
        self.in_flush = False
        self.set_cap = 0     # tiles x chunks every hand-over set holds; sets_sus: how many of them have a suspect list
        self.sets_sus = 0
        self.held = set()    # device batches the caller has promised to leave alone (DEFER_REDO: until sync / finish)
        self.submitted = set()
        self.direct = False  # some kernel may have incremented the sketch itself since the reset (K1f's slow path: the table-slot bytes)
        self.k1f_runs = 0
        self.export_expected = None
        self.unsure = False  # the tracker's G and Z are a guess since the last reset
        self.ever_off = not profiling  # some submit may have been enqueued while the engine was not profiling: enq then lags behind submits - D

    # -- classes of the coverage table --
    def klass(self):
        d, f = len(self.D), self.F
        return ("D0" if d == 0 else "D7" if d == 7 else "D1-6", "F0" if f == 0 else "F8" if f == 8 else "F1-7", "G" if self.G else "g", "Z" if self.Z else "z")

    # -- the engine's own steps --
    def _est(self, segs):
        e = 0.0
        for k in self.form.klist:
            act = [(n, L) for n, L in segs if L >= k]
            if act:
                e += sum(n * (L - k + 1) * 1.15 * 2.0 ** (1 - S_BITS) for n, L in act) + 64.0 * 4096
        return e

    def _book(self, est):
        if not self.form.has_log:
            return
        if self.G and self.log_est + est > 0.85 * self.form.log_cap():
            self._apply()
        self.log_est += est
        self.G = True

    def _join(self):
        if self.D and not self.in_flush:
            self.in_flush = True
            segs, self.D = self.D, []
            self._run_tiled(segs, len(segs), False)
            self.in_flush = False
        if self.F:
            self.k1f_runs += 1
        self.F = 0

    def _apply(self):
        self._join()
        if self.form.has_log and self.G:
            self.applies += 1
            self.G = False
            self.log_est = 0.0
            self.Z = False

    def _run_tiled(self, segs, n_submits, k1f_now):
        self._book(self._est(segs))
        defer = self.form.defer and not k1f_now
        counted = False
        need = max(-(-n // 2048) * -(-L // 16) for n, L in segs)
        for k in self.form.klist:
            na = sum(1 for n, L in segs if L >= k)
            if na == 0:
                continue
            if self.F + na > K1F_SETS:
                self._join()
            if self.profiling and not counted:
                self.enq += n_submits
                counted = True
            # the sets of these launches: a set that is too small, or the launch's first set without a suspect list, grows — behind the K1f of the launches ahead
            if self.F and self.D and not self.in_flush:
                # a set that has to grow does so behind the K1f of the launches ahead, which starts the waiting batches too — and how large a set must be
                # (suspects per wave) is nowhere in the header: from here to the next reset the counts are not pinned
                self.pin_enq = self.pin_applies = False
                self.unsure = True
            if need > self.set_cap or (self.F >= self.sets_sus):
                if self.F:
                    self._join()
                self.set_cap = max(self.set_cap, need)
                self.sets_sus = K1F_SETS if (na == 1 and defer) else max(self.sets_sus, 1)
            self.F += na
            if not defer:
                self._join()

    def _geometry(self, b):
        if b in EQUAL:
            return (EQUAL[b][0], EQUAL[b][1])
        return (n_reads(b), 16 * bin_chunks(b))

    # -- legality --
    def why_illegal(self, op):
        f, kind = self.form, op[0]
        if kind not in OPS:
            return "unknown operation"
        if kind in ("tiled", "slots", "host") and op[1] not in EQUAL:
            return "needs an equal-length batch"
        if kind == "ragged" and op[1] not in RAGGED_BINS:
            return "needs one bin of a ragged set"
        if kind == "bins" and not all(b in EQUAL or b in RAGGED_BINS for b in op[1]):
            return "needs equal-length batches or bins"
        if kind == "bins" and not 1 <= len(op[1]) <= 8:
            return "one launch takes up to 8 bins"
        if kind == "spans" and op[1] not in RAGGED:
            return "needs a ragged set"
        if kind == "long_device" and op[1] not in LONG:
            return "needs a long-sequence set"
        if kind in ("tiled", "ragged", "bins") and f.require_tiled and not f.ts_all:
            return "NTC_FLAG_REQUIRE_TILED refuses tiled batches of a configuration that is not all the tiled kernels'"
        if (kind == "ragged" or (kind == "bins" and any(b in RAGGED_BINS for b in op[1]))) and not f.ts_ok and not f.signature and not f.strand:
            return "a ragged tiled batch needs a k of the tiled kernels"
        if kind == "long_device" and f.require_tiled and not (f.ts_all and (len(f.klist) == 1 or max(f.klist) - min(f.klist) <= 15)):
            return "NTC_FLAG_REQUIRE_TILED refuses long sequences the tiled kernels do not serve"
        if kind in SUBMITS and any(b.startswith("slot") for b in op_batches(op)) and not (f.ts_all and kind in ("tiled", "bins", "host")):
            return "the general kernel K1 takes the bytes 1, 3, 4, 5, 7 for non-bases where the reference counts them (DESIGN.md, limits): such a batch only on the tiled kernels"
        if kind == "external_add" and not self.X:
            return "the caller may write to the counters only after ntc_device_state"
        if kind == "scribble":
            for b in op[1]:
                if b not in self.submitted:
                    return "scribble of a batch never submitted"
                if b in self.held:
                    return "NTC_FLAG_DEFER_REDO: the batch stays unchanged until ntc_sync / ntc_finish returns"
        if kind == "merge_devices":
            for s in op[1]:
                t = Tracker(f)
                for o in s:
                    if o[0] in ("merge_devices", "device_state", "external_add"):
                        return "a sibling's sequence only counts"
                    w = t.why_illegal(o)
                    if w:
                        return "sibling: " + w
                    t.step(o)
        return None

    def export_expect(self):
        """what ntc_log_export_device must answer: "ok", "state" (NTC_ERR_STATE: no log, or the sketch already holds counts) or "either" """
        if not self.form.has_log:
            return "state"
        if not self.form.tracked or self.unsure:
            return "either"
        if not self.Z:
            return "state"  # (an apply, a merge or the caller has written the sketch: refused whatever the kernels did, on the small-log form too)
        return "ok" if self.form.export_certain and not self.direct else "either"

    # -- one operation --
    def replaced(self, n_keys):
        """a successful export_replace has made exactly these keys the pending log"""
        self.log_est, self.G = float(n_keys), n_keys != 0

    def step(self, op, checked=False):
        """checked: the sequence is known to be legal (check_legal has walked it)"""
        why = None if checked else self.why_illegal(op)
        if why:
            raise Illegal("%r: %s" % (op, why))
        f, kind = self.form, op[0]
        if kind in SUBMITS:
            self.submits += 1
            for b in op_batches(op):
                self.submitted.add(b)
                if b.startswith("slot") or kind == "slots":  # (K1f's slow path; the general kernel, which an adaptive engine may switch to atomics)
                    self.direct = True
            if kind in ("tiled", "ragged", "bins", "slots") and f.defer:
                self.held.update(op_batches(op))
        if not f.tracked:
            self.export_expected = self.export_expect()
            if kind in ("sync", "finish"):
                self.held.clear()
            if kind == "device_state":
                self.X = True
            if kind == "profiling":
                self.profiling = bool(op[1])
            return
        if kind in ("tiled", "ragged"):
            if f.defer:
                self.D.append(self._geometry(op[1]))
                if len(self.D) >= DEFER_MAX:
                    self._join_deferred_only()
            else:
                self._run_tiled([self._geometry(op[1])], 1, False)
        elif kind == "bins":
            self._run_tiled([self._geometry(b) for b in op[1]], 1, False)
        elif kind == "host" or (kind == "spans" and f.require_tiled):
            # host reads are packed into tiles in staging the engine recycles: their K1f may not wait (k1f_now).  A ragged set: its bins of >= 1024 reads
            # (NTC_FLAG_REQUIRE_TILED lowers the bar to that) in one launch per k
            names = [op[1]] if kind == "host" else [bin_name(op[1], i) for i in reversed(range(len(RAGGED[op[1]][1])))]
            self._run_tiled([self._geometry(b) for b in names], 1, True)
        elif kind == "slots":
            n, L = self._geometry(op[1])
            self._book(64.0 * 4096 + n * sum(max(0, L - k + 1) * 1.15 * 2.0 ** (1 - S_BITS) for k in f.klist))
            if self.profiling:
                self.enq += 1
        elif kind in ("spans", "long_device"):
            # row slots with a slot table, the cut and its remainders: bookings and launches the header does not spell out
            self.pin_enq = self.pin_applies = False
            self._join()  # (recycled scratch: K1f at once — true of the cut; harmless to assume of the rows, F is not observable)
            self.G = f.has_log
        elif kind == "flush":
            self._apply()
        elif kind == "sync":
            self._join()
            self.held.clear()
        elif kind == "finish":
            self._apply()
            self.held.clear()
        elif kind == "reset":
            self._join()
            self.G, self.log_est, self.Z = False, 0.0, not self.X
            self.enq = self.applies = self.submits = 0
            self.pin_enq = self.pin_applies = True
            self.direct = self.unsure = False
        elif kind == "merge_counters":
            self.Z = False  # (adds into the counters; the waiting hash launches stay waiting: include/ntcard_hip.h, NTC_FLAG_DEFER_REDO)
        elif kind == "device_state":
            self._apply()
            self.X, self.Z = True, False
        elif kind == "external_add":
            pass
        elif kind == "export_replace":
            if f.has_log:
                self._join()  # (K1f's suspects are log entries too: the waiting launches come first, and may fill the log up); the log stays pending
            self.export_expected = self.export_expect()  # (behind the join: an apply it forced has written the sketch)
        elif kind == "merge_devices":
            self._apply()
            self.Z = False
        elif kind == "profiling":
            self.profiling = bool(op[1])
            self.ever_off |= not self.profiling
        elif kind in ("read_timers", "scribble"):
            pass

    def _join_deferred_only(self):
        """the eighth batch: the hash launch over all eight, K1f still waits"""
        self.in_flush = True
        segs, self.D = self.D, []
        self._run_tiled(segs, len(segs), False)
        self.in_flush = False


def check_legal(form, seq):
    """None, or why the sequence cannot run on the form"""
    t = Tracker(form)
    try:
        for op in seq:
            t.step(op)
    except Illegal as e:
        return str(e)
    return None


# ---- the directed sequences ----
T, S2 = "a2048", "clean2048"
FIN = ("finish",)


def _prefix(d, f, g, z):
    """operations that take a fresh all-tiled deferring engine into the class: d waiting batches, f launches awaiting K1f, log pending, sketch untouched"""
    pre = []
    if not z:
        pre += [("tiled", T), ("flush",)]
    if f:
        pre += [("bins", (T,) * f)]
    elif g:
        pre += [("tiled", T), ("sync",)]
    return pre + [("tiled", T)] * d


CLASSES = [(d, f, g, z) for z in (True, False) for g in (False, True) for f in (0, 2, 8) for d in (0, 3, 7) if g or not f]  # (a waiting K1h launch has booked the log)
COVER_OPS = {
    "tiled": [("tiled", "b2049")], "ragged": [("ragged", "rag:0")], "bins": [("bins", ("rag:1", "c4096"))], "slots": [("slots", "tiny2048")],
    "host": [("host", "b2049")], "spans": [("spans", "rag")], "long_device": [("long_device", "long")],
    "flush": [("flush",)], "sync": [("sync",)], "finish": [FIN], "reset": [("reset",), ("tiled", "b2049")],
    "merge_counters": [("merge_counters", ("b2049",))], "device_state": [("device_state",)],
    "external_add": [("external_add", (5, 30000), (65535, 7))], "export_replace": [("export_replace", 4)],
    "merge_devices": [("merge_devices", ((("tiled", "b2049"),),))], "profiling": [("profiling", False), ("tiled", "b2049"), ("profiling", True)],
    "read_timers": [("read_timers",)], "scribble": [("scribble", (S2,))],
}
COVER_FORM = "k32_tiled_defer"


def class_name(d, f, g, z):
    return ("D0" if d == 0 else "D7" if d == 7 else "D1-6", "F0" if f == 0 else "F8" if f == 8 else "F1-7", "G" if g else "g", "Z" if z else "z")


# cells of the (operation x class) table no legal sequence reaches, with the reason
UNREACHABLE = {("external_add", class_name(*c)): "ntc_device_state comes first, and from then on no reset leaves the sketch untouched (X excludes Z)"
               for c in CLASSES if c[3]}
READ_CAP = 100_000


def _cover_sequences():
    """for every operation, chains of cells [prefix of the class, the operation, finish, reset] of at most READ_CAP reads; -> {name: sequence}, and the cell
    every chain was built for: {name: [(index of the operation in the sequence, operation, class)]}"""
    form = FORM[COVER_FORM]
    seqs, cells = {}, {}
    for opname, body in COVER_OPS.items():
        chain, marks, count = [], [], 0

        def close():
            nonlocal chain, marks, count
            if chain:
                name = "cover_%s_%d" % (opname, count)
                seqs[name], cells[name] = tuple(chain), list(marks)
                chain, marks, count = [], [], count + 1

        for c in CLASSES:
            if (opname, class_name(*c)) in UNREACHABLE:
                continue
            head = []
            if opname == "scribble":
                head = [("tiled", S2), ("sync",), ("reset",)]  # a batch the engine has given back
            if opname == "external_add":
                head = [("device_state",)]
            cell = head + _prefix(*c) + body + [FIN, ("reset",)]
            at = len(head) + len(_prefix(*c))

            def fits(attempt, where):
                """the operation at `where` meets the class, the sequence is legal and within the cap"""
                if seq_reads(attempt) > READ_CAP:
                    return False
                t, met = Tracker(form), False
                try:
                    for i, op in enumerate(attempt):
                        if i == where:
                            met = t.klass() == class_name(*c)
                        t.step(op)
                except Illegal:
                    return False
                return met

            if not (chain and fits(chain + cell, len(chain) + at)):
                close()
                assert fits(cell, at), (opname, c)
            marks.append((len(chain) + at, opname, class_name(*c)))
            chain = chain + cell
        close()
    return seqs, cells


def _special_sequences():
    t = ("tiled", T)
    return {
        "ninth_batch": (t,) * 9 + (FIN,),
        "seventeen_batches": tuple(("tiled", b) for b in ("a2048", "b2049", "c4096", "tiny2048") * 4 + ("clean2048",)) + (FIN,),
        "nested_flush_host": (("bins", (T, T)), t, t, ("host", "b2049"), t, FIN),
        "nested_flush_bins": (("bins", (T, "rag:0")), t, t, t, ("bins", ("rag:1", "rag:2", "c4096")), ("flush",), t, FIN),
        "nested_flush_long": (("bins", (T, T, T)), t, t, ("long_device", "long"), t, FIN),
        "nested_flush_spans": (("bins", (T, T)), t, ("spans", "rag"), t, FIN),
        "sets_grow": (("bins", ("tiny2048", "clean2048")), ("tiled", "tiny2048"), ("tiled", "big6144"), ("tiled", "tiny2048"), FIN, ("bins", ("big6144", "d5000", "e6200")), FIN),
        "reset_with_deferred": (t, t, t, ("reset",), ("tiled", "b2049"), FIN, t, FIN),
        "exposed_reset": (("device_state",), ("external_add", (3, 77, 32767), (1, 65535, 9)), ("reset",), ("external_add", (3, 9000), (5, 65530)), t, FIN),
        # the same rule through the log exchange: once the counters are handed out, a reset does not make the export legal again
        "exposed_reset_export": (("device_state",), ("reset",), t, ("tiled", "b2049"), ("export_replace", 2), FIN, ("reset",), t, ("export_replace", 1), FIN),
        "merge_counters_ZG": (("merge_counters", ("b2049",)), t, FIN, ("reset",), t, ("sync",), ("merge_counters", ("b2049",)), FIN, ("merge_counters", ("c4096",)), FIN,
                              t, ("sync",), ("merge_counters", ("b2049",)), t, FIN),
        "export_with_deferred": (t, t, ("tiled", "b2049"), ("export_replace", 2), t, FIN),
        "export_with_suspects": (("tiled", "slot2048"), ("tiled", "d5000"), ("sync",), ("export_replace", 4), ("tiled", "slot2048"), ("export_replace", 1), FIN),
        "finish_twice": (t, ("tiled", "e6200"), FIN, FIN, t, FIN, FIN),
        "sync_scribble_all": (t, ("tiled", "b2049"), ("ragged", "rag:2"), ("slots", "tiny2048"), ("sync",), ("scribble", (T, "b2049", "rag:2", "tiny2048")),
                              ("tiled", "c4096"), t, ("host", "d5000"), FIN),
        "every_route": (t, ("ragged", "rag:0"), ("bins", ("rag:1", "b2049")), ("slots", "clean2048"), ("host", "c4096"), ("spans", "rag"), ("long_device", "long"),
                        ("read_timers",), FIN),
        "slow_path_and_clean": (("tiled", "slot2048"), ("tiled", "clean2048"), ("flush",), ("tiled", "slot2048"), ("host", "slot2048"), FIN),
        "merge_devices_mixed": (t, ("merge_devices", ((("tiled", "b2049"), ("tiled", "c4096")), (("bins", (T, T)), ("flush",), ("tiled", "tiny2048")))), t, FIN,
                                ("merge_devices", ((t,),)), FIN),
    }


def _nodefer_sequences():
    """Without NTC_FLAG_DEFER_REDO "the buffer may be reused as soon as the stream has passed the submit call": every device route, then a scribble of that very
    batch with nothing between them — no sync, no finish, no other call — then more batches.  Legal only on an engine created without the flag (with it
    the batches stay unchanged until ntc_sync, whatever the engine defers): of the forms, k32_tiled."""
    def sc(*names):
        return ("scribble", names)
    return {
        "nodefer_scribble_each_route": (("tiled", "a2048"), sc("a2048"), ("tiled", "b2049"), sc("b2049"), ("ragged", "rag:1"), sc("rag:1"),
                                        ("bins", ("c4096", "rag:0", "d5000")), sc("c4096", "rag:0", "d5000"), ("slots", "tiny2048"), sc("tiny2048"),
                                        ("long_device", "long"), sc("long"), ("tiled", "a2048"), sc("a2048"), ("tiled", "big6144"), sc("big6144"), ("tiled", "a2048"), FIN),
        "nodefer_scribble_slow_path": (("tiled", "slot2048"), sc("slot2048"), ("tiled", "d5000"), sc("d5000"), ("bins", ("slot2048", "a2048")), sc("slot2048", "a2048"),
                                       ("flush",), ("tiled", "e6200"), sc("e6200"), ("tiled", "clean2048"), FIN),
        "nodefer_scribble_same_batch": (("tiled", "d5000"), sc("d5000")) * 6 + (FIN, ("tiled", "b2049"), sc("b2049"), ("reset",), ("tiled", "b2049"), sc("b2049"), ("tiled", "a2048"), FIN),
    }


NODEFER_FORM = "k32_tiled"


# ---- the random sequences: seeds committed as data, drawn by the model's own legality rules ----
RANDOM_SEEDS = (101, 202, 303, 404, 505, 606, 707, 808)
_DRAW = [("tiled", 6), ("ragged", 2), ("bins", 2), ("slots", 1), ("host", 2), ("spans", 1), ("long_device", 1), ("flush", 2), ("sync", 2), ("finish", 2), ("reset", 1),
         ("merge_counters", 1), ("device_state", 1), ("external_add", 1), ("export_replace", 1), ("merge_devices", 1), ("profiling", 1), ("read_timers", 1),
         ("scribble", 2)]


def random_sequence(seed, form=None):
    form = form or FORM[COVER_FORM]
    rng = random.Random(seed)
    names = sorted(EQUAL)
    t, seq = Tracker(form), []
    want = rng.randint(12, 20)
    while len(seq) < want:
        kind = rng.choices([k for k, _ in _DRAW], [w for _, w in _DRAW])[0]
        if kind in ("tiled", "slots", "host"):
            op = (kind, rng.choice(names))
        elif kind == "ragged":
            op = (kind, rng.choice(RAGGED_BINS))
        elif kind == "bins":
            op = (kind, tuple(rng.choice(names + RAGGED_BINS) for _ in range(rng.randint(1, 4))))
        elif kind == "spans":
            op = (kind, "rag")
        elif kind == "long_device":
            op = (kind, "long")
        elif kind == "merge_counters":
            op = (kind, (rng.choice(names),))
        elif kind == "external_add":
            idx = tuple(sorted(rng.sample(range(2 << form.r_bits), 3)))
            op = (kind, idx, tuple(rng.choice((1, 9, 65535, 40000)) for _ in idx))
        elif kind == "export_replace":
            op = (kind, rng.choice((1, 2, 4)))
        elif kind == "merge_devices":
            op = (kind, ((("tiled", rng.choice(names)),) * rng.randint(1, 3),))
        elif kind == "profiling":
            op = (kind, rng.random() < 0.5)
        elif kind == "scribble":
            free = sorted(t.submitted - t.held)
            if not free:
                continue
            op = (kind, tuple(rng.sample(free, min(len(free), 2))))
        else:
            op = (kind,)
        if t.why_illegal(op) or seq_reads(seq + [op]) > READ_CAP:
            continue
        t.step(op)
        seq.append(op)
    return tuple(seq)


@functools.lru_cache(maxsize=None)
def sequences():
    """{name: sequence}: the directed ones (coverage chains, the specific ones) and the random ones"""
    out, _ = _cover_sequences()
    out = dict(out)
    out.update(_special_sequences())
    out.update(_nodefer_sequences())
    for s in RANDOM_SEEDS:
        out["random_%d" % s] = random_sequence(s)
    return out


PLACEMENTS = ("null", "stream", "stream_ext")  # the null stream, a caller stream, a caller stream with caller-owned sketch and F1


@functools.lru_cache(maxsize=None)
def cover_cells():
    return _cover_sequences()[1]
