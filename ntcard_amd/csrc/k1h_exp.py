"""k1h_exp.py — the timing-experiment switches of the K1h generator (K1H_EXP=a,b,...; tools/k1h_variant.sh, bench.py --k1h-timers) and the
post-pass that four of them are: it works on a finished, scheduled Prog, not on generator state.  The production kernel is built with none."""
import os

RIGHT, WRONG = "results stay right", "results WRONG"
# the only place the switches are spelt: name -> (what it does, what becomes of the results)
SWITCHES = {
    "timers": ("section clocks (walk + test + push, pack, resolve passes, end of block) added to f1[1 .. 4]; F1 and the suspects are not kept", WRONG),
    "noload": ("no buffer loads of the raw bytes", WRONG),
    "nopass": ("a resolve pass only empties the queue", WRONG),
    "nopack": ("a pack batch is skipped behind its wait", WRONG),
    "nomul": ("a shift in place of the pack's multiply-gather", WRONG),
    "nocarry": ("a v_or in place of the dirty bits' carry chain", WRONG),
    "noflags": ("no sample test, no push", WRONG),
    "noprio": ("the resolve pass does not raise its priority", RIGHT),
    "nosched": ("the list scheduler is left out", RIGHT),
    "nopslow": ("a scalar no-op behind every slow-class VALU instruction", RIGHT),
    "noprun": ("a scalar no-op behind every run of slow-class VALU instructions", RIGHT),
    "priorun": ("priority 3 around every run of slow-class VALU instructions (add noprio)", RIGHT),
    "priowalk": ("priority 3 around every run of 12 or more fast VALU instructions (add noprio)", RIGHT),
}


def parse_exp(text=None):
    """K1H_EXP (or text) -> the set of switches; a name that is none is an error: it would silently build the production kernel"""
    text = os.environ.get("K1H_EXP", "") if text is None else text
    exp = set(x for x in text.split(",") if x)
    unknown = sorted(exp - set(SWITCHES))
    if unknown:
        raise ValueError(f"K1H_EXP: unknown switch {', '.join(unknown)}; the switches are {', '.join(SWITCHES)}")
    return exp


def readme_sentence():
    """what tools/README.md says about the switches (tests/test_k1h_emulator.py holds the two together)"""
    wrong = ", ".join(f"`{n}`" for n, (_, r) in SWITCHES.items() if r == WRONG)
    right = ", ".join(f"`{n}`" for n, (_, r) in SWITCHES.items() if r == RIGHT)
    return f"`K1H_EXP` switches {wrong} — results are WRONG, only the clock is of interest; {right} keep the results"


# VALU instructions that a second wave on the SIMD overlaps with completely (profiles/r05_ubench_op_classes.txt): every other VALU
# instruction — and any of these with an SGPR source — occupies the pipe for a whole issue interval
FAST_VALU = {"v_bitop3_b32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_lshrrev_b32", "v_ashrrev_i32",
             "v_mov_b32"}


def is_slow_valu(mnem, ops):
    if not mnem.startswith("v_"):
        return False
    if mnem not in FAST_VALU:
        return True
    return any(o.startswith("s") or o.startswith("vcc") or o.startswith("exec") for o in ops[1:])


def phase_fix(p, exp):
    """K1H_EXP=nopslow | noprun | priorun | priowalk (results stay RIGHT; with priorun / priowalk add noprio, which takes the pass's own s_setprio out): scalar no-ops / priority changes next to the slow-class VALU
    instructions.  profiles/r05_ubench_sparse_slow.txt, r05_ubench_phase_fix.txt: one slow-class instruction drops a pair of waves into a
    persistent phase in which they do not overlap any more, and a scalar instruction next to it brings the overlap back."""
    if "priowalk" in exp:
        out, code = [], p.code
        i, n = 0, len(code)
        while i < n:
            c = code[i]
            if c[0] == "i" and c[1].startswith("v_") and not is_slow_valu(c[1], c[2]):
                j = i
                while j < n and code[j][0] == "i" and code[j][1].startswith("v_") and not is_slow_valu(code[j][1], code[j][2]):
                    j += 1
                if j - i >= 12:
                    out.append(("i", "s_setprio", ["3"], ""))
                    out.extend(code[i:j])
                    out.append(("i", "s_setprio", ["0"], ""))
                else:
                    out.extend(code[i:j])
                i = j
                continue
            out.append(c)
            i += 1
        p.code = out
        return
    mode = [m for m in ("nopslow", "noprun", "priorun") if m in exp]
    if not mode:
        return
    mode = mode[0]
    out = []
    pending = False   # a slow-class VALU instruction has been issued and neither a scalar instruction nor a fix since
    for c in p.code:
        if c[0] != "i":
            out.append(c)
            if c[0] == "l":
                pending = False if mode != "priorun" else pending
            continue
        mnem, ops = c[1], c[2]
        if mnem.startswith("v_"):
            slow = is_slow_valu(mnem, ops)
            if slow:
                if mode == "priorun" and not pending:
                    out.append(("i", "s_setprio", ["3"], ""))
                out.append(c)
                if mode == "nopslow":
                    out.append(("i", "s_nop", ["0"], ""))
                else:
                    pending = True
                continue
            if pending:
                out.append(("i", "s_nop", ["0"], "") if mode == "noprun" else ("i", "s_setprio", ["0"], ""))
                pending = False
            out.append(c)
            continue
        if mnem.startswith("s_") and mode != "priorun":
            pending = False   # a scalar instruction does what the no-op would
        if mode == "priorun" and pending and (mnem.startswith("s_cbranch") or mnem in ("s_branch", "s_setpc_b64", "s_endpgm")):
            out.append(("i", "s_setprio", ["0"], ""))
            pending = False
        out.append(c)
    p.code = out
