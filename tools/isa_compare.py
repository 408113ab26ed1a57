#!/usr/bin/env python3
"""tools/isa_compare.py [--pairs FILE] OLD.s NEW.s — compare two AMDGPU assembly listings kernel by kernel.

The listings are what `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S file.hip` writes.  Per kernel symbol present in
both, the script prints whether the kernel-descriptor directives (.amdhsa_*: registers, scratch, LDS, ...) are equal, the instruction counts,
and the mnemonics whose counts differ.  Exit status 1 when a descriptor differs or a kernel exists in one listing only, 0 otherwise.

--pairs FILE: for kernels whose symbol changed (a struct became a template, say).  Each line of FILE is "old-symbol-substring new-symbol-substring"
('#' starts a comment); the one kernel of NEW.s whose symbol holds the second is compared with the one kernel of OLD.s whose symbol holds the first.  A
pair neither listing knows is skipped, so one file serves several listings."""
import collections
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def parse(path):
    """{symbol: (descriptor dict, Counter of mnemonics)} of the kernels of one listing"""
    desc, code = {}, {}
    sym = in_desc = None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if s.startswith(".amdhsa_kernel "):
            in_desc = s.split()[1]
            desc[in_desc] = {}
        elif s == ".end_amdhsa_kernel":
            in_desc = None
        elif in_desc is not None:
            if s.startswith(".amdhsa_"):
                key, _, val = s.partition(" ")
                desc[in_desc][key] = val.strip()
        elif s.startswith(".type") and "@function" in s:
            sym = s.split()[1].split(",")[0]
            code[sym] = collections.Counter()
        elif sym is not None:
            m = LABEL.match(s)
            if m:
                if m.group(1).startswith(".Lfunc_end"):
                    sym = None
            elif not s.startswith("."):
                code[sym][s.split()[0]] += 1
    return {k: (desc[k], code.get(k, collections.Counter())) for k in desc}


def pair_up(path, old, new):
    """Renames the kernels of `new` that the pairs of the file at `path` name to their symbols in `old`; -> {old symbol: new symbol} of those"""
    renamed = {}
    for line in open(path):
        words = line.split("#", 1)[0].split()
        if not words:
            continue
        o, n = words
        olds, news = [s for s in old if o in s], [s for s in new if n in s]
        if not olds and not news:
            continue
        if len(olds) != 1 or len(news) != 1:
            sys.exit(f"pair {o} {n}: {len(olds)} kernels of OLD and {len(news)} of NEW match, not one each")
        renamed[olds[0]] = news[0]
        new[olds[0]] = new.pop(news[0])
    return renamed


def main(argv):
    pairs = None
    if len(argv) > 1 and argv[1] == "--pairs":
        pairs, argv = argv[2], argv[:1] + argv[3:]
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = parse(argv[1]), parse(argv[2])
    renamed = pair_up(pairs, old, new) if pairs else {}
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            print(f"{sym}\n  only in {'NEW' if sym in new else 'OLD'}")
            bad += 1
            continue
        (d0, c0), (d1, c1) = old[sym], new[sym]
        diff = {k: (d0.get(k), d1.get(k)) for k in sorted(set(d0) | set(d1)) if d0.get(k) != d1.get(k)}
        bad += bool(diff)
        n0, n1 = sum(c0.values()), sum(c1.values())
        print(sym + (f"\n  in NEW: {renamed[sym]}" if sym in renamed else ""))
        print(f"  descriptor: {'equal' if not diff else 'DIFFERENT'}   instructions: {n0} -> {n1} ({n1 - n0:+d})")
        for k, (a, b) in diff.items():
            print(f"    {k}: {a} -> {b}")
        moved = [f"{m} {c1[m] - c0[m]:+d}" for m in sorted(set(c0) | set(c1)) if c0[m] != c1[m]]
        if moved:
            print("    " + ", ".join(moved))
    print(f"{len(set(old) | set(new))} kernels, {bad} with a different descriptor or missing on one side")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
