#!/usr/bin/env python3
"""Per-kernel differences between two `hipcc --cuda-device-only -S` files of the same source unit: does
a refactor of the arithmetic headers change the machine code that matters?

Per kernel (matched by mangled name) it compares
  * the opcode histogram of the arithmetic VALU instructions: every v_* except v_mov_*, v_accvgpr_*
    and v_nop (register-allocation noise);
  * Occupancy (must be equal), ScratchSize and LDS size (must not grow), next_free_vgpr (must not
    grow where the occupancy is below 8);
  * with --loops SUB[,SUB...]: for each kernel whose name contains SUB, the valu= / mad= columns of
    loop_mix.py for the blocks inside loops, in order (a difference is listed with the block's
    arithmetic VALU count beside it: valu= counts the moves too).
Prints one line per kernel that differs (FAIL: a condition above is broken; note: an allowed change) and a
summary; exit status 1 if any kernel fails.
usage: isa_compare.py <base.s> <new.s> [--loops SUB,SUB,...] [--all]"""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_mix

NOISE = ("v_mov_", "v_accvgpr_", "v_nop")
META = {"vgpr": r"\.amdhsa_next_free_vgpr\s+(\d+)", "lds": r"\.amdhsa_group_segment_fixed_size\s+(\d+)",
        "scratch": r"; ScratchSize:\s+(\d+)", "occupancy": r"; Occupancy:\s+(\d+)"}


def kernels_of(path):
    """{kernel name: {"ops": Counter, "snop": int, "vgpr", "lds", "scratch", "occupancy"}}"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, body = collections.OrderedDict(), None, False
    for l in lines:
        m = re.match(r"^(\w+):\s*; @", l)
        if m and m.group(1) in names:
            cur, body = m.group(1), True
            out[cur] = {"ops": collections.Counter(), "snop": 0}
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            body = False
            continue
        t = l.strip()
        if body and t and not t.startswith((".", ";")) and not t.endswith(":"):
            op = t.split()[0]
            if op == "s_nop":
                out[cur]["snop"] += 1
            if op.startswith("v_") and not op.startswith(NOISE):
                out[cur]["ops"][op] += 1
        else:
            for k, pat in META.items():
                m = re.search(pat, l)
                if m and k not in out[cur]:
                    out[cur][k] = int(m.group(1))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(s):
    s = re.sub(r"\(anonymous namespace\)::|zkp::", "", s)
    return s.split("(")[0]


def loop_rows(path, name):
    """(valu, mad, arithmetic valu) of every block inside a loop, in order"""
    rows = []
    for b in loop_mix.blocks_of(path, name).values():
        if b["loop"] is not None:
            v = [(o, c) for o, c in b["ops"].items() if o.startswith("v_")]
            rows.append((sum(c for _, c in v), b["ops"].get("v_mad_u64_u32", 0), sum(c for o, c in v if not o.startswith(NOISE))))
    return rows


def main():
    base_p, new_p = sys.argv[1], sys.argv[2]
    loops = sys.argv[sys.argv.index("--loops") + 1].split(",") if "--loops" in sys.argv else []
    base, new = kernels_of(base_p), kernels_of(new_p)
    dm = demangle(sorted(set(base) | set(new)))
    fails = same_hist = 0
    for k in sorted(set(base) | set(new), key=lambda n: dm[n]):
        if k not in base or k not in new:
            print("FAIL %s: only in %s" % (short(dm[k]), "base" if k in base else "new"))
            fails += 1
            continue
        b, n = base[k], new[k]
        bad, note = [], []
        if b["ops"] != n["ops"]:
            d = {o: (b["ops"].get(o, 0), n["ops"].get(o, 0)) for o in set(b["ops"]) | set(n["ops"])
                 if b["ops"].get(o, 0) != n["ops"].get(o, 0)}
            bad.append("valu histogram " + ", ".join("%s %d->%d" % (o, x, y) for o, (x, y) in sorted(d.items())))
        else:
            same_hist += 1
        if b["occupancy"] != n["occupancy"]:
            bad.append("occupancy %d->%d" % (b["occupancy"], n["occupancy"]))
        for key in ("scratch", "lds"):
            if n[key] != b[key]:
                (bad if n[key] > b[key] else note).append("%s %d->%d" % (key, b[key], n[key]))
        if n["vgpr"] != b["vgpr"]:
            (bad if n["vgpr"] > b["vgpr"] and b["occupancy"] < 8 else note).append("vgpr %d->%d" % (b["vgpr"], n["vgpr"]))
        if n["snop"] != b["snop"]:
            note.append("s_nop %d->%d" % (b["snop"], n["snop"]))
        for sub in loops:
            if sub in k or sub in dm[k]:
                rb, rn = loop_rows(base_p, k), loop_rows(new_p, k)
                if rb == rn:
                    note.append("%d loop blocks equal in valu/mad" % len(rb))
                elif len(rb) != len(rn):
                    bad.append("loop blocks: %d -> %d" % (len(rb), len(rn)))
                else:
                    d = ["block %d valu %d->%d mad %d->%d arithmetic valu %d->%d" % (i, x[0], y[0], x[1], y[1], x[2], y[2])
                         for i, (x, y) in enumerate(zip(rb, rn)) if x != y]
                    bad.append("loop blocks (of %d): %s" % (len(rb), ", ".join(d)))
        if bad:
            fails += 1
        if bad or note or "--all" in sys.argv:
            print("%s %s [occ %d, vgpr %d, mad %d]: %s" % ("FAIL" if bad else "note", short(dm[k]), n["occupancy"], n["vgpr"],
                                                          n["ops"].get("v_mad_u64_u32", 0), "; ".join(bad + note) or "equal"))
    print("%s vs %s: %d kernels, %d with equal arithmetic-VALU histograms, %d FAIL" % (
        base_p, new_p, len(set(base) | set(new)), same_hist, fails))
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
