#!/usr/bin/env python3
"""`wtns check` on one MI355X at the Venmo shape (zkp_checker_*), timed through the C ABI.

Part 1, the synthetic Venmo circuit (synth.Circuit.venmo: 6.4 M signals, the bench's constraint count; its
rows have at most 3 terms, so every constraint takes the short kernel): one load, WARM checks thrown away, then
REPS checks from host memory and REPS staged checks against a resident prover, alternated with REPS staged
proofs of the same slot.  Two ratios from that one run: the check's kernels over the prover's buildABC stage
(both HIP-event times; buildABC does two of the three dot products on the same matrix shape), and the staged
check's wall time over the staged proof's.

Part 2, long rows (--long): a circuit built here with the same number of constraints' worth of terms, 1 % of
them moved into rows of 254 and of 4096 terms (half each, spread evenly among 4-term constraints), checked
with the library's switch and with every constraint forced through the short kernel (ZKP_WTNS_CHECK_LONG=0
at load), alternated.  --sweep: the same at 2^20 constraints with the long rows all of one length L, for
several L, with the switch at L and with none: the measurement the switch's default rests on.  These
circuits take any coefficients and the witness (1, 0, 0, ...), which satisfies them; the kernels' time does
not depend on the values (no data-dependent branch), only on the shape.

Bytes per term: 32 (coefficient) + 4 (wire) + 32 (the witness value gathered) = 68, plus 12 per constraint
of row pointers.  One JSON document (--out, default profiles/wtns_check.json).
usage: bench_wtns_check.py [--reps 20] [--warm 3] [--long] [--sweep] [--no-prover] [--out FILE]"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))
import zkp_amd  # noqa: E402
from zkp_amd import synth  # noqa: E402

SEED, SETUP_SEED, WSEED = 0x5A4B5032, 0x5A4B5033, 0x5A4B5034
R_LE = (21888242871839275222246405745257275088548364400416034343698204186575808495617).to_bytes(32, "little")
TERM = np.dtype([("wire", "<u4"), ("coef", "u1", 32)])


def stats(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def binfile(magic, version, sections):
    out = [magic, struct.pack("<II", version, len(sections))]
    for sid, payload in sections:
        out += [struct.pack("<IQ", sid, len(payload)), payload]
    return b"".join(out)


def rows(rng, n_rows, shape, n_wires):
    """n_rows constraints with shape = (terms in A, in B, in C) as section-2 bytes: random wires in
    1 .. n_wires - 1 (never wire 0: the witness (1, 0, ...) then satisfies everything), coefficients below 2^253"""
    fields = []
    for m, k in enumerate(shape):
        fields += [("n%d" % m, "<u4"), ("t%d" % m, TERM, (k,))]
    a = np.zeros(n_rows, dtype=np.dtype(fields))
    for m, k in enumerate(shape):
        a["n%d" % m] = k
        a["t%d" % m]["wire"] = rng.integers(1, n_wires, size=(n_rows, k), dtype=np.uint32)
        c = rng.integers(0, 256, size=(n_rows, k, 32), dtype=np.uint8)
        c[:, :, 31] &= 0x1F
        a["t%d" % m]["coef"] = c
    return a


def long_row_circuit(n_short, long_rows, n_wires, seed):
    """(r1cs bytes, terms): n_short constraints of 2 + 1 + 1 terms with the long rows (a list of lengths, each a
    constraint of L + 1 + 1 terms with the long row in A) spread evenly among them"""
    rng = np.random.default_rng(seed)
    short = rows(rng, n_short, (2, 1, 1), n_wires)
    parts, at = [], 0
    for k, length in enumerate(long_rows):
        upto = n_short * (k + 1) // (len(long_rows) + 1)
        parts += [short[at:upto].tobytes(), rows(rng, 1, (length, 1, 1), n_wires).tobytes()]
        at = upto
    parts.append(short[at:].tobytes())
    n = n_short + len(long_rows)
    sec1 = struct.pack("<I", 32) + R_LE + struct.pack("<IIIIQI", n_wires, 0, 2, n_wires - 3, n_wires, n)
    return binfile(b"r1cs", 1, [(1, sec1), (2, b"".join(parts))]), 4 * n_short + sum(x + 2 for x in long_rows)


def unit_witness(n_wires):
    sec1 = struct.pack("<I", 32) + R_LE + struct.pack("<I", n_wires)
    body = bytearray(32 * n_wires)
    body[0] = 1
    return binfile(b"wtns", 2, [(1, sec1), (2, bytes(body))])


def time_checks(chk, wt, reps, warm):
    for _ in range(warm):
        assert chk.check(wt).valid
    t = {"witness_copy": [], "kernels": [], "total": []}
    for _ in range(reps):
        assert chk.check(wt).valid
        x = zkp_amd.wtns_check_timings()
        for k in t:
            t[k].append(x[k])
    return {k: stats(v) for k, v in t.items()}


def load(r1cs, long_terms=None):
    if long_terms is None:
        os.environ.pop("ZKP_WTNS_CHECK_LONG", None)
    else:
        os.environ["ZKP_WTNS_CHECK_LONG"] = str(long_terms)
    chk = zkp_amd.WitnessChecker(r1cs)
    os.environ.pop("ZKP_WTNS_CHECK_LONG", None)
    return chk, zkp_amd.wtns_check_timings()


def compare_switch(r1cs, wt, switches, reps, warm):
    """kernel ms of the same circuit under each switch, the checkers resident together and alternated"""
    chks = [load(r1cs, s)[0] for s in switches]
    for c in chks:
        for _ in range(warm):
            assert c.check(wt).valid
    ms = [[] for _ in chks]
    for _ in range(reps):
        for k, c in enumerate(chks):
            assert c.check(wt).valid
            ms[k].append(zkp_amd.wtns_check_timings()["kernels"])
    out = [{"switch": s, "n_long": c.info()["n_long"], "kernels_ms": stats(m)} for s, c, m in zip(switches, chks, ms)]
    for c in chks:
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--long", action="store_true", help="part 2: 1 %% of the terms in rows of 254 and 4096")
    ap.add_argument("--sweep", action="store_true", help="the switch's measurement: long rows of one length L, several L")
    ap.add_argument("--no-prover", action="store_true", help="skip the resident prover (staged checks, both ratios)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wtns_check.json"))
    args = ap.parse_args()
    res = {"op": "wtns check", "reps": args.reps, "warm": args.warm, "bytes_per_term": 68, "bytes_per_constraint": 12}

    c = synth.Circuit.venmo(SEED)
    r1cs = c.r1cs()
    wt = c.witness(WSEED)
    chk, t_load = load(r1cs)
    info = chk.info()
    terms, n = info["n_terms"], info["n_constraints"]
    res["venmo"] = {"shape": info, "load_ms": {k: round(t_load[k], 2) for k in ("parse_csr", "upload_convert", "total")},
                    "share_long": round(info["n_long"] / n, 6), "share_short": round(1 - info["n_long"] / n, 6),
                    "check_from_host_ms": time_checks(chk, wt, args.reps, args.warm)}
    k_ms = res["venmo"]["check_from_host_ms"]["kernels"]["median"]
    res["venmo"]["kernels_GBps"] = round((68 * terms + 12 * n) / (k_ms * 1e-3) / 1e9, 1)
    res["venmo"]["ns_per_term"] = round(k_ms * 1e6 / terms, 3)
    print("# venmo: %d terms, kernels %.3f ms" % (terms, k_ms), file=sys.stderr, flush=True)

    if not args.no_prover:
        print("# building the known-tau key and loading the prover", file=sys.stderr, flush=True)
        p = zkp_amd.Prover(c.zkey(SETUP_SEED, device=0, threads=16), devices=[0])
        p.stage(wt, slot=0)
        for _ in range(args.warm):
            p.prove_staged_raw(0, 5, 7)
            assert chk.check_staged(p, 0).valid
        abc, proof_wall, ck, ck_wall = [], [], [], []
        for _ in range(args.reps):  # alternated: the two sides see the same machine
            t0 = time.perf_counter()
            p.prove_staged_raw(0, 5, 7)
            proof_wall.append((time.perf_counter() - t0) * 1e3)
            abc.append(p.timings()["build_abc"])
            t0 = time.perf_counter()
            assert chk.check_staged(p, 0).valid
            ck_wall.append((time.perf_counter() - t0) * 1e3)
            ck.append(zkp_amd.wtns_check_timings()["kernels"])
        res["staged"] = {"check_kernels_ms": stats(ck), "check_wall_ms": stats(ck_wall), "prover_build_abc_ms": stats(abc),
                         "proof_wall_ms": stats(proof_wall),
                         "check_kernels_over_build_abc": round(statistics.median(ck) / statistics.median(abc), 3),
                         "staged_check_over_staged_proof": round(statistics.median(ck_wall) / statistics.median(proof_wall), 4)}
        p.close()
    chk.close()
    del r1cs, wt, c

    if args.long:
        moved = terms // 100
        long_rows = [254] * (moved // 2 // 256) + [4096] * (moved // 2 // 4098)
        n_short = (terms - sum(x + 2 for x in long_rows)) // 4
        n_wires = synth.VENMO["n_vars"]
        lr, lterms = long_row_circuit(n_short, long_rows, n_wires, 1)
        got = compare_switch(lr, unit_witness(n_wires), [None, 0], args.reps, args.warm)
        res["long_rows"] = {"terms": lterms, "constraints": n_short + len(long_rows), "rows_of_254": long_rows.count(254),
                            "rows_of_4096": long_rows.count(4096), "default_switch": got[0], "forced_short": got[1],
                            "forced_short_over_default": round(got[1]["kernels_ms"]["median"] / got[0]["kernels_ms"]["median"], 3)}
        del lr
    if args.sweep:
        n_short, n_wires = 1 << 20, 1 << 20
        res["sweep"] = []
        for length in (8, 12, 16, 24, 32, 48, 64, 96, 128, 254):
            count = max(1, (4 * n_short // 100) // length)
            lr, lterms = long_row_circuit(n_short, [length] * count, n_wires, length)
            got = compare_switch(lr, unit_witness(n_wires), [length, 0], max(5, args.reps // 2), args.warm)
            res["sweep"].append({"L": length, "rows": count, "terms": lterms, "long_ms": got[0]["kernels_ms"],
                                 "short_ms": got[1]["kernels_ms"],
                                 "short_over_long": round(got[1]["kernels_ms"]["median"] / got[0]["kernels_ms"]["median"], 3)})
            print("# sweep L=%d: %s" % (length, res["sweep"][-1]["short_over_long"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
