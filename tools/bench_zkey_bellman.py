#!/usr/bin/env python3
"""The third-party path of phase 2 on one MI355X, timed through the C ABI at the Venmo shape: on the key after one
contribution, `zkp_zkey_export_bellman` -> `zkp_zkey_bellman_contribute` -> `zkp_zkey_import_bellman`, the median of
--runs runs of each with its device split (zkp_zkey_bellman_timings), and beside them, in the same process and on
the same key, `zkp_zkey_contribute_entropy`: the yardstick the import is compared with (the coordinator's
alternative to an outside contribution is a contribution of its own).  The imported key must pass `zkey verify`
against the initial key, equal the yardstick's key in every section but 9 and export to the response file.

The inputs (a synthetic circuit of the Venmo shape, a known-tau ptau of power 24, `zkey new`) are tooling and are
not timed.  The measurement runs in a child process under a time limit.  --shape small runs a 2^17-domain circuit
where the Venmo shape does not fit (17 GB of ptau in host memory).

usage: bench_zkey_bellman.py [--shape venmo|small] [--runs 3] [--out profiles/zkey_bellman.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))

RAND64 = bytes(range(7, 71))
RAND64_B = bytes(range(9, 73))
COEFF_SEED = bytes(range(100, 132))
SEED = 0x5A4B5032
SHAPES = {"venmo": None, "small": (100000, 120000, 26, 18)}  # n_vars, n_constraints, n_public, ptau power
LIMIT_S = {"venmo": 1100, "small": 300}


def mem_available_gb():
    for ln in open("/proc/meminfo"):
        if ln.startswith("MemAvailable:"):
            return int(ln.split()[1]) / 1e6
    return 0.0


def sections(buf):
    """{id: (offset, length)} of a binfile"""
    n = int.from_bytes(buf[8:12], "little")
    o, out = 12, {}
    for _ in range(n):
        sid, ln = int.from_bytes(buf[o:o + 4], "little"), int.from_bytes(buf[o + 4:o + 12], "little")
        out[sid] = (o + 12, ln)
        o += 12 + ln
    return out


def child(shape, runs):
    import zkp_amd
    from zkp_amd import synth
    if SHAPES[shape] is None:
        c, power = synth.Circuit.venmo(SEED), 24
    else:
        nv, nc, npub, power = SHAPES[shape]
        c = synth.Circuit(nv, nc, npub, SEED)
    res = {"op": "zkey export bellman -> bellman contribute -> import bellman; zkey contribute beside", "shape": shape,
           "circuit": {"n_vars": c.n_vars, "n_constraints": c.n_constraints, "n_public": c.n_public, "domain": c.domain_size},
           "runs": runs, "note": "medians; device figures are HIP-event ms summed over chunks, the rest host wall"}
    t0 = time.time()
    k0 = zkp_amd.zkey_new(c.r1cs(), synth.ptau(power, SEED))
    k1 = zkp_amd.zkey_contribute_entropy(k0, "first", rand64=RAND64, name="first")
    res["inputs_s"] = round(time.time() - t0, 2)
    print("inputs: %.1f s" % res["inputs_s"], file=sys.stderr, flush=True)
    res["zkey_bytes"] = len(k1)
    # warm-up: the code objects and the first pinned allocation of every path, on a small key
    w = synth.Circuit(300, 400, 3, 5)
    wk = zkp_amd.zkey_new(w.r1cs(), synth.ptau(10, 5))
    zkp_amd.zkey_import_bellman(wk, zkp_amd.zkey_bellman_contribute(zkp_amd.zkey_export_bellman(wk), "w", rand64=RAND64))

    def timed(call):
        walls, splits, out = [], [], None
        for _ in range(runs):
            out = None
            t0 = time.time()
            out = call()
            walls.append(time.time() - t0)
            splits.append(zkp_amd.zkey_bellman_timings())
        med = {k: round(statistics.median(s[k] for s in splits), 2) for k in splits[0]}
        print("  %.3f s" % statistics.median(walls), file=sys.stderr, flush=True)
        return out, {"wall_s": round(statistics.median(walls), 3), "wall_s_runs": [round(x, 3) for x in walls], "timings_ms": med}

    challenge, res["export_bellman"] = timed(lambda: zkp_amd.zkey_export_bellman(k1))
    res["export_bellman"]["bytes"] = len(challenge)
    response, res["bellman_contribute"] = timed(
        lambda: zkp_amd.zkey_bellman_contribute(challenge, "bench contribution", rand64=RAND64_B))
    del challenge
    new, res["import_bellman"] = timed(lambda: zkp_amd.zkey_import_bellman(k1, response, name="second"))
    for key in ("export_bellman", "import_bellman"):
        t = res[key]["timings_ms"]
        res[key]["coset_scaling_over_transform"] = round(t["coset_scale"] / t["transform"], 3) if t["transform"] else None
        res[key]["coset_scaling_share_of_total"] = round(t["coset_scale"] / t["total"], 3) if t["total"] else None
    walls, yard = [], None
    for _ in range(runs):
        yard = None
        t0 = time.time()
        yard = zkp_amd.zkey_contribute_entropy(k1, "bench contribution", rand64=RAND64_B, name="second")
        walls.append(time.time() - t0)
    res["zkey_contribute_yardstick"] = {"wall_s": round(statistics.median(walls), 3), "wall_s_runs": [round(x, 3) for x in walls]}
    res["import_wall_over_contribute_wall"] = round(res["import_bellman"]["wall_s"] / res["zkey_contribute_yardstick"]["wall_s"], 3)
    sa, sb = sections(new), sections(yard)
    res["import_equals_contribute_except_section_9"] = len(new) == len(yard) and all(
        new[sa[i][0]:sa[i][0] + sa[i][1]] == yard[sb[i][0]:sb[i][0] + sb[i][1]] for i in sb if i != 9)
    del yard
    res["export_of_the_imported_key_is_the_response"] = zkp_amd.zkey_export_bellman(new) == response
    del response
    t0 = time.time()
    ok, msg = zkp_amd.zkey_verify_frominit(k0, new, seed=COEFF_SEED)
    res["verify"] = {"wall_s": round(time.time() - t0, 3), "verdict": msg}
    print(json.dumps(res), flush=True)
    good = ok and res["import_equals_contribute_except_section_9"] and res["export_of_the_imported_key_is_the_response"]
    return 0 if good else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="venmo", choices=sorted(SHAPES))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args.shape, args.runs))
    need_gb = 45 if args.shape == "venmo" else 4
    if mem_available_gb() < need_gb:
        print("host memory: %.0f GB available, %.0f GB wanted for --shape %s" % (mem_available_gb(), need_gb, args.shape),
              file=sys.stderr)
        sys.exit(2)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", args.shape, "--runs", str(args.runs)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT_S[args.shape])  # stderr: progress
    except subprocess.TimeoutExpired:
        print("time limit of %d s" % LIMIT_S[args.shape], file=sys.stderr)
        sys.exit(1)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if lines:
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(json.loads(lines[-1]), f, indent=1)
                f.write("\n")
    sys.exit(r.returncode if lines else 1)


if __name__ == "__main__":
    main()
