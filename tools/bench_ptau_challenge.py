#!/usr/bin/env python3
"""The third-party path of phase 1 on one MI355X, timed through the C ABI: per power, on a file with one
contribution, `zkp_ptau_export_challenge` -> `zkp_ptau_challenge_contribute` -> `zkp_ptau_import_response` ->
`zkp_ptau_verify` (reference circuit/scripts/generate_keys_phase1.sh:12-14,16), and beside them, in the same run
and on the same file, `zkp_ptau_contribute`: the yardstick, the one in-project call that does the same hashing
and strictly more device work than the import.  The verdict must be "OK" and the imported file must equal the
yardstick's byte for byte.

Every power runs in a child process of its own under a time limit; the first failure ends the run.  Power 24
runs only if the host has memory for it (the file is 6.4 GB; the child holds the old file, the challenge, the
response and two results).

Per power, one JSON line (collected into --out as a list):
* the wall time and the timing vector of each call (zkp_ptau_challenge_timings, zkp_ptau_contribute_timings,
  zkp_ptau_verify_timings), and which of its host hashes is the longer one;
* ns per G1 and per G2 point of k_decompress_points (device time of the import), and the kernel's field
  products per second as a fraction of the measured v_mad_u64_u32 peak of profiles/ubench_r05.json: per G1
  point 363 Fq products (x^3 + b: 2, the root a^((p + 1) / 4) by square-and-multiply and its check: 361), per
  G2 point 733 (x^3 + b: an Fq2 square of 2 and an Fq2 product counted as 3; the norm-method root and its
  check: 728), 136 multiply-accumulates per product, as DESIGN §8f - §8h count them.
usage: bench_ptau_challenge.py [--powers 16,20,24] [--out profiles/ptau_challenge.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))

RAND64 = bytes(range(7, 71))
RAND64_B = bytes(range(9, 73))
COEFF_SEED = bytes(range(100, 132))
G1_PRODUCTS, G2_PRODUCTS, MADS_PER_PRODUCT = 363, 733, 136
LIMIT_S = {16: 240, 20: 420, 24: 1100}


def mem_available_gb():
    for ln in open("/proc/meminfo"):
        if ln.startswith("MemAvailable:"):
            return int(ln.split()[1]) / 1e6
    return 0.0


def child(power):
    import zkp_amd
    N = 1 << power
    g1_points, g2_points = 4 * N - 1, N + 1
    peak = json.load(open(os.path.join(ROOT, "profiles", "ubench_r05.json")))["v_mad_u64_u32_tops"] * 1e12
    res = {"op": "powersoftau export challenge -> challenge contribute -> import response -> verify; contribute beside",
           "power": power, "points": {"g1": g1_points, "g2": g2_points}, "runs": 1}
    # warm-up: the device, the code objects and the first pinned allocation of every path
    warm = zkp_amd.ptau_contribute(zkp_amd.ptau_new(4), "warm", rand64=RAND64)
    zkp_amd.ptau_import_response(warm, zkp_amd.ptau_challenge_contribute(zkp_amd.ptau_export_challenge(warm), "w", rand64=RAND64))
    old = zkp_amd.ptau_contribute(zkp_amd.ptau_new(power), "first", rand64=RAND64, name="first")
    rnd = lambda t: {k: round(v, 2) for k, v in t.items()}  # noqa: E731

    t0 = time.time()
    challenge = zkp_amd.ptau_export_challenge(old)
    wall = time.time() - t0
    t = zkp_amd.ptau_challenge_timings()
    res["export_challenge"] = {"wall_s": round(wall, 3), "bytes": len(challenge), "timings_ms": rnd(t),
                               "bound_by": "the hash of the challenge file as it is written (hash_threads)"
                               if t["hash_threads"] > 0.5 * t["total"] else "not the hash"}
    t0 = time.time()
    response = zkp_amd.ptau_challenge_contribute(challenge, "bench contribution", rand64=RAND64_B)
    wall = time.time() - t0
    t = zkp_amd.ptau_challenge_timings()
    res["challenge_contribute"] = {"wall_s": round(wall, 3), "bytes": len(response), "timings_ms": rnd(t),
                                   "device_ms": round(t["decode"] + t["parse_point_check"] + t["g1_scale"] + t["g2_scale"], 2),
                                   "bound_by": "the hash of the challenge file (challenge_hash)"
                                   if t["challenge_hash"] > t["g1_scale"] + t["g2_scale"] else "the scaling on the device"}
    del challenge
    t0 = time.time()
    new = zkp_amd.ptau_import_response(old, response, name="second")
    wall = time.time() - t0
    t = zkp_amd.ptau_challenge_timings()
    dec = {}
    for key, pts, products in (("g1", g1_points, G1_PRODUCTS), ("g2", g2_points, G2_PRODUCTS)):
        s = t[key + "_decompress"] / 1e3
        dec[key] = {"ns_per_point": round(s * 1e9 / pts, 2), "fq_products": pts * products,
                    "fraction_of_v_mad_u64_u32_peak": round(pts * products * MADS_PER_PRODUCT / s / peak, 4)}
    res["import_response"] = {"wall_s": round(wall, 3), "timings_ms": rnd(t), "decompress": dec,
                              "bound_by": "the two chained hashes on one host thread: the response file's, then the next "
                                          "challenge's over the uncompressed sections (hash_threads)"
                              if t["hash_threads"] > 0.5 * t["total"] else "not the hashes"}
    del response
    t0 = time.time()
    yard = zkp_amd.ptau_contribute(old, "bench contribution", rand64=RAND64_B, name="second")
    wall = time.time() - t0
    res["contribute_yardstick"] = {"wall_s": round(wall, 3), "timings_ms": rnd(zkp_amd.ptau_contribute_timings())}
    res["import_equals_contribute"] = new == yard
    res["import_wall_over_contribute_wall"] = round(res["import_response"]["wall_s"] / wall, 3)
    del yard, old
    t0 = time.time()
    ok, msg = zkp_amd.ptau_verify(new, seed=COEFF_SEED)
    res["verify"] = {"wall_s": round(time.time() - t0, 3), "verdict": msg, "timings_ms": rnd(zkp_amd.ptau_verify_timings())}
    print(json.dumps(res), flush=True)
    return 0 if ok and msg == "OK" and res["import_equals_contribute"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--powers", default="16,20,24")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args.child))
    results, failed = [], False
    for power in [int(p) for p in args.powers.split(",") if p]:
        need_gb = 6 * 384 * (1 << power) / 1e9 + 4
        if mem_available_gb() < need_gb:
            results.append({"power": power, "skipped": "host memory: %.0f GB available, %.0f GB wanted" % (mem_available_gb(), need_gb)})
            print(json.dumps(results[-1]), flush=True)
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(power)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S.get(power, 600))
        except subprocess.TimeoutExpired:
            print("power %d: time limit of %d s" % (power, LIMIT_S.get(power, 600)), file=sys.stderr)
            failed = True
            break
        sys.stderr.write(r.stderr)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if lines:
            results.append(json.loads(lines[-1]))
            print(lines[-1], flush=True)
        if r.returncode != 0:  # nothing more starts after a failure
            print("power %d: exit status %d" % (power, r.returncode), file=sys.stderr)
            failed = True
            break
    if args.out and results:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    bad = [x for x in results if "skipped" not in x and x.get("verify", {}).get("verdict") != "OK"]
    sys.exit(1 if bad or failed or not results else 0)


if __name__ == "__main__":
    main()
