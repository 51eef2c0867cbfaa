#!/usr/bin/env python3
"""Phase 1 from its start on one MI355X, timed through the C ABI: per power `zkp_ptau_new` ->
`zkp_ptau_contribute` -> `zkp_ptau_beacon` -> `zkp_ptau_verify` (reference
circuit/scripts/generate_keys_phase1.sh:6,8,18,16).  The verdict must be "OK".

Every power runs in a child process of its own under a time limit; the first failure ends the run.  Power 24
runs only if the host has memory for it (the file is 6.4 GB; a call holds its input, its output and two
transient copies of the output).

Per power, one JSON line (collected into --out as a list):
* the timing vector of each call (zkp_ptau_contribute_timings, zkp_ptau_verify_timings) and its wall time;
* ns per G1 and per G2 point of k_scale_powers (device time of the contribute call), and the kernel's field
  products per second as a fraction of the measured v_mad_u64_u32 peak of profiles/ubench_r05.json: per point
  the 2-bit ladder over a 254-bit scalar is 254 doublings and 127 * 3/4 additions (a digit is nonzero with
  probability 3/4; the wave pays for all 127 where lanes diverge, which is what the fraction shows), 9 field
  products per doubling and 14 per addition, 3 Fq products per Fq2 product, 136 multiply-accumulates per
  product, as DESIGN §8f / §8g count them;
* with --common-scalar: the in-project yardstick, `zkp_zkey_contribute` (k_scale_points: one common scalar,
  wave-uniform branches) over the L and H sections of a synthetic key with 2^power constraints, about
  2 * 2^power G1 points, as wall ns per point beside the wall ns per point of the contribute call.
usage: bench_ptau_contribute.py [--powers 16,20,24] [--common-scalar] [--out profiles/ptau_contribute.json]"""
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
BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
COEFF_SEED = bytes(range(100, 132))
LADDER_DBL, LADDER_ADD = 254, 127 * 0.75
ADD_PRODUCTS, DBL_PRODUCTS, FQ_PER_FQ2, MADS_PER_PRODUCT = 14, 9, 3, 136
LIMIT_S = {16: 240, 20: 420, 24: 1100}


def mem_available_gb():
    for ln in open("/proc/meminfo"):
        if ln.startswith("MemAvailable:"):
            return int(ln.split()[1]) / 1e6
    return 0.0


def child(power, common_scalar):
    import zkp_amd
    N = 1 << power
    g1_points, g2_points = 4 * N - 1, N + 1
    peak = json.load(open(os.path.join(ROOT, "profiles", "ubench_r05.json")))["v_mad_u64_u32_tops"] * 1e12
    res = {"op": "powersoftau new -> contribute -> beacon -> verify", "power": power,
           "points": {"g1": g1_points, "g2": g2_points}}
    # warm-up: the device, the code objects and the first pinned allocation
    zkp_amd.ptau_contribute(zkp_amd.ptau_new(4), "warm", rand64=RAND64)
    t0 = time.time()
    fresh = zkp_amd.ptau_new(power)
    res["new"] = {"wall_s": round(time.time() - t0, 3), "bytes": len(fresh)}

    def scale_figures(t):
        out = {}
        per_lane = LADDER_DBL * DBL_PRODUCTS + LADDER_ADD * ADD_PRODUCTS
        for key, pts, fq in (("g1", g1_points, 1), ("g2", g2_points, FQ_PER_FQ2)):
            s = t[key + "_scale"] / 1e3
            out[key] = {"ns_per_point": round(s * 1e9 / pts, 1),
                        "fq_products": round(pts * per_lane * fq),
                        "fraction_of_v_mad_u64_u32_peak": round(pts * per_lane * fq * MADS_PER_PRODUCT / s / peak, 4)}
        return out

    t0 = time.time()
    first = zkp_amd.ptau_contribute(fresh, "bench contribution", rand64=RAND64, name="first")
    wall = time.time() - t0
    t = zkp_amd.ptau_contribute_timings()
    res["contribute"] = {"wall_s": round(wall, 3), "timings_ms": {k: round(v, 2) for k, v in t.items()},
                         "scale": scale_figures(t), "wall_ns_per_point": round(wall * 1e9 / (g1_points + g2_points), 1)}
    del fresh
    t0 = time.time()
    final = zkp_amd.ptau_beacon(first, BEACON, 10, name="final beacon")
    wall = time.time() - t0
    t = zkp_amd.ptau_contribute_timings()
    res["beacon"] = {"wall_s": round(wall, 3), "timings_ms": {k: round(v, 2) for k, v in t.items()}, "scale": scale_figures(t)}
    del first
    t0 = time.time()
    ok, msg = zkp_amd.ptau_verify(final, seed=COEFF_SEED)
    wall = time.time() - t0
    res["verify"] = {"wall_s": round(wall, 3), "verdict": msg,
                     "timings_ms": {k: round(v, 2) for k, v in zkp_amd.ptau_verify_timings().items()}}
    del final
    if common_scalar:
        from zkp_amd import synth
        circ = synth.Circuit(N, N - 64, 26, 0x5A4B5032)
        key = circ.zkey(0x5A4B5033, device=0)
        zkp_amd.zkey_contribute(key, 0x1234567 + (1 << 200))  # warm
        pts = (circ.n_vars - circ.n_public - 1) + circ.domain_size
        t0 = time.time()
        zkp_amd.zkey_contribute(key, 0x2b1f3c5d7e9a0b1c2d3e4f5061728394a5b6c7d8e9fa0b1c2d3e4f5061728394 % (1 << 253))
        wall = time.time() - t0
        res["common_scalar_yardstick"] = {"call": "zkp_zkey_contribute (k_scale_points over sections 8 and 9)", "g1_points": pts,
                                          "wall_s": round(wall, 3), "wall_ns_per_point": round(wall * 1e9 / pts, 1)}
    print(json.dumps(res), flush=True)
    return 0 if ok and msg == "OK" else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--powers", default="16,20,24")
    ap.add_argument("--common-scalar", action="store_true", help="also time zkp_zkey_contribute on about 2 * 2^power points")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.exit(child(args.child, args.common_scalar))
    results, failed = [], False
    for power in [int(p) for p in args.powers.split(",") if p]:
        need_gb = 4.5 * 384 * (1 << power) / 1e9 + 4
        if mem_available_gb() < need_gb:
            results.append({"power": power, "skipped": "host memory: %.0f GB available, %.0f GB wanted" % (mem_available_gb(), need_gb)})
            print(json.dumps(results[-1]), flush=True)
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(power)] + (["--common-scalar"] if args.common_scalar else [])
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
