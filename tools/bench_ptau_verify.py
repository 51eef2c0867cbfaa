#!/usr/bin/env python3
"""`powersoftau verify`, the point sections, on one MI355X (zkp_ptau_verify_sections; reference
circuit/scripts/generate_keys_phase1.sh:16), timed through the C ABI.

Input (tooling, not timed): the prepared known-tau ptau of power P built on the GPU (zkp_synth_ptau), verified
in place (no copy) under a fixed seed after one warm-up at power 10.  The verdict must be "OK".

One JSON line: the zkp_ptau_verify_timings fields and, beside them, the yardsticks of the same run:
* zkp_ptau_prepare_phase2 of the same file stripped to sections 1-7 (--prepare);
* the tauG1 and tauG2 pair sums through zkp_rlc_pairs against the same sums through the public MSMs
  zkp_msm_g1 / zkp_msm_g2 with the coefficients widened to 32-byte scalars, two MSMs per section, as
  DESIGN §8e measured zkey verify (--msm; wall times, uploads included on both sides);
* the subgroup kernel's field products per second (per point 253 doublings and 80 additions of the 2-bit
  ladder over r; 9 and 14 Fq2 products, each 3 Fq products of 136 multiply-accumulates, as bench_prepare.py
  counts them) as a fraction of the measured v_mad_u64_u32 peak of profiles/ubench_r05.json.
usage: bench_ptau_verify.py --power P [--prepare] [--msm] [--out FILE (appended)]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zkp_amd  # noqa: E402
from zkp_amd import synth  # noqa: E402
from bench_prepare import prepare, sections, strip  # noqa: E402

SEED = 0x5A4B5033
COEFF_SEED = bytes(range(100, 132))
LADDER_DBL, LADDER_ADD = 253, 80
ADD_PRODUCTS, DBL_PRODUCTS, FQ_PER_FQ2, MADS_PER_PRODUCT = 14, 9, 3, 136
u8p = ctypes.POINTER(ctypes.c_uint8)


def verify(lib, ptr, n):
    ok, msg = ctypes.c_int(), ctypes.create_string_buffer(256)
    seed = ctypes.cast(ctypes.c_char_p(COEFF_SEED), u8p)
    t0 = time.time()
    st = lib.zkp_ptau_verify_sections(0, ptr, n, seed, ctypes.byref(ok), msg, 256)
    dt = time.time() - t0
    if st != 0:
        raise SystemExit("zkp_ptau_verify_sections: status %d: %s" % (st, lib.zkp_last_error().decode()))
    return bool(ok.value), msg.value.decode(), dt


def pair_sums_both_ways(view, secs, sid):
    """wall s of zkp_rlc_pairs over section sid and of the same two sums through two public MSMs"""
    g2 = sid == 3
    pb = 128 if g2 else 64
    o, ln = secs[sid]
    pts = bytes(view[o:o + ln])
    n = ln // pb
    t0 = time.time()
    a, b = zkp_amd.rlc_pairs(COEFF_SEED, 0, pts, g2=g2)
    t_pairs = time.time() - t0
    t0 = time.time()
    co = zkp_amd.rlc_coeffs(COEFF_SEED, 0, n - 1)
    scal = b"".join(c.to_bytes(32, "little") for c in co)
    t_coeffs = time.time() - t0
    msm = zkp_amd.msm_g2 if g2 else zkp_amd.msm_g1
    t0 = time.time()
    a2 = msm(pts[:-pb], scal)
    b2 = msm(pts[pb:], scal)
    t_msm = time.time() - t0
    return {"points": n, "rlc_pairs_s": round(t_pairs, 3), "two_public_msms_s": round(t_msm, 3),
            "coefficients_to_host_s": round(t_coeffs, 3), "equal": (a, b) == (a2, b2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, required=True)
    ap.add_argument("--prepare", action="store_true", help="also time zkp_ptau_prepare_phase2 at this power")
    ap.add_argument("--msm", action="store_true", help="also compute the pair sums through zkp_msm_g1 / zkp_msm_g2")
    ap.add_argument("--out", default="", help="append the JSON line to this file")
    args = ap.parse_args()
    lib = zkp_amd.load_library()
    warm = synth.ptau(10, SEED, device=0)
    assert verify(lib, warm.ptr, warm.len)[0]
    del warm
    t0 = time.time()
    full = synth.ptau(args.power, SEED, device=0)
    t_synth = time.time() - t0
    print("# synthetic ptau power %d: %.2f GB in %.1f s" % (args.power, full.len / 1e9, t_synth), file=sys.stderr, flush=True)
    ok, msg, wall = verify(lib, full.ptr, full.len)
    t = zkp_amd.ptau_verify_timings()
    N = 1 << args.power
    g2_points = N + 1 + 2 * N - 1
    peak = json.load(open(os.path.join(ROOT, "profiles", "ubench_r05.json")))["v_mad_u64_u32_tops"] * 1e12
    products = g2_points * (LADDER_DBL * DBL_PRODUCTS + LADDER_ADD * ADD_PRODUCTS) * FQ_PER_FQ2
    sub_s = t["subgroup_check"] / 1e3
    res = {"op": "powersoftau verify (sections)", "power": args.power, "input_bytes": full.len, "valid": ok, "message": msg,
           "wall_s": round(wall, 3), "timings_ms": {k: round(v, 2) for k, v in t.items()},
           "points": {"g1": (2 * N - 1) + 2 * N + 3 * (2 * N - 1), "g2": g2_points},
           "ns_per_point": round(wall * 1e9 / ((2 * N - 1) * 5 + 3 * N + 1), 1),
           "subgroup": {"g2_points": g2_points, "doublings_per_point": LADDER_DBL, "additions_per_point": LADDER_ADD,
                        "fq_products": products, "mac_per_field_product": MADS_PER_PRODUCT,
                        "ns_per_point": round(sub_s * 1e9 / g2_points, 1) if sub_s > 0 else None,
                        "fraction_of_v_mad_u64_u32_peak": round(products * MADS_PER_PRODUCT / sub_s / peak, 4) if sub_s > 0 else None},
           "inputs_note": "known-tau tooling input (zkp_synth_ptau %.1f s), not timed" % t_synth}
    if args.prepare or args.msm:
        stripped, view, secs = strip(full)
        if args.msm:
            res["pair_sums"] = {"tauG1": pair_sums_both_ways(view, secs, 2), "tauG2": pair_sums_both_ways(view, secs, 3)}
        if args.prepare:
            out, out_len, pwall = prepare(lib, ctypes.cast(ctypes.c_char_p(stripped), u8p), len(stripped))
            lib.zkp_buffer_free(out)
            res["prepare_phase2_same_power"] = {"wall_s": round(pwall, 3), "verify_over_prepare": round(wall / pwall, 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not ok or (args.msm and not all(v["equal"] for v in res["pair_sums"].values())):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
