#!/usr/bin/env python3
"""`powersoftau prepare phase2` on one MI355X (zkp_ptau_prepare_phase2; reference
circuit/scripts/generate_keys_phase1.sh:20), timed through the C ABI.

Input (tooling, not timed): the known-tau ptau of power P built on the GPU (zkp_synth_ptau), stripped to
sections 1-7.  After one warm-up at power 10 it is prepared once; sections 12-15 of the result must equal
the synthetic file's, whose Lagrange points come from the closed form L_c(tau), not from an iFFT.

One JSON line: the zkp_ptau_prepare_timings fields, the points per level, the group additions and
doublings the schedule performs on generic points (counted from the twiddles: per butterfly the two
additions of a +- t b, and bitlen(t) - 1 doublings and popcount(t) - 1 additions for each scalar
multiplication, none for t = 1), and the field products per second of the G1 part (14 per XYZZ addition,
9 per doubling, each 136 multiply-accumulates as bench.py's rooflines count a field product: SURVEY.md
§8d D4) as a fraction of the measured v_mad_u64_u32 peak of profiles/ubench_r05.json.
usage: bench_prepare.py --power P [--window 1|2] [--out FILE (appended)]"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-p2p-onramp_amd"))
import zkp_amd  # noqa: E402
from zkp_amd import synth  # noqa: E402

SEED = 0x5A4B5033
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT_28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904  # Fr.w[28]
ADD_PRODUCTS, DBL_PRODUCTS, MADS_PER_PRODUCT = 14, 9, 136
DEFAULT_WINDOW = 2  # ptau_prepare.hip DEFAULT_WINDOW_G1 / _G2


def sections(view):
    n = struct.unpack_from("<I", view, 8)[0]
    o, out = 12, {}
    for _ in range(n):
        sid, ln = struct.unpack_from("<IQ", view, o)
        out[sid] = (o + 12, ln)
        o += 12 + ln
    return out


M55 = int("55" * 32, 16)


def scalar_ops(x, window):
    """(additions, doublings) of gfft::scale for the scalar x != 1 on a finite point: the first digit's step
    lands on infinity and costs nothing; the 2-bit window adds 2b (a doubling) and 3b (an addition)"""
    if window == 1:
        return bin(x).count("1") - 1, x.bit_length() - 1
    digits, nonzero = (x.bit_length() + 1) // 2, bin((x | (x >> 1)) & M55).count("1")
    return nonzero, 2 * (digits - 1) + 1


def schedule_ops(power, window=1):
    """(additions, doublings) of one vector over levels 0..power.  Stage s of any level uses the twiddles
    w_(2^(s+1))^-k, k < 2^s, each in 2^(p-1-s) butterflies; the last stage (s = p - 1) multiplies both
    operands: a by 2^-p and b by 2^-p w_(2^p)^-k."""
    if power == 0:
        return 0, 0
    top = power - 1  # twiddles of stage s: g^(k 2^(top - s)), g = w_(2^power)^-1
    g = pow(pow(ROOT_28, 1 << (28 - power), R), R - 2, R)
    sums = [[0, 0] for _ in range(power)]  # per stage s: sum over k of (popcount - 1, bitlen - 1), t != 1
    t = 1
    for e in range(1 << top):
        if e:
            tz = (e & -e).bit_length() - 1
            a, d = scalar_ops(t, window)
            for s in range(top - min(tz, top), power):
                sums[s][0] += a
                sums[s][1] += d
        t = t * g % R
    adds = dbls = 0
    half = (R + 1) // 2
    for p in range(1, power + 1):
        n = 1 << p
        adds += (n // 2) * 2 * p  # the butterflies' own two additions
        for s in range(p - 1):
            adds += sums[s][0] << (p - 1 - s)
            dbls += sums[s][1] << (p - 1 - s)
        ninv = pow(half, p, R)
        gp = pow(pow(ROOT_28, 1 << (28 - p), R), R - 2, R)
        t = ninv
        for _ in range(n // 2):  # the last stage: ninv on a, ninv * twiddle on b
            for x in (ninv, t):
                if x != 1:
                    a, d = scalar_ops(x, window)
                    adds += a
                    dbls += d
            t = t * gp % R
    return adds, dbls


def prepare(lib, ptr, n):
    out, out_len = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    t0 = time.time()
    st = lib.zkp_ptau_prepare_phase2(0, ptr, n, ctypes.byref(out), ctypes.byref(out_len))
    dt = time.time() - t0
    if st != 0:
        raise SystemExit("zkp_ptau_prepare_phase2: status %d: %s" % (st, lib.zkp_last_error().decode()))
    return out, out_len.value, dt


def strip(full):
    """sections 1-7 of a library-owned ptau as a new file (bytes)"""
    view = memoryview((ctypes.c_uint8 * full.len).from_address(ctypes.cast(full.ptr, ctypes.c_void_p).value))
    secs = sections(view)
    parts = [b"ptau", struct.pack("<II", 1, 7)]
    for sid in range(1, 8):
        o, ln = secs[sid]
        parts += [struct.pack("<IQ", sid, ln), view[o:o + ln]]
    return b"".join(parts), view, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, required=True)
    ap.add_argument("--out", default="", help="append the JSON line to this file")
    ap.add_argument("--window", type=int, choices=(1, 2), default=0,
                    help="window bits of the scalar multiplications (sets ZKP_GFFT_WINDOW; default: the library's)")
    args = ap.parse_args()
    if args.window:
        os.environ["ZKP_GFFT_WINDOW"] = str(args.window)
    window = int(os.environ.get("ZKP_GFFT_WINDOW") or DEFAULT_WINDOW)
    lib = zkp_amd.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    memcmp = ctypes.CDLL(None).memcmp
    memcmp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    # warm-up at power 10
    warm, _, _ = strip(synth.ptau(10, SEED, device=0))
    o, _, _ = prepare(lib, ctypes.cast(ctypes.c_char_p(warm), u8p), len(warm))
    lib.zkp_buffer_free(o)
    t0 = time.time()
    full = synth.ptau(args.power, SEED, device=0)
    t_synth = time.time() - t0
    stripped, _, fsecs = strip(full)
    print("# synthetic ptau power %d: %.2f GB in %.1f s; stripped %.2f GB" %
          (args.power, full.len / 1e9, t_synth, len(stripped) / 1e9), file=sys.stderr, flush=True)
    out, out_len, wall = prepare(lib, ctypes.cast(ctypes.c_char_p(stripped), u8p), len(stripped))
    timings = zkp_amd.ptau_prepare_timings()
    oaddr = ctypes.cast(out, ctypes.c_void_p).value
    faddr = ctypes.cast(full.ptr, ctypes.c_void_p).value
    osecs = sections(memoryview((ctypes.c_uint8 * out_len).from_address(oaddr)))
    same = {}
    for sid in (12, 13, 14, 15):
        (oo, ol), (fo, fl) = osecs[sid], fsecs[sid]
        same[str(sid)] = ol == fl and memcmp(oaddr + oo, faddr + fo, ol) == 0
    lib.zkp_buffer_free(out)
    adds, dbls = schedule_ops(args.power, window)
    peak = json.load(open(os.path.join(ROOT, "profiles", "ubench_r05.json")))["v_mad_u64_u32_tops"] * 1e12
    g1_products = 3 * (adds * ADD_PRODUCTS + dbls * DBL_PRODUCTS)
    g1_s = timings["g1_ifft"] / 1e3
    res = {"op": "powersoftau prepare phase2", "power": args.power, "input_bytes": len(stripped), "output_bytes": out_len,
           "wall_s": round(wall, 3), "timings_ms": {k: round(v, 2) for k, v in timings.items()},
           "points_per_level": [1 << p for p in range(args.power + 1)],
           "sections_12_15_equal_synthetic": same, "valid": all(same.values()),
           "per_vector": {"group_additions": adds, "group_doublings": dbls},
           "vectors": {"g1": 3, "g2": 1},
           "g1_field_products": g1_products, "mac_per_field_product": MADS_PER_PRODUCT,
           "g1_field_products_per_s": round(g1_products / g1_s) if g1_s > 0 else None,
           "g1_fraction_of_v_mad_u64_u32_peak": round(g1_products * MADS_PER_PRODUCT / g1_s / peak, 4) if g1_s > 0 else None,
           "variant": "per-thread left-to-right, %d-bit window" % window, "window_bits": window,
           "inputs_note": "known-tau tooling input (zkp_synth_ptau %.1f s), not timed" % t_synth}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if not res["valid"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
