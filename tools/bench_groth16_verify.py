#!/usr/bin/env python3
"""Measure batched `groth16 verify` (zkp_verifier_verify) against the host verifier (zkp_proof_verify) and write
profiles/groth16_verify.json.

    python tools/bench_groth16_verify.py [--sizes 1,256,4096,65536] [--reps 20] [--out profiles/groth16_verify.json]

One box, one GPU; every figure is the median of --reps calls after one warm-up call, and the file says so.
Proofs: 256 distinct circuit_tiny proofs from the GPU prover (random r, s), repeated cyclically to fill a batch
(the verifier does the same work for a repeated proof: coefficients differ per position).  Per size: the batch
call's wall time and the zkp_verifier_timings split.  At 4096 also: one bad proof, 1 % bad proofs, and
zkp_proof_verify over the same proofs on 16 host threads; on 1 thread over the first 256 of them (per-proof
time, extrapolated to the batch and marked so)."""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zk-p2p-onramp_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import zkp_amd  # noqa: E402
from oracle import bn254  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
# a Miller loop's field products per lane, counted from csrc/pairing_kernels.hpp: per doubling step 12 + 15 Fq2
# products of f12_sqr_mem / f12_mul_line_mem and 17 of dbl_step; per addition step 15 + 14; an Fq2 product is 4
# Fq products + 2 reductions = 6 x 81 v_mad_u64_u32 (mul2 sums count as two)
DBL_STEPS, ADD_STEPS = 64, bin(0x9d797039be763ba8).count("1") + 2
FQ2_PRODUCTS = DBL_STEPS * (12 + 15 + 17) + ADD_STEPS * (15 + 14)
MADS_PER_LOOP = FQ2_PRODUCTS * 6 * 81


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,256,4096,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify.json"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    zk = open(os.path.join(GOLD, "circuit_tiny.zkey"), "rb").read()
    wt = open(os.path.join(GOLD, "circuit_tiny.wtns"), "rb").read()
    rng = random.Random(4096)
    prover = zkp_amd.Prover(zk, devices=[0])
    base = prover.prove_batch_raw([wt] * 256, [rng.randrange(1, bn254.R) for _ in range(256)],
                                  [rng.randrange(1, bn254.R) for _ in range(256)])
    prover.close()
    base = [(p, list(pub)) for p, pub in base]
    v = zkp_amd.Verifier(zkp_amd.export_verification_key(zk))
    peak = None
    try:
        ub = json.load(open(os.path.join(ROOT, "profiles", "ubench_r05.json")))
        peak = ub.get("v_mad_u64_u32_tops")
    except Exception:
        pass
    res = {"what": "zkp_verifier_verify on circuit_tiny proofs; medians of %d calls after one warm-up, one box, one GPU"
                   % args.reps,
           "proofs": "256 distinct GPU proofs repeated cyclically", "mads_per_miller_loop_counted": MADS_PER_LOOP,
           "sizes": {}}

    def bad(item):
        (a, b, c), pub = item
        return ((a, b, bn254.g1_add(c, bn254.G1_GEN)), pub)

    for n in sizes:
        items = [base[i % 256] for i in range(n)]
        splits = []

        def call(items=items):
            assert all(v.verify_batch(items))
            splits.append(v.timings())

        reps = args.reps if n < 65536 else min(args.reps, 5)  # building 65,536 argument structs in Python dominates
        median_ms(call, reps)
        split = {k: statistics.median(s[k] for s in splits[1:]) for k in splits[0]}
        ms = split["total_ms"]  # the library's own wall time of the call: no Python marshalling in it
        row_reps = reps
        row = {"reps": row_reps, "batch_ms": ms, "per_proof_us": ms * 1e3 / n, "timings_median": split}
        if split["miller_ms"] > 0:
            row["miller_kernel_mads_T_per_s"] = n * MADS_PER_LOOP / (split["miller_ms"] * 1e-3) / 1e12
        if n == 4096:
            one = list(items)
            one[1234] = bad(one[1234])
            pct = list(items)
            for i in random.Random(1).sample(range(n), n // 100):
                pct[i] = bad(pct[i])
            for name, its in (("one_bad", one), ("one_percent_bad", pct)):
                want = [x is y for x, y in zip(its, items)]
                got = []
                tms = []

                def bad_call(its=its):
                    got.append(v.verify_batch(its))
                    tms.append(v.timings())

                median_ms(bad_call, max(3, args.reps // 4))
                assert got[-1] == want
                row[name + "_ms"] = statistics.median(t["total_ms"] for t in tms[1:])
                row[name + "_search_ms"] = statistics.median(t["search_ms"] for t in tms[1:])
                row[name + "_node_checks"] = tms[-1]["node_checks"]
            # through the same Python binding (about 1 % marshalling per call beside the 2.6 ms check)
            host = lambda it: zkp_amd.proof_verify(zk, it[0], it[1])  # noqa: E731
            with ThreadPoolExecutor(16) as ex:
                row["host_16_threads_ms"] = median_ms(lambda: list(ex.map(host, items, chunksize=64)), 3)
            sub = items[:256]
            one_ms = median_ms(lambda: [host(it) for it in sub], 3)
            row["host_1_thread_per_proof_ms"] = one_ms / len(sub)
            row["host_1_thread_ms_extrapolated"] = one_ms / len(sub) * n
            row["batch_not_slower_than_16_host_threads"] = ms <= row["host_16_threads_ms"]
        res["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
    if peak:
        res["v_mad_u64_u32_peak_T_per_s"] = peak
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
