"""The general XYZZ addition's doubling and cancellation branches on the GPU, in every stage after the
buckets are filled -- among them the two reductions that no CPU replay runs as the device does: the shuffle
butterfly rowcol_tree (the branches sit between the shuffles of a wave) and the workgroup LDS trees (a
lazily reduced x passes through LDS into the doubling).

The inputs are the designed catalogue of tests/helpers/msm_designs.py, which tests/test_host_xyzz_events.py
certifies on the CPU to reach the branches it aims at; here each design runs through zkp_amd.msm_g1 /
msm_g2 on both plan variants and must equal the oracle's MSM bit for bit.  One prover-level case: a small
synthetic key whose A, B1, B2 and C sections hold copies and negations of other bases, with a witness whose
values on those signals are small and neighbouring, so that equal and opposite bucket sums meet in the row
and column chains and trees of the witness MSMs."""
import functools
import os
import sys
import time

import pytest

from oracle import binfile, bn254, cpu_oracle
import zkp_amd
from zkp_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import msm_designs as md  # noqa: E402

pytestmark = pytest.mark.gpu
POINTS = {}


@pytest.mark.parametrize("plan", ["dense", "compact"])
@pytest.mark.parametrize("c", sorted({cfg[0] for cfg in md.CONFIGS}))
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_designs_equal_oracle(monkeypatch, curve, c, plan):
    if curve not in POINTS:
        POINTS[curve] = md.Points(curve)
    pts = POINTS[curve]
    gpu = zkp_amd.msm_g2 if curve == "g2" else zkp_amd.msm_g1
    wrong, ran, t_gpu = [], 0, 0.0
    for cfg in md.CONFIGS:
        if cfg[0] != c:
            continue
        geo = md.Geometry(*cfg)
        monkeypatch.setenv("ZKP_MSM", geo.zkp_msm(plan))
        for d in md.designs(geo):
            p, s, _ = pts.encode(d, c)
            want = pts.expected(d, c)
            t0 = time.perf_counter()
            got = gpu(p, s, window_bits=c, table_depth=cfg[1])
            t_gpu += time.perf_counter() - t0
            ran += 1
            if got != want:
                print("wrong:", curve, plan, cfg, d.name, d.targets)   # every one: the assertion's list is cut short
                wrong.append((cfg, d.name, d.targets))
    print("%s c=%d %s: %d MSMs, %.2f s on the GPU path" % (curve, c, plan, ran, t_gpu))
    assert ran > 0 and not wrong, wrong


# ------------------------------------------------------------------ prover

N_VARS, N_CONS, N_PUB = 3001, 3500, 5
R_FIX, S_FIX = 0x1234567, 0x7654321
P_MOD = bn254.P
FIRST = 64    # the first designed signal (private; the designed signals are consecutive)
# (source base, negated, witness value): value v sits in bucket k = v - 1 of window 0, k = u V + v.  The witness
# MSMs take c = 8 (U x V = 8 x 16 buckets) or, as the second configuration, c = 10 (16 x 32); both sum chains
# of 8 buckets, so a row has 2 (4) partials.  Every other private value is 0 or 1 (bool_pct=100) and the
# public ones are set to 1: only bucket 0 holds anything else, and every value stays a single positive digit
# (<= 128).
PLACED = [
    (0, False, 33), (0, False, 34),                  # neighbours in one row at both widths, equal: a row chain doubles
    (1, False, 65), (1, True, 66), (2, False, 67),   # P, -P, then Q behind the infinity, in a row chain
    (3, False, 41), (3, False, 73),                  # column 8 at both widths, one chain: it doubles
    (4, False, 26), (4, True, 42), (4, False, 74),   # column 9: P - P + P at c = 8, -P + P at c = 10
    (5, False, 50), (5, False, 58),                  # the two partials of a lane (pair add) at both widths
    (6, False, 99), (6, True, 115),                  # c = 10: partials 0 and 2 of row 3, opposite (butterfly)
    (7, False, 1), (7, False, 2), (7, True, 3),      # row 0: no row sum may see them
]


def _neg(pt: bytes) -> bytes:
    """-(x, y) in the zkey's Montgomery encoding (32-byte words; y is the second half)"""
    half = len(pt) // 2
    ys = [bn254.le_to_int(pt[half + 32 * i:half + 32 * i + 32]) for i in range(half // 32)]
    return pt[:half] + b"".join(bn254.int_to_le((P_MOD - y) % P_MOD) for y in ys)


@functools.lru_cache(maxsize=None)
def _case():
    circ = synth.Circuit(N_VARS, N_CONS, N_PUB, 0x5A4B5032, bool_pct=100)
    zk = bytearray(circ.zkey(0x5A4B5033).bytes())
    _, secs = binfile.read_binfile(bytes(zk), b"zkey", 1)
    nsrc = 1 + max(s for s, _, _ in PLACED)
    last = FIRST + len(PLACED)
    srcs = {}
    for name, sid, pw, first in (("A", 5, 64, 0), ("B1", 6, 64, 0), ("B2", 7, 128, 0), ("C", 8, 64, N_PUB + 1)):
        pos, _ = secs[sid][0]

        def at(i):
            return pos + pw * (i - first)
        # the sources: finite bases behind the designed signals (B2 takes B1's: one plan serves both)
        if name == "B2":
            srcs[name] = srcs["B1"]
        else:
            srcs[name] = [i for i in range(last, N_VARS) if any(zk[at(i):at(i) + pw])][:nsrc]
        assert len(srcs[name]) == nsrc and all(any(zk[at(i):at(i) + pw]) for i in srcs[name])
        for j, (s, neg, _) in enumerate(PLACED):
            pt = bytes(zk[at(srcs[name][s]):at(srcs[name][s]) + pw])
            zk[at(FIRST + j):at(FIRST + j) + pw] = _neg(pt) if neg else pt
    zk = bytes(zk)
    wt = circ.witness(11)
    off = len(wt) - 32 * N_VARS
    w = bytearray(wt)
    for j, (_, _, v) in enumerate(PLACED):
        w[off + 32 * (FIRST + j):off + 32 * (FIRST + j + 1)] = bn254.int_to_le(v)
    for i in range(1, N_PUB + 1):
        w[off + 32 * i:off + 32 * (i + 1)] = bn254.int_to_le(1)
    wt = bytes(w)
    vals = [bn254.le_to_int(wt[off + 32 * i:off + 32 * i + 32]) for i in range(N_VARS)]
    assert all(v <= 1 for i, v in enumerate(vals) if not FIRST <= i < last)   # the premise of PLACED
    want, _ = cpu_oracle.prove(zk, wt, R_FIX, S_FIX, threads=8)
    return zk, wt, want


@pytest.mark.parametrize("wsel", ["first", "second"])
def test_prover_with_duplicate_bases(monkeypatch, wsel):
    """The witness does not satisfy the circuit; the proof is still a function of (key, witness, r, s)."""
    zk, wt, want = _case()
    monkeypatch.setenv("ZKP_MSM", "wsel=" + wsel)
    p = zkp_amd.Prover(zk, devices=[0])
    try:
        cfg = p.msm_config()
        assert cfg["witness"]["c"] == 8 and cfg["witness_second"]["c"] == 10     # what PLACED is laid out for
        got, _ = p.prove_raw(wt, R_FIX, S_FIX)
        took = p.timings()["witness_config"]
        p.stage(wt, slot=0)
        staged, _ = p.prove_staged_raw(0, R_FIX, S_FIX)
    finally:
        p.close()
    assert took == (1 if wsel == "second" else 0)
    assert got == want
    assert staged == want
