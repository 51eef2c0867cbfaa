"""Bases at infinity emit no digit (msm.hpp BaseMask, ZKP_MSM sparse=): a base table reports the mask of
its finite bases, a plan built with it drops the scalars of the others, and a prover keeps one witness
plan per distinct mask (B1 and B2 share theirs).

* kernel-level MSMs, G1 and G2, with infinity bases (all-zero point bytes) at the bitset-word, wave and
  pass-A-block boundaries, against oracle/cpu's MSM of the same input and of the input with the infinity
  bases and their scalars removed;
* small synthetic circuits: the proof at fixed r, s equals oracle/cpu's with and without the masks, on
  both witness configurations, and as a 3-part split whose slices start inside a bitset word;
* the additions each launch reports are exactly the nonzero witness values on a finite base of its
  table (bool_pct=100: one digit per value), computed here from the key's bytes.
"""
import functools
import os

import pytest

from oracle import binfile, bn254, circuit, cpu_oracle
import zkp_amd
from zkp_amd import synth

pytestmark = pytest.mark.gpu
R = bn254.R
R_FIX, S_FIX = 0x1234567, 0x7654321
SIZES = [1, 31, 32, 33, 64, 65, 512, 513, 4097]
NMAX = max(SIZES)


# ------------------------------------------------------------------ kernel-level MSMs

@pytest.fixture(scope="module")
def msm_inputs():
    """NMAX finite points per curve (zkey layout) and the three scalar vectors, made once."""
    gen = synth.scalars(0x51, 0, NMAX)
    pts = {False: synth.points(gen, g2=False), True: synth.points(gen, g2=True)}
    rng = circuit.SplitMix64(0x52, 0)
    big = [R, R + 1, 2 * R + 5, (1 << 256) - 1000, (1 << 255) + 12345, 3 * R - 1]  # every one >= r
    sc = {
        "uniform": synth.scalars(0x53, 1, NMAX),
        "ones": b"".join(bn254.int_to_le(1) for _ in range(NMAX)),
        "above_r": b"".join(bn254.int_to_le(big[i % len(big)] + (rng.next() % 1000 if i >= len(big) else 0))
                            for i in range(NMAX)),
    }
    return pts, sc


def _patterns(n):
    """name -> list of n booleans: base i is finite"""
    rng = circuit.SplitMix64(0x54, n)
    lo = 32 if n >= 64 else 0  # the bitset word that is absent as a whole
    return {
        "none_finite": [False] * n,
        "first_only": [i == 0 for i in range(n)],
        "last_only": [i == n - 1 for i in range(n)],
        "alternating": [i % 2 == 0 for i in range(n)],
        "word_absent": [not (lo <= i < lo + 32) for i in range(n)],
        "random_75_absent": [rng.next() % 4 == 0 for _ in range(n)],
    }


def _apply(points, scalars, pw, finite):
    """(points with the absent bases zeroed, scalars) and the same with those entries removed"""
    n = len(finite)
    zero = bytes(pw)
    full = b"".join(points[pw * i:pw * i + pw] if finite[i] else zero for i in range(n))
    kp = b"".join(points[pw * i:pw * i + pw] for i in range(n) if finite[i])
    ks = b"".join(scalars[32 * i:32 * i + 32] for i in range(n) if finite[i])
    return full, scalars[:32 * n], kp, ks


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_msm_with_infinity_bases(msm_inputs, g2, n):
    pts, sc = msm_inputs
    pw = 128 if g2 else 64
    gpu = zkp_amd.msm_g2 if g2 else zkp_amd.msm_g1
    cpu = cpu_oracle.msm_g2 if g2 else cpu_oracle.msm_g1
    for pname, finite in _patterns(n).items():
        for sname, scal in sc.items():
            full, s, kp, ks = _apply(pts[g2], scal, pw, finite)
            want = cpu(full, s)
            assert cpu(kp, ks) == want, (pname, sname)  # the oracle itself: dropping them changes nothing
            if pname == "none_finite":
                assert want is None
            # default tables (every window its own row), and 13-bit windows over a single row
            assert gpu(full, s) == want, (pname, sname, "default")
            if sname != "ones":
                assert gpu(full, s, window_bits=13, table_depth=1) == want, (pname, sname, "c13 d1")
            assert gpu(kp, ks) == want, (pname, sname, "removed")


@pytest.mark.parametrize("plan", ["dense", "compact"])
def test_msm_masked_equals_unmasked(msm_inputs, monkeypatch, plan):
    """sparse=0 keeps the unmasked plan (the bases at infinity are skipped lane by lane, as before):
    both give the oracle's sum, on either plan variant."""
    pts, sc = msm_inputs
    n = 513
    finite = _patterns(n)["random_75_absent"]
    full, s, kp, ks = _apply(pts[False], sc["uniform"], 64, finite)
    want = cpu_oracle.msm_g1(kp, ks)
    for sparse in (1, 0):
        monkeypatch.setenv("ZKP_MSM", "plan=%s,sparse=%d" % (plan, sparse))
        assert zkp_amd.msm_g1(full, s) == want, sparse


@pytest.mark.parametrize("spec", ["sparse=2", "sparse=", "sparse=yes", "sparse=-1", "sparse=01"])
def test_bad_sparse_value_is_rejected(msm_inputs, golden_dir, monkeypatch, spec):
    pts, sc = msm_inputs
    monkeypatch.setenv("ZKP_MSM", spec)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.msm_g1(pts[False][:64], sc["ones"][:32])
    assert e.value.status == 1 and "ZKP_MSM" in e.value.message
    zk = open(os.path.join(golden_dir, "circuit_small.zkey"), "rb").read()
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.Prover(zk, devices=[0])
    assert e.value.status == 1 and "ZKP_MSM" in e.value.message


# ------------------------------------------------------------------ provers

N_VARS, N_CONS, N_PUB = 3001, 3500, 5  # 3-part slices start at 1000 and 2000: inside a bitset word


@functools.lru_cache(maxsize=None)
def _case(bool_pct):
    """(zkey, witness, oracle/cpu's proof at R_FIX, S_FIX) of one small synthetic circuit, made once"""
    circ = synth.Circuit(N_VARS, N_CONS, N_PUB, 0x5A4B5032, bool_pct=bool_pct)
    zk = circ.zkey(0x5A4B5033).bytes()
    wt = circ.witness(11)
    want, _ = cpu_oracle.prove(zk, wt, R_FIX, S_FIX, threads=8)
    return zk, wt, want


@pytest.fixture(scope="module", params=[0, 70, 100], ids=lambda b: "bool%d" % b)
def case(request):
    return _case(request.param)


def _finite(zk):
    """per table (zkey sections 5, 6, 7, 8 = A, B1, B2, C): is the base of signal i finite"""
    _, secs = binfile.read_binfile(zk, b"zkey", 1)
    out = {}
    for name, sid, pw, first in (("A", 5, 64, 0), ("B1", 6, 64, 0), ("B2", 7, 128, 0), ("C", 8, 64, N_PUB + 1)):
        pos, ln = secs[sid][0]
        assert ln == (N_VARS - first) * pw
        out[name] = [False] * first + [any(zk[pos + pw * i:pos + pw * i + pw]) for i in range(N_VARS - first)]
    return out


def test_synthetic_key_has_infinity_bases(case):
    """what the other prover tests rely on: A, B1 and B2 hold bases at infinity, B1 and B2 the same ones"""
    zk, _, _ = case
    f = _finite(zk)
    assert 0 < sum(f["A"]) < N_VARS and 0 < sum(f["B1"]) < N_VARS
    assert f["B1"] == f["B2"]


@pytest.mark.parametrize("spec", ["sparse=1", "sparse=0", "sparse=1,wsel=first", "sparse=1,wsel=second",
                                  "sparse=0,wsel=second", None])
def test_proof_equals_oracle(case, monkeypatch, spec):
    zk, wt, want = case
    if spec is None:
        monkeypatch.delenv("ZKP_MSM", raising=False)
    else:
        monkeypatch.setenv("ZKP_MSM", spec)
    p = zkp_amd.Prover(zk, devices=[0])
    try:
        if spec and "wsel" in spec:
            assert p.msm_config()["witness_second"]
        got, _ = p.prove_raw(wt, R_FIX, S_FIX)
        took = p.timings()["witness_config"]
        p.stage(wt, slot=0)
        staged, _ = p.prove_staged_raw(0, R_FIX, S_FIX)
    finally:
        p.close()
    assert got == want and staged == want
    if spec and "wsel" in spec:
        assert took == (1 if "second" in spec else 0)


@pytest.mark.parametrize("sparse", [1, 0])
def test_three_part_split_equals_unsplit(case, monkeypatch, sparse):
    zk, wt, want = case
    monkeypatch.setenv("ZKP_MSM", "sparse=%d" % sparse)
    parts = []
    for k in range(3):
        p = zkp_amd.Prover(zk, devices=[0], part=k, nparts=3)
        try:
            parts.append(p.prove_partial(wt))
        finally:
            p.close()
    combined, _ = zkp_amd.proof_combine_raw(zk, parts, wt, R_FIX, S_FIX)
    p = zkp_amd.Prover(zk, devices=[0])
    try:
        unsplit, _ = p.prove_raw(wt, R_FIX, S_FIX)
    finally:
        p.close()
    assert combined == unsplit == want


def _launch_adds(zk, wt, spec, monkeypatch):
    """({kind: adds} of one instrumented proof, the witness plan's window bits)"""
    monkeypatch.setenv("ZKP_MSM", spec)
    p = zkp_amd.Prover(zk, devices=[0])
    try:
        c = p.msm_config()["witness"]["c"]
        p.instrument(True)
        p.prove_raw(wt, R_FIX, S_FIX)
        rec = p.launch_stats()
    finally:
        p.close()
    adds = {}
    for r in rec:
        assert r["msm"] not in adds  # one proof: one launch per kind
        adds[r["msm"]] = r["adds"]
    return adds, c


def _digits(v, c):
    """nonzero signed c-bit digits of v < r (msm_kernels.hpp digit_mag): the additions it costs"""
    half, full, carry, cnt = 1 << (c - 1), 1 << c, 0, 0
    for w in range((255 + c - 1) // c):
        raw = ((v >> (w * c)) & (full - 1)) + carry
        carry = 1 if raw > half else 0
        cnt += (full - raw if carry else raw) != 0
    return cnt


def test_launch_adds_count_finite_bases(monkeypatch):
    """bool_pct=100: every private witness value is 0 or 1, so a nonzero private value on a finite base
    is exactly one digit and each launch's `adds` is a plain count over its own table: the signals
    with w_i != 0 and a nonzero base in zkey sections 5, 6, 7, 8.  The public values (64-bit, a handful)
    are not single digits, and a key's A section does hold a finite base for each of them (the
    setup's public-input rows), so they count by their nonzero signed window digits; every other
    signal must count one."""
    zk, wt, _ = _case(100)
    _, w = binfile.read_wtns(wt)
    assert len(w) == N_VARS
    f = _finite(zk)
    got, c = _launch_adds(zk, wt, "sparse=1,wsel=first", monkeypatch)
    dig = [_digits(x, c) for x in w]
    assert all(dig[i] == (1 if w[i] else 0) for i in range(N_PUB + 1, N_VARS))  # the premise
    assert dig[0] == 1
    want = {k: sum(dig[i] for i in range(N_VARS) if f[k][i]) for k in ("A", "B1", "B2", "C")}
    signals = {k: sum(1 for i in range(N_VARS) if w[i] and f[k][i]) for k in want}
    print("adds sparse=1:", got, "expected:", want, "signals:", signals)
    assert {k: got[k] for k in want} == want
    for k in ("B1", "B2", "C"):  # no public value on a finite base: digits are signals
        assert want[k] == signals[k], k
    assert got["B1"] == got["B2"]
    assert got["A"] < got["C"] and got["B1"] < got["C"]
    flat, _ = _launch_adds(zk, wt, "sparse=0,wsel=first", monkeypatch)
    print("adds sparse=0:", flat)
    assert flat["A"] == flat["B1"] == flat["B2"] == flat["C"] == sum(dig)
    assert flat["H"] == got["H"]
