"""`snarkjs powersoftau prepare phase2` on the GPU (zkp_ptau_prepare_phase2, csrc/ptau_prepare.hip): the
Lagrange sections 12-15 of a ptau by group inverse FFTs.

The oracle's prepared ptau (setup.ptau_known_tau) computes its Lagrange points from the closed form
L_c(tau) with the toxic waste; the GPU computes them from the tau powers alone, so a byte-identical file
checks the transform, the 1/n factor, the level layout and the copied sections together."""
import json
import os
import struct

import pytest

from oracle import binfile, bn254, circuit, groth16, mpc, setup
import zkp_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
R = bn254.R
TAU, ALPHA, BETA = 0x1234567890ABCDEF1122334455667788 % groth16.R, 987654321987654321, 555555555555
G1B = bn254.FixedBase(bn254.G1_GEN)
G2B = bn254.FixedBase(bn254.G2_GEN, g2=True)
BASE = {False: G1B, True: G2B}
_cache = {}


def _oracle_ptau(power):
    if power not in _cache:
        _cache[power] = setup.ptau_known_tau(power, TAU, ALPHA, BETA)
    return _cache[power]


def _sections(buf, magic=b"ptau"):
    _, secs = binfile.read_binfile(buf, magic, 1)
    return {sid: bytes(buf[v[0][0]:v[0][0] + v[0][1]]) for sid, v in secs.items()}


def _stripped(secs, extra=()):
    return binfile.write_binfile(b"ptau", 1, [(sid, secs[sid]) for sid in range(1, 8)] + list(extra))


def _first_difference(got, want):
    """'section <id> point <i>' of the first differing point, or None"""
    for sid in sorted(want):
        if got.get(sid) == want[sid]:
            continue
        if sid not in got or len(got[sid]) != len(want[sid]):
            return "section %d: %s bytes, expected %d" % (sid, len(got[sid]) if sid in got else "no", len(want[sid]))
        pb = {3: 128, 13: 128}.get(sid, 64)
        if sid in (1, 6, 7):
            return "section %d" % sid
        i = next(i for i in range(len(want[sid]) // pb) if got[sid][i * pb:(i + 1) * pb] != want[sid][i * pb:(i + 1) * pb])
        return "section %d point %d" % (sid, i)
    return None


@pytest.mark.parametrize("power", [1, 2, 5, 7])
def test_prepared_file_is_the_oracles(power):
    want = _oracle_ptau(power)
    ws = _sections(want)
    out = zkp_amd.ptau_prepare_phase2(_stripped(ws))
    assert _first_difference(_sections(out), ws) is None
    assert out == want
    # sections 12-15 of the input are ignored and rebuilt
    junk = [(sid, bytes((7 * i + sid) & 0xFF for i in range(len(ws[sid])))) for sid in (12, 13, 14, 15)]
    assert zkp_amd.ptau_prepare_phase2(_stripped(ws, junk)) == want
    t = zkp_amd.ptau_prepare_timings()
    assert t["total"] > 0 and t["launches"] == 2  # every level fits one workgroup: one launch per curve


def test_levels_beyond_one_workgroup():
    """P = 13.  A workgroup transforms 2^9 G1 or 2^8 G2 points in LDS (gfft_kernels.hpp Geom), so the smallest
    power whose top level takes two global stages is 11 for G1 (10 for G2); the floor of 13 decides.  At 13
    the top level runs 4 global stages in G1 and 5 in G2, and levels 10..13 (9..13) each take the tiled path
    with another stage count.  The synthetic file's Lagrange points come from the closed form on the device,
    not from an iFFT."""
    from zkp_amd import synth
    P = 13
    full = synth.ptau(P, 0xC0FFEE, device=0).bytes()
    ws = _sections(full)
    out = zkp_amd.ptau_prepare_phase2(_stripped(ws))
    assert _first_difference(_sections(out), {sid: ws[sid] for sid in (12, 13, 14, 15)}) is None
    assert _first_difference(_sections(out), {sid: ws[sid] for sid in range(1, 8)}) is None
    t = zkp_amd.ptau_prepare_timings()
    # G1: levels 10..13 take 2 + (p - 9) launches, the rest one; G2: levels 9..13 take 2 + (p - 8)
    assert t["launches"] == sum(2 + p - 9 for p in range(10, 14)) + 1 + sum(2 + p - 8 for p in range(9, 14)) + 1


def _enc(pts, g2):
    return b"".join((bn254.g2_to_lem if g2 else bn254.g1_to_lem)(p) for p in pts)


def _ifft(pts, log_n, g2):
    return zkp_amd.group_ifft(_enc(pts, g2), log_n, g2=g2)


@pytest.mark.parametrize("g2,log_n", [(False, 4), (True, 2)])
def test_group_ifft_constant_vector(g2, log_n):
    P = BASE[g2].mul(77)
    n = 1 << log_n
    assert _ifft([P] * n, log_n, g2) == _enc([P] + [None] * (n - 1), g2)


@pytest.mark.parametrize("g2", [False, True])
def test_group_ifft_tau_inside_the_domain(g2):
    # lagrange_at raises "tau in domain" here: L_c(w^3) is 1 at c = 3 and 0 elsewhere
    t = pow(setup.ROOTS[3], 3, R)
    pts = [BASE[g2].mul(pow(t, j, R)) for j in range(8)]
    assert _ifft(pts, 3, g2) == _enc([BASE[g2].mul(1) if c == 3 else None for c in range(8)], g2)


@pytest.mark.parametrize("g2", [False, True])
def test_group_ifft_one_finite_point(g2):
    P = BASE[g2].mul(123456789)
    mul = bn254.g2_mul if g2 else bn254.g1_mul
    w, ninv = setup.ROOTS[3], bn254.inv(8, R)
    want = [mul(P, ninv * pow(w, (-5 * c) % 8, R) % R) for c in range(8)]
    assert _ifft([P if j == 5 else None for j in range(8)], 3, g2) == _enc(want, g2)


@pytest.mark.parametrize("g2,log_n", [(False, 3), (True, 2), (False, 0)])
def test_group_ifft_all_infinity(g2, log_n):
    n = 1 << log_n
    assert _ifft([None] * n, log_n, g2) == _enc([None] * n, g2)


def test_prepare_then_zkey_new_then_prove():
    m = json.load(open(os.path.join(GOLD, "manifest.json")))["circuits"]["tiny"]
    r1cs, w = circuit.gen_circuit(m["n_vars"], m["n_constraints"], m["n_public"], m["circuit_seed"])
    k = circuit.domain_size_for(r1cs.n_constraints, r1cs.n_public).bit_length() - 1
    z = setup.zkey_new(r1cs, TAU, ALPHA, BETA)
    z.extra["mpc"] = {"cs_hash": mpc.cs_hash(z, TAU), "contributions": []}  # section 10 of a new key
    prepared = zkp_amd.ptau_prepare_phase2(_stripped(_sections(_oracle_ptau(k + 1))))
    out = zkp_amd.zkey_new(binfile.write_r1cs(r1cs), prepared)
    want = binfile.write_zkey(z)
    if out != want:  # name the first differing section
        got, exp = _sections(out, b"zkey"), _sections(want, b"zkey")
        assert [s for s in exp if got.get(s) != exp[s]] == []
    assert out == want
    (a, b, c), pub = zkp_amd.Prover(out).prove_raw(binfile.write_wtns(w))
    assert groth16.verify_with_zkey(z, pub, {"A": a, "B": b, "C": c})


def test_errors():
    ws = _sections(_oracle_ptau(5))

    def fails(secs, magic=b"ptau"):
        buf = binfile.write_binfile(magic, 1, [(sid, secs[sid]) for sid in range(1, 8) if sid in secs])
        with pytest.raises(zkp_amd.ZkpError) as e:
            zkp_amd.ptau_prepare_phase2(buf)
        return e.value.status, e.value.message

    def swap(sid, payload):
        return {k: (payload if k == sid else v) for k, v in ws.items()}

    st, msg = fails({sid: v for sid, v in ws.items() if sid != 4})
    assert st == 3 and "section 4" in msg
    st, msg = fails(swap(3, ws[3][:-128]))
    assert st == 3 and "section 3" in msg
    st, msg = fails(swap(1, ws[1][:4] + bn254.int_to_le(R) + ws[1][36:]))
    assert st == 5
    x = int.from_bytes(ws[2][9 * 64:9 * 64 + 32], "little") + 1
    bad2 = ws[2][:9 * 64] + x.to_bytes(32, "little") + ws[2][9 * 64 + 32:]
    st, msg = fails(swap(2, bad2))
    assert st == 3 and "section 2 point 9" in msg, msg
    st, msg = fails(ws, magic=b"xxxx")
    assert st == 3
