"""`zkey verify` on the GPU (zkp_zkey_verify_frominit / zkp_zkey_verify; reference gate
circuit/scripts/generate_keys_phase2_groth16.sh:26) against the oracle's restatement
(oracle/mpc.py zkey_verify): every key of a GPU ceremony is accepted, every class of tampering the
oracle catches is caught with the oracle's message, and the device parts are pinned on their own:
the coefficient stream against the oracle's ChaCha, the point check, and the paired linear
combination against oracle.mpc._lincomb_g1 with the same coefficients."""
import copy
import json
import os
import subprocess
import sys

import pytest

from oracle import binfile, bn254, circuit, mpc
from oracle.beacon import ChaCha
from test_setup_new import TAU as _SETUP_TAU, _case as _setup_case
import zkp_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "zkey_verify_child.py")
TAU, ALPHA, BETA = 0x1234567890ABCDEF1122334455667788 % bn254.R, 987654321987654321, 555555555555
BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20")
RAND64 = bytes(range(7, 71))
SIZES = {"tiny": (12, 10, 2, 11), "small": (200, 230, 26, 21)}
SEED = bytes(range(100, 132))
SEED_B = bytes(range(3, 35))
L_MSG = "INVALID: L section is not the initial one times delta^-1"
H_MSG = "INVALID: H section is not the initial one times delta^-1"
P = bn254.P
assert _SETUP_TAU == TAU
_cache = {}


def _inputs(name, seed=None):
    """(r1cs bytes, ptau bytes); the known-tau ptau (seconds of oracle time for small) is the one
    tests/test_setup_new.py builds for the same circuit, computed once per session"""
    r1cs, _, n, _, ptau, _ = _setup_case(name)
    assert (r1cs.n_vars, r1cs.n_constraints, r1cs.n_public) == SIZES[name][:3]
    if seed is not None:  # another circuit of the same shape: the same ptau serves it
        r1cs, _ = circuit.gen_circuit(*(SIZES[name][:3] + (seed,)))
        assert circuit.domain_size_for(r1cs.n_constraints, r1cs.n_public) == n
    return binfile.write_r1cs(r1cs), ptau


def _chain(name):
    """The ceremony of tests/test_setup_mpc.py:_chain (same circuit, ptau and entropy) through the C ABI:
    (r1cs bytes, ptau bytes, k0, k1, k2)."""
    if name not in _cache:
        r1cs, ptau = _inputs(name)
        k0 = zkp_amd.zkey_new(r1cs, ptau)
        k1 = zkp_amd.zkey_contribute_entropy(k0, "some entropy text", rand64=RAND64, name="first contribution")
        k2 = zkp_amd.zkey_beacon(k1, BEACON, 10, name="Final Beacon phase2")
        _cache[name] = (r1cs, ptau, k0, k1, k2)
    return _cache[name]


def _sizes(name):
    nv, _, npub, _ = SIZES[name]
    z = binfile.read_zkey(_chain(name)[2])
    assert len(z.c) == nv - npub - 1
    return len(z.c), len(z.h)


def test_section_sizes_are_the_ones_the_cases_assume():
    assert _sizes("tiny") == (9, 16) and _sizes("small") == (173, 512)


# ------------------------------------------------------------------ accept

def test_accepts_every_key_of_the_tiny_ceremony():
    _, _, k0, k1, k2 = _chain("tiny")
    for k in (k0, k1, k2):
        got = zkp_amd.zkey_verify_frominit(k0, k, seed=SEED)
        assert got == (True, "OK") and got == mpc.zkey_verify(k, k0)


def test_accepts_every_key_of_the_small_ceremony():
    r1cs, ptau, k0, k1, k2 = _chain("small")
    for k in (k0, k1, k2):
        assert zkp_amd.zkey_verify_frominit(k0, k, seed=SEED) == (True, "OK")
    assert mpc.zkey_verify(k2, k0) == (True, "OK")
    assert zkp_amd.zkey_verify_frominit(k0, k2, seed=SEED_B) == (True, "OK")  # other coefficients agree
    assert zkp_amd.zkey_verify_frominit(k0, k2) == (True, "OK")  # production: seeded by the OS


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_verify_from_r1cs_and_ptau(name):
    r1cs, ptau, _, _, k2 = _chain(name)
    assert zkp_amd.zkey_verify(r1cs, ptau, k2, seed=SEED) == (True, "OK")
    assert zkp_amd.zkey_verify(r1cs, ptau, k2, seed=SEED_B) == (True, "OK")
    t = zkp_amd.zkey_verify_timings()
    assert t["chunks"] == 2 and t["total"] > 0


# ------------------------------------------------------------------ reject (tiny)

def _z2():
    return copy.deepcopy(binfile.read_zkey(_chain("tiny")[4]))


def _swap_l():
    z = _z2()
    z.c[0], z.c[-1] = z.c[-1], z.c[0]
    return binfile.write_zkey(z)


def _double_last_h():
    z = _z2()
    z.h[-1] = bn254.g1_mul(z.h[-1], 2)
    return binfile.write_zkey(z)


def _swap_a():
    z = _z2()
    j = next(j for j in range(1, len(z.a)) if z.a[j] != z.a[0])
    z.a[0], z.a[j] = z.a[j], z.a[0]
    return binfile.write_zkey(z)


def _double_g1_sx():
    z = _z2()
    c = z.extra["mpc"]["contributions"][-1]
    c["g1_sx"] = bn254.g1_mul(c["g1_sx"], 2)
    return binfile.write_zkey(z)


def _fewer_iterations():
    z = _z2()
    c = z.extra["mpc"]["contributions"][-1]
    assert c["numIterationsExp"] == 10
    c["numIterationsExp"] = 9
    return binfile.write_zkey(z)


def _no_record():
    return zkp_amd.zkey_contribute(_chain("tiny")[4], 12345)


def _double_delta2():
    z = _z2()
    z.delta2 = bn254.g2_mul(z.delta2, 2)
    return binfile.write_zkey(z)


TAMPERED = {
    "L first and last swapped": (_swap_l, L_MSG),
    "last H doubled": (_double_last_h, H_MSG),
    "two A swapped": (_swap_a, "INVALID: section 5 is not identical to the initial key's"),
    "g1_sx doubled": (_double_g1_sx, "INVALID(1): inconsistent transcript"),
    "numIterationsExp 9": (_fewer_iterations, "INVALID(1): does not match the beacon"),
    "contribute without a record": (_no_record, "INVALID: delta1 is not the last deltaAfter"),
    "delta2 doubled": (_double_delta2, "INVALID: delta2"),
}


@pytest.mark.parametrize("case", sorted(TAMPERED))
def test_rejects_with_the_oracles_message(case):
    make, text = TAMPERED[case]
    k0 = _chain("tiny")[2]
    bad = make()
    want = mpc.zkey_verify(bad, k0)
    assert want == (False, text)
    assert zkp_amd.zkey_verify_frominit(k0, bad, seed=SEED) == want


def test_rejects_another_circuits_initial_key():
    k2 = _chain("tiny")[4]
    other = zkp_amd.zkey_new(*_inputs("tiny", seed=99))
    want = mpc.zkey_verify(k2, other)
    assert want == (False, "INVALID: circuit does not match (csHash)")
    assert zkp_amd.zkey_verify_frominit(other, k2, seed=SEED) == want


def _section(buf, sid):
    _, secs = binfile.read_binfile(buf, b"zkey", 1)
    return secs[sid][0]


def test_rejects_an_l_point_off_the_curve_with_its_index():
    k0, k2 = _chain("tiny")[2], _chain("tiny")[4]
    z = binfile.read_zkey(k2)
    off, _ = _section(k2, 8)
    for idx in (3, 8, 0):
        x, y = z.c[idx]
        bad = bytearray(k2)
        bad[off + 64 * idx:off + 64 * idx + 64] = bn254.g1_to_lem((x, (y + 1) % P))
        assert zkp_amd.zkey_verify_frominit(k0, bytes(bad), seed=SEED) == \
            (False, "INVALID: L section point %d is not on the curve" % idx)
    # two bad points: the smallest index is reported
    bad = bytearray(k2)
    for idx in (6, 2):
        x, y = z.c[idx]
        bad[off + 64 * idx:off + 64 * idx + 64] = bn254.g1_to_lem((x, (y + 1) % P))
    assert zkp_amd.zkey_verify_frominit(k0, bytes(bad), seed=SEED) == \
        (False, "INVALID: L section point 2 is not on the curve")


def test_rejects_a_non_canonical_h_coordinate():
    """x stored as x + p names the same residue and fits in 256 bits: the arithmetic would accept it."""
    k0, k2 = _chain("tiny")[2], _chain("tiny")[4]
    off, _ = _section(k2, 9)
    idx = 5
    bad = bytearray(k2)
    x = int.from_bytes(bad[off + 64 * idx:off + 64 * idx + 32], "little")
    assert 0 < x < P
    bad[off + 64 * idx:off + 64 * idx + 32] = (x + P).to_bytes(32, "little")
    assert zkp_amd.zkey_verify_frominit(k0, bytes(bad), seed=SEED) == \
        (False, "INVALID: H section point %d is not on the curve" % idx)


# ------------------------------------------------------------------ chunk boundaries (small)

def _doubled(key, sid, idx):
    off, _ = _section(key, sid)
    pt = bn254.g1_from_lem(key[off + 64 * idx:off + 64 * idx + 64])
    bad = bytearray(key)
    bad[off + 64 * idx:off + 64 * idx + 64] = bn254.g1_to_lem(bn254.g1_mul(pt, 2))
    return bytes(bad)


def _child(tmp_path, chunk, init, keys):
    (tmp_path / "init.zkey").write_bytes(init)
    paths = []
    for i, k in enumerate(keys):
        paths.append(str(tmp_path / ("k%d.zkey" % i)))
        open(paths[-1], "wb").write(k)
    env = dict(os.environ, ZKP_VERIFY_CHUNK=chunk)
    r = subprocess.run([sys.executable, CHILD, str(tmp_path / "init.zkey"), SEED.hex()] + paths, capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_chunk_boundaries(tmp_path):
    """ZKP_VERIFY_CHUNK=64 on small: L (173) is two full chunks and a ragged 45, H (512) eight exact
    chunks; a doubled point in the first, at both sides of a boundary and in the last chunk is caught in
    the right section, and the verdicts are those of the default chunk size (one chunk per section)."""
    _, _, k0, _, k2 = _chain("small")
    cases = [(k2, (True, "OK"))]
    cases += [(_doubled(k2, 8, i), (False, L_MSG)) for i in (0, 63, 64, 172)]
    cases += [(_doubled(k2, 9, 511), (False, H_MSG))]
    assert mpc.zkey_verify(cases[3][0], k0) == (False, L_MSG)
    got = _child(tmp_path, "64", k0, [k for k, _ in cases])
    assert [tuple(g) for g in got] == [w for _, w in cases]
    assert [zkp_amd.zkey_verify_frominit(k0, k, seed=SEED) for k, _ in cases] == [w for _, w in cases]


@pytest.mark.parametrize("value", ["0", "abc", "-4", "64x", ""])
def test_malformed_chunk_size_is_an_invalid_argument(tmp_path, value):
    _, _, k0, _, k2 = _chain("tiny")
    assert _child(tmp_path, value, k0, [k2]) == [{"status": 1}]


# ------------------------------------------------------------------ zkp_rlc_coeffs

def _coeffs(seed, first, n):
    rng = ChaCha(mpc.seed_words(seed))
    words = [rng.next_u32() for _ in range(4 * (first + n))]
    return [sum(words[4 * i + j] << (32 * j) for j in range(4)) for i in range(first, first + n)]


@pytest.mark.parametrize("first", [0, 1, 6])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_rlc_coeffs_are_the_chacha_stream(n, first):
    assert zkp_amd.rlc_coeffs(SEED, first, n) == _coeffs(SEED, first, n)


def test_rlc_coeffs_depend_on_the_seed_and_handle_zero():
    assert zkp_amd.rlc_coeffs(SEED, 0, 0) == []
    assert zkp_amd.rlc_coeffs(SEED_B, 2, 9) == _coeffs(SEED_B, 2, 9) != _coeffs(SEED, 2, 9)


# ------------------------------------------------------------------ zkp_points_check

def _multiples(n):
    """G, 2G, ..., nG"""
    pts, acc = [], None
    for _ in range(n):
        acc = bn254.g1_add(acc, bn254.G1_GEN)
        pts.append(acc)
    return pts


def _lem(pts):
    return b"".join(bn254.g1_to_lem(p) for p in pts)


def _off_curve(pt):
    return (pt[0], (pt[1] + 1) % P)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_points_check_g1(n):
    pts = _multiples(n)
    if n > 1:
        pts[n // 2] = None  # infinity is a valid point
    assert zkp_amd.points_check(_lem(pts)) == (0, None)
    assert zkp_amd.points_check(_lem([None] * n)) == (0, None)
    for where in ([0], [n - 1], sorted({n - 1, n // 3})):
        bad = list(pts)
        for i in where:
            bad[i] = _off_curve(_multiples(1)[0] if bad[i] is None else bad[i])
        assert zkp_amd.points_check(_lem(bad)) == (len(where), where[0])
    # a coordinate stored as x + p is not canonical
    raw = bytearray(_lem(pts))
    at = 64 * (n - 1)
    raw[at:at + 32] = (int.from_bytes(raw[at:at + 32], "little") + P).to_bytes(32, "little")
    assert zkp_amd.points_check(bytes(raw)) == (1, n - 1)


def test_points_check_g2():
    pts = [bn254.g2_mul(bn254.G2_GEN, k) for k in (1, 2, 5)] + [None]
    raw = b"".join(bn254.g2_to_lem(p) for p in pts)
    assert zkp_amd.points_check(raw, g2=True) == (0, None)
    (x, (y0, y1)) = pts[2]
    bad = raw[:256] + bn254.g2_to_lem((x, ((y0 + 1) % P, y1))) + raw[384:]
    assert zkp_amd.points_check(bad, g2=True) == (1, 2)


# ------------------------------------------------------------------ zkp_rlc_g1

@pytest.mark.parametrize("n,first", [(1, 0), (63, 0), (63, 5), (257, 0)])
def test_rlc_g1_matches_the_oracle(n, first):
    """Set a: distinct points with an infinity, a repeated point and a pair P, -P.  Set b: only P, -P, Q
    and infinity, so equal points meet in one bucket (the doubling case of the mixed addition) and
    opposite ones cancel."""
    a = _multiples(n)
    if n >= 8:
        a[1] = None
        a[4] = a[0]
        a[6] = bn254.g1_neg(a[5])
    p, q = bn254.g1_mul(bn254.G1_GEN, 77), bn254.g1_mul(bn254.G1_GEN, 1234567)
    cycle = [p, p, bn254.g1_neg(p), None, q]
    b = [cycle[i % 5] for i in range(n)]
    co = _coeffs(SEED, first, n)
    got_a, got_b = zkp_amd.rlc_g1(SEED, first, _lem(a), _lem(b))
    assert got_a == mpc._lincomb_g1(a, co)
    assert got_b == mpc._lincomb_g1(b, co)


def test_rlc_g1_of_infinities_is_infinity_and_bad_points_are_refused():
    assert zkp_amd.rlc_g1(SEED, 0, bytes(64 * 5), bytes(64 * 5)) == (None, None)
    pts = _multiples(4)
    bad = list(pts)
    bad[2] = _off_curve(bad[2])
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.rlc_g1(SEED, 0, _lem(pts), _lem(bad))
    assert e.value.status == 1 and "point 2 of set b" in e.value.message
