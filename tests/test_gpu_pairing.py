"""The device Miller loop and the Fq12 reduction kernel (csrc/pairing_kernels.hpp, groth16_verify.hip) on the
GPU through zkp_miller_loop / zkp_fq12_product, against the host pairing (zkp_pairing) and the oracle.

Device Miller values differ from the host's by factors the final exponentiation removes, so every comparison
is made after zkp_final_exponentiation.  Sizes: a partial wave (1, 63), a full wave (64), the wave border (65)
and a third workgroup (130); at lanes 0, 63, 64 and n - 1 sit infinity in P, infinity in Q, the generators and
a repeated pair."""
import json
import os
import random

import pytest

from oracle import bn254
import zkp_amd

pytestmark = pytest.mark.gpu

R = bn254.R
ONE = [[(1, 0), (0, 0), (0, 0)], [(0, 0), (0, 0), (0, 0)]]
FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_fixtures.json")))
VK = FIX["vkey_ts"]


@pytest.fixture(scope="module")
def pool():
    """24 random multiples of each generator with the host pairing of pool pair k (computed once)"""
    rng = random.Random(20240611)
    ps = [bn254.g1_mul(bn254.G1_GEN, rng.randrange(1, R)) for _ in range(24)]
    qs = [bn254.g2_mul(bn254.G2_GEN, rng.randrange(1, R)) for _ in range(24)]
    return ps, qs, {}


def _want(pool, p, q):
    cache = pool[2]
    key = (p, q)
    if key not in cache:
        cache[key] = zkp_amd.pairing(p, q)
    return cache[key]


def _pairs(pool, n):
    ps, qs, _ = pool
    pairs = [(ps[i % 24], qs[(7 * i + i // 24) % 24]) for i in range(n)]
    special = [(None, qs[1]), (ps[1], None), (bn254.G1_GEN, bn254.G2_GEN), (ps[2], qs[2])]
    for k, lane in enumerate((0, 63, 64, n - 1)):
        if 0 <= lane < n:
            pairs[lane] = special[(k + lane) % 4] if n > 1 else special[2]
    if n > 3:
        pairs[2] = pairs[1]  # a repeated pair in neighbouring lanes
    return pairs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_final_exponentiation_of_every_miller_value_is_the_pairing(pool, n):
    pairs = _pairs(pool, n)
    got = zkp_amd.miller_loop(pairs)
    assert len(got) == n
    for i, ((p, q), f) in enumerate(zip(pairs, got)):
        if p is None or q is None:
            assert f == ONE, i  # infinity on either side: exactly 1, before any exponentiation
        assert zkp_amd.final_exponentiation(f) == _want(pool, p, q), i


def test_infinity_everywhere_and_an_empty_batch():
    ps = [(None, None), (None, bn254.G2_GEN), (bn254.G1_GEN, None)]
    assert zkp_amd.miller_loop(ps) == [ONE] * 3
    assert zkp_amd.miller_loop([]) == []


def test_alpha_beta_gives_vk_alphabeta_12():
    a1 = (int(VK["vk_alpha_1"][0]), int(VK["vk_alpha_1"][1]))
    b2 = tuple((int(c[0]), int(c[1])) for c in VK["vk_beta_2"][:2])
    got = zkp_amd.final_exponentiation(zkp_amd.miller_loop([(a1, b2)])[0])
    assert [[[str(x[0]), str(x[1])] for x in c] for c in got] == VK["vk_alphabeta_12"]


def test_bilinearity():
    p, q = bn254.g1_mul(bn254.G1_GEN, 7), bn254.g2_mul(bn254.G2_GEN, 11)
    f = zkp_amd.miller_loop([(bn254.g1_mul(p, 5), bn254.g2_mul(q, 3)), (bn254.g1_mul(p, 15), q)])
    e1, e2 = zkp_amd.final_exponentiation(f[0]), zkp_amd.final_exponentiation(f[1])
    assert e1 == e2 and e1 != ONE


def _f12(t):
    return [[tuple(c) for c in h] for h in t]


def _rand_f12(rng):
    return [[(rng.randrange(bn254.P), rng.randrange(bn254.P)) for _ in range(3)] for _ in range(2)]


def _oracle(f):
    return tuple(tuple(tuple(c) for c in h) for h in f)


# 257 and 300: above one workgroup's share of 256 values; 257 leaves the second workgroup one value
@pytest.mark.parametrize("n", [0, 1, 2, 64, 65, 257, 300])
def test_fq12_product_equals_the_host_product(n):
    rng = random.Random(1000 + n)
    vals = [_rand_f12(rng) for _ in range(n)]
    if n >= 2:
        x = _oracle(vals[0])
        vals[-1] = _f12(bn254.f12_inv(x))  # a pair x, 1/x
    if n >= 64:
        vals[5] = ONE
        vals[63] = ONE
    want = bn254.F12_ONE
    for v in vals:
        want = bn254.f12_mul(want, _oracle(v))
    assert _oracle(zkp_amd.fq12_product(vals)) == want
