"""GPU parity of the bucket reduction by row and column sums (k_rowcol_chain, k_rowcol_tree, the second
level over the 2G sub-groups, msm_fold) through zkp_amd.msm_g1 / msm_g2 against the oracle, bit-exact.

Window widths with U < V (c = 8, 16: c - 1 odd) and U = V (9, 13), columns of a single partial (c = 8:
U = 8), with one, two and all base-table rows (32, 16 ... 1 bucket groups); c = 20 and 22 for the rows of
128 partials (a whole wave per sum) and the chains longer than the default (V = 2048).  The weight
corners of tests/test_host_bucket_reduction.py sit in MSMs of 2^10 and 2^11 points: each alone among
zero scalars (one occupied bucket per window), all together among uniform scalars, and one scalar whose
every window lands in the last bucket."""
import pytest

from oracle import bn254, circuit, groth16
import zkp_amd

pytestmark = pytest.mark.gpu
R = bn254.R
NB = 16  # distinct bases: point i of an MSM is base i % NB, so the oracle multiplies NB points

rng = circuit.SplitMix64(29, 0)
G1B = bn254.FixedBase(bn254.G1_GEN)
K = [rng.fr() or 1 for _ in range(NB)]
BASES = {"g1": [G1B.mul(k) for k in K], "g2": [bn254.g2_mul(bn254.G2_GEN, k) for k in K]}
ENC = {"g1": bn254.g1_to_lem, "g2": bn254.g2_to_lem}
ORACLE = {"g1": groth16.msm_g1, "g2": groth16.msm_g2}
GPU = {"g1": zkp_amd.msm_g1, "g2": zkp_amd.msm_g2}
_POINTS = {}


def _points(curve, n):
    if (curve, n) not in _POINTS:
        enc = [ENC[curve](p) for p in BASES[curve]]
        _POINTS[curve, n] = b"".join(enc[i % NB] for i in range(n))
    return _POINTS[curve, n]


def _check(curve, sc, c, d):
    """MSM of len(sc) points (base i % NB) on the GPU against the oracle over the NB summed scalars."""
    acc = [0] * NB
    for i, x in enumerate(sc):
        acc[i % NB] = (acc[i % NB] + x) % R
    got = GPU[curve](_points(curve, len(sc)), b"".join(bn254.int_to_le(x) for x in sc), window_bits=c, table_depth=d)
    assert got == ORACLE[curve](BASES[curve], acc)


def corner_weights(c):
    H = 1 << (c - 1)
    V = 1 << (c // 2)
    w = [1, V - 1, V, V + 1, H - V, H - 1, H]
    return w + [R - x for x in w]


def all_windows_top(c):
    # windows 0 .. W - 2: the top window of a scalar below r has no room for H
    W = (255 + c - 1) // c
    return sum((1 << (c - 1)) << (c * w) for w in range(W - 1))


CASES = [(c, d) for c in (8, 9, 13, 16) for d in (1, 2, 32)]  # depth 32 >= W: every row, one bucket group


@pytest.mark.parametrize("c,d", CASES)
@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_weight_corners(curve, c, d):
    ws = corner_weights(c)
    for j, w in enumerate(ws):  # alone
        sc = [0] * 1024
        sc[(67 * j + 5) % 1024] = w
        _check(curve, sc, c, d)
    r = circuit.SplitMix64(1000 * c + d, 0)  # together, among uniform scalars
    sc = [r.fr() for _ in range(2048)]
    for j, w in enumerate(ws):
        sc[(131 * j + 7) % 2048] = w
    _check(curve, sc, c, d)
    sc = [0] * 1024  # every window in the last bucket
    sc[333] = all_windows_top(c)
    _check(curve, sc, c, d)


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_uniform_4096(curve):
    r = circuit.SplitMix64(4096, 0)
    _check(curve, [r.fr() for _ in range(4096)], 0, 0)


@pytest.mark.parametrize("curve,c", [("g1", 20), ("g1", 22), ("g2", 20)])
def test_wide_rows(curve, c):
    r = circuit.SplitMix64(c, 0)
    sc = [r.fr() for _ in range(1024)]
    for j, w in enumerate(corner_weights(c)):
        sc[(67 * j + 5) % 1024] = w
    _check(curve, sc, c, 32)
