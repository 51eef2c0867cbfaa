"""Points of the BN254 twist E'(Fq2): y^2 = x^3 + 3 / (9 + u) outside G2, for the subgroup-check tests.

#E' = r (2p - r); the cofactor 2p - r is divisible by 10069.  Q is the curve point with x = 5 + 7u (its
order is a multiple of a cofactor factor), T = [(2p - r) r / 10069] Q has order exactly 10069.  The oracle's
g2_mul reduces its scalar mod r, which is only right inside G2: mul_any does not."""
from oracle import bn254

P, R = bn254.P, bn254.R
COFACTOR = 2 * P - R
SMALL = 10069


def f2_sqrt(a):
    """a square root of a in Fq2 = Fq[u] / (u^2 + 1), p = 3 mod 4, or None"""
    if a == (0, 0):
        return a
    a1 = bn254.f2_pow(a, (P - 3) // 4)
    alpha = bn254.f2_mul(bn254.f2_sqr(a1), a)
    x0 = bn254.f2_mul(a1, a)
    if alpha == (P - 1, 0):
        x = bn254.f2_mul((0, 1), x0)
    else:
        b = bn254.f2_pow(bn254.f2_add((1, 0), alpha), (P - 1) // 2)
        x = bn254.f2_mul(b, x0)
    return x if bn254.f2_sqr(x) == a else None


def mul_any(pt, k: int):
    """k * pt on the twist for any k >= 0 (no reduction mod r)"""
    acc, base = bn254.G2J_INF, bn254.g2j_from_affine(pt)
    while k:
        if k & 1:
            acc = bn254.g2j_add(acc, base)
        base = bn254.g2j_double(base)
        k >>= 1
    return bn254.g2j_to_affine(acc)


_cache = {}


def q_point():
    """the twist point with x = 5 + 7u: on the curve, not in G2"""
    if "q" not in _cache:
        x = (5, 7)
        y = f2_sqrt(bn254.f2_add(bn254.f2_mul(bn254.f2_sqr(x), x), bn254.B2))
        assert y is not None, "x = 5 + 7u is not the abscissa of a twist point"
        q = (x, y)
        assert bn254.g2_on_curve(q) and mul_any(q, R) is not None
        _cache["q"] = q
    return _cache["q"]


def t_point():
    """a twist point of order exactly 10069"""
    if "t" not in _cache:
        assert COFACTOR % SMALL == 0
        t = mul_any(q_point(), COFACTOR // SMALL * R)
        assert t is not None and bn254.g2_on_curve(t)
        assert mul_any(t, SMALL) is None and mul_any(t, R) is not None
        _cache["t"] = t
    return _cache["t"]
