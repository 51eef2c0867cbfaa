"""The inputs that the host replay (tests/test_host_ptau_decompress.py) and the GPU test
(tests/test_gpu_ptau_challenge.py) of the square-root and decompression kernels share, with their expected
results from oracle/bn254.py, oracle/mpc.py and the encodings of ptau_model.py."""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ptau_model as pm  # noqa: E402

from oracle import bn254, mpc  # noqa: E402

P = bn254.P


def legendre(a: int) -> int:
    return 0 if a % P == 0 else (1 if pow(a, (P - 1) // 2, P) == 1 else -1)


@functools.lru_cache(maxsize=None)
def fq_elements():
    rnd = random.Random(0x5EED01)
    return tuple([0, 1, P - 1] + list(range(2, 24)) + [rnd.randrange(P) for _ in range(24)])


@functools.lru_cache(maxsize=None)
def fq2_elements():
    rnd = random.Random(0x5EED02)
    res = [a for a in range(2, 40) if legendre(a) == 1][:5]
    non = [a for a in range(2, 40) if legendre(a) == -1][:5]
    out = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1)]
    out += [(a, 0) for a in res + non]  # c1 = 0: the root is real (c0 a residue) or purely imaginary
    out += [(0, a) for a in res + non]  # c0 = 0
    out += [(a, b) for a in (1, 2, 3) for b in (1, 2, 5)]
    out += [(rnd.randrange(P), rnd.randrange(P)) for _ in range(28)]
    out += [(rnd.randrange(P), 0) for _ in range(4)] + [(0, rnd.randrange(P)) for _ in range(4)]
    return tuple(out)


def fq_bytes(a: int) -> bytes:
    return a.to_bytes(32, "little")


def fq2_bytes(a) -> bytes:
    return fq_bytes(a[0]) + fq_bytes(a[1])


def fq_is_square(a: int) -> bool:
    return bn254.fq_sqrt(a) is not None


def fq2_is_square(a) -> bool:
    return mpc.f2_sqrt(a) is not None


def check_roots(fq2: bool, elements, roots: bytes, is_square: bytes):
    """the kernel's (or the replay's) answer against the oracle: the verdict, and the root by squaring"""
    eb = 64 if fq2 else 32
    assert len(roots) == eb * len(elements) and len(is_square) == len(elements)
    yes = no = 0
    for i, a in enumerate(elements):
        raw = roots[i * eb:(i + 1) * eb]
        want = fq2_is_square(a) if fq2 else fq_is_square(a)
        assert bool(is_square[i]) == want, (i, a)
        if not want:
            assert raw == bytes(eb), (i, a)
            no += 1
            continue
        yes += 1
        if fq2:
            r = (int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little"))
            assert r[0] < P and r[1] < P and bn254.f2_sqr(r) == a, (i, a)
            ref = mpc.f2_sqrt(a)
            assert r in (ref, bn254.f2_neg(ref)), (i, a)
        else:
            r = int.from_bytes(raw, "little")
            assert r < P and r * r % P == a, (i, a)
            assert r in (bn254.fq_sqrt(a), (-bn254.fq_sqrt(a)) % P), (i, a)
    # neither verdict goes untested
    assert yes >= 8 and no >= 8, (yes, no)


def neg_point(p, g2):
    if p is None:
        return None
    return (p[0], bn254.f2_neg(p[1])) if g2 else (p[0], (-p[1]) % P)


@functools.lru_cache(maxsize=None)
def points(g2: bool):
    """65 points: multiples of the generator, some negated (so both roots occur), a repeat, three at infinity"""
    base = bn254.FixedBase(bn254.G2_GEN, g2=True) if g2 else bn254.FixedBase(bn254.G1_GEN)
    pts = [base.mul(3 + 7 * j) for j in range(65)]
    for j in range(1, 65, 2):
        pts[j] = neg_point(pts[j - 1] if j % 4 == 1 else pts[j], g2)  # j % 4 == 1: -P right after P
    for j in (2, 31, 64):
        pts[j] = None
    return tuple(pts)


def comp(p, g2):
    return pm.g2_c(p) if g2 else pm.g1_c(p)


def unc(p, g2):
    return mpc.g2_u(p) if g2 else mpc.g1_u(p)


def lem(p, g2):
    return bn254.g2_to_lem(p) if g2 else bn254.g1_to_lem(p)


@functools.lru_cache(maxsize=None)
def non_residue_x(g2: bool):
    """the compressed bytes of an x whose x^3 + b is a non-residue, found by search"""
    x = 1
    while True:
        x += 1
        if g2:
            xx = (x, 1)
            if mpc.f2_sqrt(bn254.f2_add(bn254.f2_mul(bn254.f2_sqr(xx), xx), bn254.B2)) is None:
                return (1).to_bytes(32, "big") + x.to_bytes(32, "big")
        elif bn254.fq_sqrt((x * x * x + 3) % P) is None:
            return x.to_bytes(32, "big")


def bad_compressed(g2: bool):
    """{kind: bytes} of the compressed forms that decompression refuses"""
    tail = bytes(32) if g2 else b""  # G2: x.c0 after x.c1; the flagged coordinate comes first
    kinds = {"x_is_p": P.to_bytes(32, "big") + tail, "inf_with_tail": bytes([0x40]) + bytes(30) + b"\x01" + tail,
             "inf_and_greater": bytes([0xC0]) + bytes(31) + tail, "non_residue": non_residue_x(g2)}
    assert P + 1 < 1 << 254
    kinds["x_is_p_plus_1"] = (P + 1).to_bytes(32, "big") + tail
    if g2:
        kinds["c0_is_p"] = (5).to_bytes(32, "big") + P.to_bytes(32, "big")
        kinds["inf_with_c0"] = bytes([0x40]) + bytes(62) + b"\x01"
    return kinds


def bad_uncompressed(g2: bool):
    """{kind: bytes} of the uncompressed forms that decoding refuses"""
    good = unc(points(g2)[0], g2)
    n = len(good)
    kinds = {"x_is_p": P.to_bytes(32, "big") + good[32:], "y_is_p": good[:n - 32] + P.to_bytes(32, "big"),
             "x_is_p_plus_1": (P + 1).to_bytes(32, "big") + good[32:],
             "inf_with_tail": bytes([0x40]) + bytes(n - 2) + b"\x01", "inf_and_greater": bytes([0xC0]) + bytes(n - 1),
             "top_bit": bytes([good[0] | 0x80]) + good[1:]}
    return kinds
