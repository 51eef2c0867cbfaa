"""TEST INFRASTRUCTURE -- the `MPCParams` file of `snarkjs zkey export bellman | bellman contribute | import
bellman` (csrc/zkey_bellman.hpp), restated on oracle.bn254 / oracle.mpc / oracle.setup independently of the
library: the layout, the H points from known toxic values, the import's change of basis by its defining sum, and
the relaxed H rule of `zkey verify`.  Recalled from snarkjs 0.4.22 (zkey_export_bellman.js, zkey_bellman_
contribute.js, zkey_import_bellman.js); parity unpinned: no snarkjs-written MPCParams file exists here.

Layout (every integer a big-endian u32, every point oracle.mpc.g1_u / g2_u):
  alpha1 beta1 beta2 gamma2 delta1 delta2 | u32 nPublic+1, IC | u32 n-1, B | u32 nVars-nPublic-1, L | u32 nVars, A |
  u32 nVars, B1 | u32 nVars, B2 | csHash | u32 nContributions, per contribution deltaAfter g1_s g1_sx g2_spx transcript
Up to csHash this is what oracle.mpc.cs_hash hashes.

n = 2^p the key's domain, w = ROOTS[p], w2 = ROOTS[p+1], H_j = delta^-1 L^(2n)_(2j+1)(tau) G1 (oracle/setup.py):
  B_i  = delta^-1 tau^i (tau^n - 1) G1 = -2 w2^i sum_j w^(ij) H_j                  i < n - 1
  H'_j = n^-1 sum_i w^(-ij) (-1/2 w2^-i) B_i        with B_(n-1) := infinity
H' differs from H by a multiple of (w^j)_j, so sum_j w^(-j) H'_j = infinity.

The relaxed verify rule: the H combination uses coefficients r_0..r_(n-2) and r'_(n-1) = -w sum_(j<n-1) r_j w^j,
for which sum_j r_j w^j = 0."""
import struct

from oracle import bn254, mpc, setup

R = bn254.R
G1B = bn254.FixedBase(bn254.G1_GEN)
HEADER = 576
CONTRIBUTION = 384


def u32be(n):
    return struct.pack(">I", n)


def bellman_h(tau, n, delta):
    """B_0..B_(n-2) from the toxic values"""
    k = (pow(tau, n, R) - 1) * bn254.inv(delta, R) % R
    return [G1B.mul(pow(tau, i, R) * k % R) for i in range(n - 1)]


def contribution_bytes(c):
    return mpc.g1_u(c["deltaAfter"]) + mpc.g1_u(c["g1_s"]) + mpc.g1_u(c["g1_sx"]) + mpc.g2_u(c["g2_spx"]) + c["transcript"]


def body_bytes(z, b_points):
    """the file up to but not including csHash: the bytes csHash is the Blake2b-512 of (for a new key)"""
    out = [mpc.g1_u(z.alpha1), mpc.g1_u(z.beta1), mpc.g2_u(z.beta2), mpc.g2_u(z.gamma2), mpc.g1_u(z.delta1),
           mpc.g2_u(z.delta2)]
    for sec in (z.ic, b_points, z.c, z.a, z.b1):
        out.append(u32be(len(sec)))
        out += [mpc.g1_u(p) for p in sec]
    out.append(u32be(len(z.b2)))
    out += [mpc.g2_u(p) for p in z.b2]
    return b"".join(out)


def file_bytes(z, b_points):
    """the MPCParams file of key z (an oracle ZKey with extra["mpc"]) whose H section is b_points"""
    m = z.extra["mpc"]
    return body_bytes(z, b_points) + m["cs_hash"] + u32be(len(m["contributions"])) + \
        b"".join(contribution_bytes(c) for c in m["contributions"])


def export_model(z, tau, delta):
    return file_bytes(z, bellman_h(tau, z.domain_size, delta))


def _g1(b):
    if b[0] & 0x40:
        assert b == bytes([0x40]) + bytes(63)
        return None
    return (int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))


def _g2(b):
    if b[0] & 0x40:
        assert b == bytes([0x40]) + bytes(127)
        return None
    v = [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(4)]
    return ((v[1], v[0]), (v[3], v[2]))


def parse(data):
    """-> dict: the header points, the sections as point lists, cs_hash, contributions, and `at`: the byte offset
    of each part (the first point of a section; "cs_hash"; "contributions": its count)"""
    o = 0
    out, at = {}, {}
    for name, g2 in (("alpha1", 0), ("beta1", 0), ("beta2", 1), ("gamma2", 1), ("delta1", 0), ("delta2", 1)):
        pb = 128 if g2 else 64
        at[name] = o
        out[name] = (_g2 if g2 else _g1)(data[o:o + pb])
        o += pb
    for name, g2 in (("ic", 0), ("h", 0), ("l", 0), ("a", 0), ("b1", 0), ("b2", 1)):
        pb = 128 if g2 else 64
        (n,) = struct.unpack_from(">I", data, o)
        o += 4
        at[name] = o
        out[name] = [(_g2 if g2 else _g1)(data[o + pb * i:o + pb * (i + 1)]) for i in range(n)]
        o += pb * n
    at["cs_hash"] = o
    out["cs_hash"] = data[o:o + 64]
    o += 64
    (n,) = struct.unpack_from(">I", data, o)
    at["contributions"] = o
    o += 4
    out["contributions"] = []
    for _ in range(n):
        b = data[o:o + CONTRIBUTION]
        out["contributions"].append({"deltaAfter": _g1(b[:64]), "g1_s": _g1(b[64:128]), "g1_sx": _g1(b[128:192]),
                                     "g2_spx": _g2(b[192:320]), "transcript": b[320:384]})
        o += CONTRIBUTION
    assert o == len(data)
    out["at"] = at
    return out


def h_from_b(b_points, n):
    """H'_j by the defining sum (O(n^2) scalar multiplications: n = 16 only)"""
    assert len(b_points) == n - 1
    p = n.bit_length() - 1
    w, w2 = setup.ROOTS[p], setup.ROOTS[p + 1]
    ninv, mhalf = bn254.inv(n, R), (-bn254.inv(2, R)) % R
    w2inv, winv = bn254.inv(w2, R), bn254.inv(w, R)
    out = []
    for j in range(n):
        acc = None
        for i, b in enumerate(b_points):
            if b is not None:
                k = ninv * mhalf % R * pow(w2inv, i, R) % R * pow(winv, i * j, R) % R
                acc = bn254.g1_add(acc, bn254.g1_mul(b, k))
        out.append(acc)
    return out


def w_direction_sum(h_points):
    """sum_j w^(-j) H_j: infinity (None) for every section an import writes"""
    n = len(h_points)
    winv = bn254.inv(setup.ROOTS[n.bit_length() - 1], R)
    acc = None
    for j, h in enumerate(h_points):
        if h is not None:
            acc = bn254.g1_add(acc, bn254.g1_mul(h, pow(winv, j, R)))
    return acc


def relaxed_h_coefficients(r):
    """the verifier's H coefficients from the stream's r_0..r_(n-1): the last one replaced"""
    n = len(r)
    w = setup.ROOTS[n.bit_length() - 1]
    s = sum(r[j] * pow(w, j, R) for j in range(n - 1)) % R
    out = list(r[:n - 1]) + [(-w * s) % R]
    assert sum(out[j] * pow(w, j, R) for j in range(n)) % R == 0
    return out


def relaxed_h_check(old_h, new_h, r, delta2_key, delta2_init):
    """e(sum r'_j old_j, delta2_key) == e(sum r'_j new_j, delta2_init) under the relaxed coefficients"""
    co = relaxed_h_coefficients(r)
    return mpc.same_ratio(mpc._lincomb_g1(old_h, co), mpc._lincomb_g1(new_h, co), delta2_key, delta2_init)
