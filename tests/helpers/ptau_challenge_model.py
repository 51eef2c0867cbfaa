"""A pure-Python model of `powersoftau export challenge | challenge contribute | import response`
(zkp_ptau_export_challenge, zkp_ptau_challenge_contribute, zkp_ptau_import_response): the third-party path of a
phase-1 ceremony, on the encodings and hashes that ptau_model.py fixes (recalled from snarkjs 0.4.22,
powersoftau_export_challenge.js / powersoftau_challenge_contribute.js / powersoftau_import.js; restated, parity
unpinned).  INSECURE as ptau_model is: tiny powers, Python speed.  N = 2^power.

challenge file  384 N + 128 bytes: the last record's response hash (Blake2b-512 of "" when there is none), then
                sections 2-6 uncompressed.  Its Blake2b-512 is the challenge: the last record's nextChallenge.
response file   192 N + 864 bytes: the challenge hash, sections 2-6 after the contribution compressed, the
                contributor's key (ptau_model.key_bytes).  Its Blake2b-512 is the response hash, and the hasher's
                state just before the key is the record's partialHash.

import_response(f, challenge_contribute(export_challenge(f), rng), name) == ptau_model.contribute(f, rng, name):
the challenge is the same, the key is drawn from rng in the same order, and the partial hash runs over the same
bytes (challenge, then the new sections compressed)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ptau_model as pm  # noqa: E402

from oracle import bn254, mpc  # noqa: E402

P, R = bn254.P, bn254.R
COUNTS = lambda n: ((2, 2 * n - 1), (3, n), (4, n), (5, n), (6, 1))  # noqa: E731


class BadPoint(ValueError):
    pass


# ------------------------------------------------------------------ decoding

def g1_from_u(b: bytes):
    """an uncompressed G1 point (mpc.g1_u); a coordinate >= p or a misused flag byte raises BadPoint"""
    if b[0] & 0x40:
        if b != bytes([0x40]) + bytes(63):
            raise BadPoint("infinity flag with other bits")
        return None
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
    if x >= P or y >= P:
        raise BadPoint("coordinate out of range")
    return (x, y)


def g2_from_u(b: bytes):
    if b[0] & 0x40:
        if b != bytes([0x40]) + bytes(127):
            raise BadPoint("infinity flag with other bits")
        return None
    x1, x0, y1, y0 = (int.from_bytes(b[i:i + 32], "big") for i in range(0, 128, 32))
    if max(x1, x0, y1, y0) >= P:
        raise BadPoint("coordinate out of range")
    return ((x0, x1), (y0, y1))


def g1_decompress(b: bytes):
    """a compressed G1 point (ptau_model.g1_c): y is the root of x^3 + 3 whose "greater" predicate is the 0x80 flag"""
    if b[0] & 0x40:
        if b != bytes([0x40]) + bytes(31):
            raise BadPoint("infinity flag with other bits")
        return None
    x = int.from_bytes(bytes([b[0] & 0x3F]) + b[1:], "big")
    if x >= P:
        raise BadPoint("coordinate out of range")
    y = bn254.fq_sqrt((x * x * x + 3) % P)
    if y is None:
        raise BadPoint("not a point of the curve")
    if mpc._neg_fq(y) != bool(b[0] & 0x80):
        y = (-y) % P
    return (x, y)


def g2_decompress(b: bytes):
    if b[0] & 0x40:
        if b != bytes([0x40]) + bytes(63):
            raise BadPoint("infinity flag with other bits")
        return None
    x1, x0 = int.from_bytes(bytes([b[0] & 0x3F]) + b[1:32], "big"), int.from_bytes(b[32:], "big")
    if x1 >= P or x0 >= P:
        raise BadPoint("coordinate out of range")
    x = (x0, x1)
    y = mpc.f2_sqrt(bn254.f2_add(bn254.f2_mul(bn254.f2_sqr(x), x), bn254.B2))
    if y is None:
        raise BadPoint("not a point of the curve")
    if mpc._neg_fq2(y) != bool(b[0] & 0x80):
        y = bn254.f2_neg(y)
    return (x, y)


def _read_sections(buf: bytes, at: int, n: int, compressed: bool):
    secs = {}
    for sid, count in COUNTS(n):
        g2 = pm._g2(sid)
        pb = (64 if g2 else 32) if compressed else (128 if g2 else 64)
        dec = (g2_decompress if g2 else g1_decompress) if compressed else (g2_from_u if g2 else g1_from_u)
        secs[sid] = [dec(buf[at + i * pb:at + (i + 1) * pb]) for i in range(count)]
        at += count * pb
    return secs, at


def challenge_power(length: int) -> int:
    n, rem = divmod(length - 128, 384)
    if length < 128 or rem or n < 2 or n > 1 << 28 or n & (n - 1):
        raise ValueError("challenge: not 384 * 2^power + 128 bytes with power within 1..28")
    return n.bit_length() - 1


# ------------------------------------------------------------------ the three commands

def export_challenge(ptau: bytes) -> bytes:
    pt = pm.Ptau.read(ptau)
    last = pm.response_hash(pt.contributions[-1]) if pt.contributions else pm.blake2b()
    return last + pm.sections_uncompressed(pt.sections)


def challenge_contribute(challenge: bytes, rng) -> bytes:
    n = 1 << challenge_power(len(challenge))
    s, end = _read_sections(challenge, 64, n, False)
    assert end == len(challenge)
    for sid, pts in s.items():
        on = bn254.g2_on_curve if pm._g2(sid) else bn254.g1_on_curve
        for i, p in enumerate(pts):
            if p is not None and not on(p):
                raise BadPoint("challenge: section %d point %d is not on the curve" % (sid, i))
    h = pm.blake2b(challenge)
    prv, key = pm.draw_key(rng, h)
    tau, alpha, beta = prv["tau"], prv["alpha"], prv["beta"]
    tp = [pow(tau, i, R) for i in range(len(s[2]))]
    new_s = {2: [bn254.g1_mul(p, t) for p, t in zip(s[2], tp)], 3: [bn254.g2_mul(p, t) for p, t in zip(s[3], tp)],
             4: [bn254.g1_mul(p, alpha * t % R) for p, t in zip(s[4], tp)],
             5: [bn254.g1_mul(p, beta * t % R) for p, t in zip(s[5], tp)], 6: [bn254.g2_mul(s[6][0], beta)]}
    return h + pm.sections_compressed(new_s) + pm.key_bytes(key)


def import_response(ptau: bytes, response: bytes, name: str = None) -> bytes:
    pt = pm.Ptau.read(ptau)
    n = 1 << pt.power
    if len(response) != 192 * n + 864:
        raise ValueError("response: size of the contribution is invalid")
    if response[:64] != pm._last_challenge(pt):
        raise ValueError("response: this contribution is not based on the previous hash")
    new_s, end = _read_sections(response, 64, n, True)
    assert end == len(response) - 768
    kb = response[end:]
    key = {}
    for i, k in enumerate(pm.KEYS):
        key[k] = {"g1_s": g1_from_u(kb[128 * i:128 * i + 64]), "g1_sx": g1_from_u(kb[128 * i + 64:128 * i + 128]),
                  "g2_spx": g2_from_u(kb[384 + 128 * i:512 + 128 * i])}
    partial = pm.Blake2b512().update(response[:end])
    c = {"tauG1": new_s[2][1], "tauG2": new_s[3][1], "alphaG1": new_s[4][0], "betaG1": new_s[5][0], "betaG2": new_s[6][0],
         "key": key, "partialHash": partial.export_state(), "type": 0}
    if name is not None:
        c["name"] = name
    assert pm.response_hash(c) == pm.blake2b(response)
    c["nextChallenge"] = pm.blake2b(pm.response_hash(c) + pm.sections_uncompressed(new_s))
    return pm.Ptau(pt.power, pt.ceremony_power, new_s, pt.contributions + [c]).write()
