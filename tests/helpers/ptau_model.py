"""A pure-Python model of the phase-1 ceremony file that `powersoftau verify` reads (zkp_ptau_verify): the
file this project fixes the recalled snarkjs 0.4.22 formats with (powersoftau_utils.js,
powersoftau_verify.js; restated, parity unpinned: no snarkjs-written ptau exists here).

new / contribute / beacon make fixtures (INSECURE: tiny powers, Python speed); verify restates the checks of
zkp_ptau_verify in its order and with its messages.

Section 7: u32 count, then per contribution
  tauG1, tauG2, alphaG1, betaG1, betaG2            LEM points (448 bytes)
  tau / alpha / beta g1_s, g1_sx (6 G1), then the three g2_spx (768 bytes)
  partialHash                                       216 bytes: a Blake2b-512 state in progress (below)
  nextChallenge                                     64 bytes
  type (u32: 0 contribute, 1 beacon), parameter length (u32), parameters as in section 10 of a zkey
partialHash: h[8] u64 LE, t (bytes compressed so far) u64, f (0) u64, the 128-byte buffer, its fill u64: the
hasher after prev.nextChallenge and the new sections 2-6 in ffjavascript's compressed form (as recalled; no
verifier reads it).  responseHash = that state resumed, updated with the key's nine points uncompressed.
nextChallenge = Blake2b(responseHash || sections 2-6 uncompressed)."""
import functools
import hashlib
import struct

from oracle import binfile, bn254, mpc
from oracle.beacon import ChaCha

P, R = bn254.P, bn254.R
MASK64 = (1 << 64) - 1
KEYS = ("tau", "alpha", "beta")
NO_CONTRIBUTION = "This file has no contribution! It cannot be used in production"
HASH_MSG = "Hash of the values does not match the next challenge of the last contributor in the contributions section"

# ------------------------------------------------------------------ Blake2b-512 with an exportable state

_IV = [0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
       0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179]
_SIGMA = [
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
    [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4], [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
    [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13], [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
    [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11], [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
    [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5], [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0]]


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & MASK64


class Blake2b512:
    """RFC 7693, 64-byte digest, no key.  A full buffer is compressed only when more data arrives, so the
    last block is always in the buffer: fill ranges over 0..128 and t counts the bytes compressed."""

    def __init__(self):
        self.h = list(_IV)
        self.h[0] ^= 0x01010000 ^ 64
        self.t = 0
        self.buf = b""

    def _compress(self, block, t, last):
        m = struct.unpack("<16Q", block)
        v = self.h + list(_IV)
        v[12] ^= t & MASK64
        v[13] ^= t >> 64
        if last:
            v[14] ^= MASK64

        def g(a, b, c, d, x, y):
            v[a] = (v[a] + v[b] + x) & MASK64
            v[d] = _rotr(v[d] ^ v[a], 32)
            v[c] = (v[c] + v[d]) & MASK64
            v[b] = _rotr(v[b] ^ v[c], 24)
            v[a] = (v[a] + v[b] + y) & MASK64
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = (v[c] + v[d]) & MASK64
            v[b] = _rotr(v[b] ^ v[c], 63)

        for r in range(12):
            s = _SIGMA[r % 10]
            g(0, 4, 8, 12, m[s[0]], m[s[1]])
            g(1, 5, 9, 13, m[s[2]], m[s[3]])
            g(2, 6, 10, 14, m[s[4]], m[s[5]])
            g(3, 7, 11, 15, m[s[6]], m[s[7]])
            g(0, 5, 10, 15, m[s[8]], m[s[9]])
            g(1, 6, 11, 12, m[s[10]], m[s[11]])
            g(2, 7, 8, 13, m[s[12]], m[s[13]])
            g(3, 4, 9, 14, m[s[14]], m[s[15]])
        return [self.h[i] ^ v[i] ^ v[i + 8] for i in range(8)]

    def update(self, data):
        data = bytes(data)
        while data:
            if len(self.buf) == 128:
                self.t += 128
                self.h = self._compress(self.buf, self.t, False)
                self.buf = b""
            k = min(len(data), 128 - len(self.buf))
            self.buf += data[:k]
            data = data[k:]
        return self

    def digest(self):
        h = self._compress(self.buf.ljust(128, b"\0"), self.t + len(self.buf), True)
        return struct.pack("<8Q", *h)

    def export_state(self) -> bytes:
        return struct.pack("<8Q", *self.h) + struct.pack("<QQ", self.t, 0) + self.buf.ljust(128, b"\0") + \
            struct.pack("<Q", len(self.buf))

    @classmethod
    def import_state(cls, s: bytes):
        if len(s) != 216:
            raise ValueError("a Blake2b state has 216 bytes")
        o = cls()
        o.h = list(struct.unpack_from("<8Q", s, 0))
        o.t, f = struct.unpack_from("<QQ", s, 64)
        (fill,) = struct.unpack_from("<Q", s, 208)
        if f != 0 or fill > 128:
            raise ValueError("Blake2b state: final flag set or buffer fill above 128")
        o.buf = bytes(s[80:80 + fill])
        return o


def blake2b(data=b""):
    return hashlib.blake2b(data, digest_size=64).digest()


# ------------------------------------------------------------------ encodings

def g1_c(pt) -> bytes:
    """ffjavascript's compressed G1 (as recalled): x big-endian, 0x80 when y is the greater root, 0x40 infinity"""
    if pt is None:
        return bytes([0x40]) + bytes(31)
    b = bytearray(pt[0].to_bytes(32, "big"))
    if pt[1] > (P - 1) // 2:
        b[0] |= 0x80
    return bytes(b)


def g2_c(pt) -> bytes:
    if pt is None:
        return bytes([0x40]) + bytes(63)
    (x0, x1), y = pt
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))
    if mpc._neg_fq2(y):
        b[0] |= 0x80
    return bytes(b)


SECTION_IDS = (2, 3, 4, 5, 6)
LAGRANGE_IDS = {12: 2, 13: 3, 14: 4, 15: 5}


def _g2(sid):
    return sid in (3, 6, 13)


class Ptau:
    def __init__(self, power, ceremony_power, sections, contributions):
        self.power, self.ceremony_power = power, ceremony_power
        self.sections = sections  # {id: [points]}
        self.contributions = contributions  # dicts

    @classmethod
    def read(cls, buf: bytes):
        _, secs = binfile.read_binfile(buf, b"ptau", 1)
        raw = {sid: bytes(buf[v[0][0]:v[0][0] + v[0][1]]) for sid, v in secs.items()}
        n8, = struct.unpack_from("<I", raw[1], 0)
        assert n8 == 32 and bn254.le_to_int(raw[1][4:36]) == P
        power, cp = struct.unpack_from("<II", raw[1], 36)
        sections = {}
        for sid, b in raw.items():
            if sid in SECTION_IDS or sid in LAGRANGE_IDS:
                pb, dec = (128, bn254.g2_from_lem) if _g2(sid) else (64, bn254.g1_from_lem)
                sections[sid] = [dec(b[i:i + pb]) for i in range(0, len(b), pb)]
        return cls(power, cp, sections, read_contributions(raw[7]))

    def write(self) -> bytes:
        out = [(1, struct.pack("<I", 32) + bn254.int_to_le(P) + struct.pack("<II", self.power, self.ceremony_power))]
        for sid in sorted(self.sections):
            enc = bn254.g2_to_lem if _g2(sid) else bn254.g1_to_lem
            out.append((sid, b"".join(enc(p) for p in self.sections[sid])))
        out.append((7, write_contributions(self.contributions)))
        return binfile.write_binfile(b"ptau", 1, sorted(out))


def _params_bytes(c) -> bytes:
    params = []
    if c.get("name") is not None:
        nm = mpc.mpc_name_bytes(c["name"])
        params += [1, len(nm)] + list(nm)
    if c["type"] == 1:
        params += [2, c["numIterationsExp"], 3, len(c["beaconHash"])] + list(c["beaconHash"])
    return bytes(params)


def write_contributions(cons) -> bytes:
    out = [struct.pack("<I", len(cons))]
    for c in cons:
        out += [bn254.g1_to_lem(c["tauG1"]), bn254.g2_to_lem(c["tauG2"]), bn254.g1_to_lem(c["alphaG1"]),
                bn254.g1_to_lem(c["betaG1"]), bn254.g2_to_lem(c["betaG2"])]
        for k in KEYS:
            out += [bn254.g1_to_lem(c["key"][k]["g1_s"]), bn254.g1_to_lem(c["key"][k]["g1_sx"])]
        out += [bn254.g2_to_lem(c["key"][k]["g2_spx"]) for k in KEYS]
        prm = _params_bytes(c)
        out += [c["partialHash"], c["nextChallenge"], struct.pack("<II", c["type"], len(prm)), prm]
    return b"".join(out)


def read_contributions(sec: bytes):
    (n,) = struct.unpack_from("<I", sec, 0)
    o, cons = 4, []
    for _ in range(n):
        g1 = lambda at: bn254.g1_from_lem(sec[o + at:o + at + 64])
        g2 = lambda at: bn254.g2_from_lem(sec[o + at:o + at + 128])
        c = {"tauG1": g1(0), "tauG2": g2(64), "alphaG1": g1(192), "betaG1": g1(256), "betaG2": g2(320), "key": {}}
        for i, k in enumerate(KEYS):
            c["key"][k] = {"g1_s": g1(448 + 128 * i), "g1_sx": g1(448 + 128 * i + 64), "g2_spx": g2(448 + 384 + 128 * i)}
        o += 1216
        c["partialHash"], c["nextChallenge"] = bytes(sec[o:o + 216]), bytes(sec[o + 216:o + 280])
        c["type"], plen = struct.unpack_from("<II", sec, o + 280)
        o += 288
        prm = bytes(sec[o:o + plen])
        if len(prm) != plen:
            raise ValueError("ptau: section 7 parameter length runs past the section's end")
        o += plen
        j = 0
        while j < len(prm):
            pid = prm[j]
            if pid == 2:
                c["numIterationsExp"] = prm[j + 1]
                j += 2
                continue
            ln = prm[j + 1]
            val = prm[j + 2:j + 2 + ln]
            if pid == 1:
                c["name"] = val.decode("utf-8")
            elif pid == 3:
                c["beaconHash"] = bytes(val)
            else:
                raise ValueError("ptau: contribution parameter %d not recognized" % pid)
            j += 2 + ln
        cons.append(c)
    if o != len(sec):
        raise ValueError("ptau: section 7 has trailing bytes")
    return cons


# ------------------------------------------------------------------ the hashes

def first_challenge(cp: int) -> bytes:
    n = 1 << cp
    g1, g2 = mpc.g1_u(bn254.G1_GEN), mpc.g2_u(bn254.G2_GEN)
    return blake2b(blake2b() + g1 * (2 * n - 1) + g2 * n + g1 * n + g1 * n + g2)


def sections_uncompressed(sections) -> bytes:
    return b"".join((mpc.g2_u if _g2(sid) else mpc.g1_u)(p) for sid in SECTION_IDS for p in sections[sid])


def sections_compressed(sections) -> bytes:
    return b"".join((g2_c if _g2(sid) else g1_c)(p) for sid in SECTION_IDS for p in sections[sid])


def key_bytes(key) -> bytes:
    return b"".join(mpc.g1_u(key[k]["g1_s"]) + mpc.g1_u(key[k]["g1_sx"]) for k in KEYS) + \
        b"".join(mpc.g2_u(key[k]["g2_spx"]) for k in KEYS)


def response_hash(c) -> bytes:
    return Blake2b512.import_state(c["partialHash"]).update(key_bytes(c["key"])).digest()


def key_g2_sp(i: int, challenge: bytes, g1_s, g1_sx):
    return mpc.hash_to_g2(blake2b(bytes([i]) + challenge + mpc.g1_u(g1_s) + mpc.g1_u(g1_sx)))


def draw_key(rng: ChaCha, challenge: bytes):
    """-> (secrets {tau, alpha, beta}, public key)"""
    prv = {k: mpc.fr_from_rng(rng) for k in KEYS}
    key = {}
    for i, k in enumerate(KEYS):
        g1_s = mpc.g1_from_rng(rng)
        g1_sx = bn254.g1_mul(g1_s, prv[k])
        key[k] = {"g1_s": g1_s, "g1_sx": g1_sx, "g2_spx": bn254.g2_mul(key_g2_sp(i, challenge, g1_s, g1_sx), prv[k])}
    return prv, key


# ------------------------------------------------------------------ new / contribute / beacon

def new(power: int, ceremony_power: int = None) -> bytes:
    """`powersoftau new`: every point a generator, no contribution"""
    n = 1 << power
    secs = {2: [bn254.G1_GEN] * (2 * n - 1), 3: [bn254.G2_GEN] * n, 4: [bn254.G1_GEN] * n, 5: [bn254.G1_GEN] * n,
            6: [bn254.G2_GEN]}
    return Ptau(power, power if ceremony_power is None else ceremony_power, secs, []).write()


def _last_challenge(pt: Ptau) -> bytes:
    return pt.contributions[-1]["nextChallenge"] if pt.contributions else first_challenge(pt.ceremony_power)


def contribute(ptau: bytes, rng: ChaCha, name: str = None, ctype: int = 0, beacon_params=None) -> bytes:
    """`powersoftau contribute` with the key drawn from rng"""
    pt = Ptau.read(ptau)
    challenge = _last_challenge(pt)
    prv, key = draw_key(rng, challenge)
    tau, alpha, beta = prv["tau"], prv["alpha"], prv["beta"]
    s = pt.sections
    tp = [pow(tau, i, R) for i in range(len(s[2]))]
    new_s = {2: [bn254.g1_mul(p, t) for p, t in zip(s[2], tp)], 3: [bn254.g2_mul(p, t) for p, t in zip(s[3], tp)],
             4: [bn254.g1_mul(p, alpha * t % R) for p, t in zip(s[4], tp)],
             5: [bn254.g1_mul(p, beta * t % R) for p, t in zip(s[5], tp)], 6: [bn254.g2_mul(s[6][0], beta)]}
    partial = Blake2b512().update(challenge).update(sections_compressed(new_s))
    c = {"tauG1": new_s[2][1], "tauG2": new_s[3][1], "alphaG1": new_s[4][0], "betaG1": new_s[5][0], "betaG2": new_s[6][0],
         "key": key, "partialHash": partial.export_state(), "type": ctype}
    if name is not None:
        c["name"] = name
    if ctype == 1:
        c["beaconHash"], c["numIterationsExp"] = beacon_params
    c["nextChallenge"] = blake2b(response_hash(c) + sections_uncompressed(new_s))
    return Ptau(pt.power, pt.ceremony_power, new_s, pt.contributions + [c]).write()


def beacon(ptau: bytes, beacon_hash: bytes, num_iterations_exp: int, name: str = None) -> bytes:
    return contribute(ptau, mpc.beacon_rng(beacon_hash, num_iterations_exp), name, 1,
                      (bytes(beacon_hash), num_iterations_exp))


# ------------------------------------------------------------------ verify

@functools.lru_cache(maxsize=None)
def same_ratio(g1a, g1b, g2a, g2b) -> bool:
    return mpc.same_ratio(g1a, g1b, g2a, g2b)


@functools.lru_cache(maxsize=None)
def _in_g2(pt) -> bool:
    return pt is None or (bn254.g2_on_curve(pt) and mpc.g2_mul_full(pt, R) is None)


def check_contribution(i: int, c, prev) -> str:
    """"" if contribution i follows prev = (tauG1, tauG2, alphaG1, betaG1, betaG2, nextChallenge)"""
    tag = "contribution %d: " % i
    g1s = [c["tauG1"], c["alphaG1"], c["betaG1"]] + [c["key"][k][n] for k in KEYS for n in ("g1_s", "g1_sx")]
    g2s = [c["tauG2"], c["betaG2"]] + [c["key"][k]["g2_spx"] for k in KEYS]
    if not all(p is None or bn254.g1_on_curve(p) for p in g1s):
        return tag + "a G1 point is not on the curve"
    if not all(_in_g2(p) for p in g2s):
        return tag + "a G2 point is not in G2"
    p_tau_g1, p_tau_g2, p_alpha_g1, p_beta_g1, p_beta_g2, challenge = prev
    if c["type"] == 1:
        _, key = draw_key(mpc.beacon_rng(c["beaconHash"], c["numIterationsExp"]), challenge)
        for k in KEYS:
            for n, label in (("g1_s", "G1_s"), ("g1_sx", "G1_sx"), ("g2_spx", "G2_spx")):
                if key[k][n] != c["key"][k][n]:
                    return "BEACON key (%s%s) is not generated correctly" % (k, label)
    sp = {}
    for j, k in enumerate(KEYS):
        sp[k] = key_g2_sp(j, challenge, c["key"][k]["g1_s"], c["key"][k]["g1_sx"])
        if not same_ratio(c["key"][k]["g1_s"], c["key"][k]["g1_sx"], sp[k], c["key"][k]["g2_spx"]):
            return "INVALID key (%s)" % k
    K = c["key"]
    if not same_ratio(p_tau_g1, c["tauG1"], sp["tau"], K["tau"]["g2_spx"]):
        return "INVALID tau*G1. contribution"
    if not same_ratio(K["tau"]["g1_s"], K["tau"]["g1_sx"], p_tau_g2, c["tauG2"]):
        return "INVALID tau*G2. contribution"
    if not same_ratio(p_alpha_g1, c["alphaG1"], sp["alpha"], K["alpha"]["g2_spx"]):
        return "INVALID alpha*G1. contribution"
    if not same_ratio(p_beta_g1, c["betaG1"], sp["beta"], K["beta"]["g2_spx"]):
        return "INVALID beta*G1. contribution"
    if not same_ratio(K["beta"]["g1_s"], K["beta"]["g1_sx"], p_beta_g2, c["betaG2"]):
        return "INVALID beta*G2. contribution"
    return ""


def _coeffs(seed: bytes, first: int, n: int):
    rng = ChaCha(mpc.seed_words(seed))
    words = [rng.next_u32() for _ in range(4 * (first + n))]
    return [sum(words[4 * i + j] << (32 * j) for j in range(4)) for i in range(first, first + n)]


def _lincomb(pts, co, g2):
    add, mul = (bn254.g2_add, bn254.g2_mul) if g2 else (bn254.g1_add, bn254.g1_mul)
    acc = None
    for p, k in zip(pts, co):
        if p is not None:
            acc = add(acc, mul(p, k))
    return acc


def verify_sections(pt: Ptau, seed: bytes) -> str:
    """"" or the first failing check of zkp_ptau_verify_sections"""
    s = pt.sections
    ids = [sid for sid in (2, 3, 4, 5, 6, 12, 13, 14, 15) if sid in s]
    for sid in ids:
        on = bn254.g2_on_curve if _g2(sid) else bn254.g1_on_curve
        for i, p in enumerate(s[sid]):
            if p is not None and not on(p):
                return "section %d point %d is not on the curve" % (sid, i)
    for sid in ids:
        if _g2(sid):
            for i, p in enumerate(s[sid]):
                if not _in_g2(p):
                    return "section %d point %d is not in the subgroup" % (sid, i)
    if s[2][0] != bn254.G1_GEN:
        return "First element of tau*G1 section must be the generator"
    if s[3][0] != bn254.G2_GEN:
        return "First element of tau*G2 section must be the generator"
    for p, what in ((s[2][1], "Second element of tau*G1 section"), (s[3][1], "Second element of tau*G2 section"),
                    (s[4][0], "First element of alpha*tau*G1 section"), (s[5][0], "First element of beta*tau*G1 section"),
                    (s[6][0], "beta*G2")):
        if p is None:
            return what + " is the point at infinity"
    first = 0
    for sid, name in ((2, "tauG1"), (3, "tauG2"), (4, "alphaTauG1"), (5, "betaTauG1")):
        pts = s[sid]
        co = _coeffs(seed, first, len(pts) - 1)
        first += len(pts) - 1
        a, b = _lincomb(pts[:-1], co, _g2(sid)), _lincomb(pts[1:], co, _g2(sid))
        ok = same_ratio(bn254.G1_GEN, s[2][1], a, b) if sid == 3 else same_ratio(a, b, bn254.G2_GEN, s[3][1])
        if not ok:
            return "%s section. Powers do not match" % name
    if not same_ratio(bn254.G1_GEN, s[5][0], bn254.G2_GEN, s[6][0]):
        return "betaG2 does not match betaTauG1"
    for lid, tid in sorted(LAGRANGE_IDS.items()):
        if lid not in s:
            continue
        from oracle import setup
        add, mul = (bn254.g2_add, bn254.g2_mul) if _g2(lid) else (bn254.g1_add, bn254.g1_mul)
        for p in range(pt.power + 1):
            n, w = 1 << p, setup.ROOTS[p]
            ninv = bn254.inv(n, R)
            for c in range(n):
                acc = None
                for j in range(n):
                    if s[tid][j] is not None:
                        acc = add(acc, mul(s[tid][j], ninv * pow(w, (-c * j) % n, R) % R))
                if acc != s[lid][n - 1 + c]:
                    return "Lagrange section %d does not match section %d at level %d" % (lid, tid, p)
    return ""


def verify(ptau: bytes, seed: bytes = bytes(32)):
    """-> (valid, message) as zkp_ptau_verify"""
    pt = Ptau.read(ptau)
    cons = pt.contributions
    if not cons:
        return False, NO_CONTRIBUTION

    def check(i):
        if i == 0:
            g1, g2 = bn254.G1_GEN, bn254.G2_GEN
            prev = (g1, g2, g1, g1, g2, first_challenge(pt.ceremony_power))
        else:
            p = cons[i - 1]
            prev = (p["tauG1"], p["tauG2"], p["alphaG1"], p["betaG1"], p["betaG2"], p["nextChallenge"])
        return check_contribution(i, cons[i], prev)

    last = cons[-1]
    m = check(len(cons) - 1)
    if m:
        return False, m
    s = pt.sections
    tail = " does not match the one in the contribution section"
    for got, want, what in ((s[2][1], last["tauG1"], "Second element of tau*G1 section"),
                            (s[3][1], last["tauG2"], "Second element of tau*G2 section"),
                            (s[4][0], last["alphaG1"], "First element of alpha*tau*G1 section"),
                            (s[5][0], last["betaG1"], "First element of beta*tau*G1 section"),
                            (s[6][0], last["betaG2"], "beta*G2")):
        if got != want:
            return False, what + tail
    m = verify_sections(pt, seed)
    if m:
        return False, m
    if pt.power == pt.ceremony_power:
        if blake2b(response_hash(last) + sections_uncompressed(s)) != last["nextChallenge"]:
            return False, HASH_MSG
    for i in range(len(cons) - 2, -1, -1):
        m = check(i)
        if m:
            return False, m
    return True, "OK"
