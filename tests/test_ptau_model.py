"""The Python model of a phase-1 ceremony file (tests/helpers/ptau_model.py), which fixes the recalled
section-7 format for zkp_ptau_verify: its Blake2b against hashlib across exports of the state, its own
power-2 ceremony (one contribution and a beacon) accepted, every record mutation rejected with the named
message; and the library's verdicts that need no device (everything before the sections) equal the model's.
CPU-only."""
import copy
import ctypes
import hashlib
import os
import struct
import sys

import pytest

from oracle import bn254
from oracle.beacon import ChaCha

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_model as pm  # noqa: E402
import zkp_amd  # noqa: E402

BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20")
SEED = bytes(range(100, 132))
NO_DEVICE = 1 << 20
G1X = bn254.g1_mul(bn254.G1_GEN, 999)
G2X = bn254.g2_mul(bn254.G2_GEN, 999)
_cache = {}


def ceremony(power=2, ceremony_power=None, contributions=1):
    """new -> `contributions` contributions -> beacon, every stage kept"""
    key = (power, ceremony_power, contributions)
    if key not in _cache:
        stages = [pm.new(power, ceremony_power)]
        for i in range(contributions):
            stages.append(pm.contribute(stages[-1], ChaCha([7 + i] * 8), name="contributor %d" % i))
        stages.append(pm.beacon(stages[-1], BEACON, 5, name="Final Beacon"))
        _cache[key] = stages
    return _cache[key]


def mutated(buf, fn):
    pt = copy.deepcopy(pm.Ptau.read(buf))
    fn(pt)
    return pt.write()


def library_verdict(buf):
    """zkp_ptau_verify with a device ordinal no machine has -> (status, valid, message)"""
    lib = zkp_amd.load_library()
    ok, msg = ctypes.c_int(), ctypes.create_string_buffer(256)
    st = lib.zkp_ptau_verify(NO_DEVICE, ctypes.cast(ctypes.c_char_p(buf), ctypes.POINTER(ctypes.c_uint8)), len(buf),
                             ctypes.cast(ctypes.c_char_p(SEED), ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(ok), msg, 256)
    return st, bool(ok.value), msg.value.decode()


# ------------------------------------------------------------------ Blake2b

@pytest.mark.parametrize("n", [0, 1, 63, 127, 128, 129, 255, 256, 257, 1000])
def test_blake2b_is_hashlibs(n):
    data = bytes((7 * i + 3) & 0xFF for i in range(n))
    want = hashlib.blake2b(data, digest_size=64).digest()
    assert pm.Blake2b512().update(data).digest() == want
    for cut in sorted({0, 1, n // 2, max(n - 1, 0), n}):
        h = pm.Blake2b512().update(data[:cut]).update(data[cut:])
        assert h.digest() == want and h.digest() == want  # digest does not consume the state


@pytest.mark.parametrize("fill,before", [(0, 0), (1, 1), (127, 127), (128, 128), (1, 129), (127, 255), (128, 256), (44, 300)])
def test_blake2b_resumes_across_an_export(fill, before):
    data = bytes((11 * i + 1) & 0xFF for i in range(before + 200))
    h = pm.Blake2b512().update(data[:before])
    st = h.export_state()
    assert len(st) == 216 and struct.unpack_from("<Q", st, 208)[0] == fill
    assert struct.unpack_from("<QQ", st, 64) == (before - fill, 0)
    r = pm.Blake2b512.import_state(st)
    assert r.export_state() == st
    assert r.update(data[before:]).digest() == hashlib.blake2b(data, digest_size=64).digest()
    with pytest.raises(ValueError):
        pm.Blake2b512.import_state(st[:208] + struct.pack("<Q", 129))
    with pytest.raises(ValueError):
        pm.Blake2b512.import_state(st[:72] + struct.pack("<Q", 1) + st[80:])


# ------------------------------------------------------------------ the model on its own ceremony

def test_first_challenge_counts_the_generators():
    g1, g2 = bytes(31) + b"\x01" + bytes(31) + b"\x02", None
    assert pm.mpc.g1_u(bn254.G1_GEN) == g1
    h = hashlib.blake2b(hashlib.blake2b(digest_size=64).digest(), digest_size=64)
    g2 = pm.mpc.g2_u(bn254.G2_GEN)
    for part in (g1 * 7, g2 * 4, g1 * 8, g2):
        h.update(part)
    assert pm.first_challenge(2) == h.digest() != pm.first_challenge(3)


def test_accepts_its_own_ceremony_and_round_trips():
    stages = ceremony()
    assert pm.verify(stages[0]) == (False, pm.NO_CONTRIBUTION)
    assert pm.verify(stages[1], SEED) == (True, "OK")
    assert pm.verify(stages[2], SEED) == (True, "OK")
    pt = pm.Ptau.read(stages[2])
    assert pt.write() == stages[2]
    assert [c["type"] for c in pt.contributions] == [0, 1]
    assert pt.contributions[1]["beaconHash"] == BEACON and pt.contributions[1]["numIterationsExp"] == 5
    assert pt.contributions[0]["name"] == "contributor 0"
    # the sections are the powers of the product of the secrets
    assert pt.sections[2][0] == bn254.G1_GEN and pt.sections[3][0] == bn254.G2_GEN
    assert bn254.pairing_prod_is_one([(bn254.g1_neg(pt.sections[2][2]), bn254.G2_GEN), (pt.sections[2][1], pt.sections[3][1])])


def _set(path, value):
    def fn(pt):
        o = pt.contributions
        for k in path[:-1]:
            o = o[k]
        o[path[-1]] = value
    return fn


RECORD_MUTATIONS = [
    ("last key tau g1_s", _set((1, "key", "tau", "g1_s"), G1X), "BEACON key (tauG1_s) is not generated correctly"),
    ("last key beta g2_spx", _set((1, "key", "beta", "g2_spx"), G2X), "BEACON key (betaG2_spx) is not generated correctly"),
    ("beacon exponent", _set((1, "numIterationsExp"), 4), "BEACON key (tauG1_s) is not generated correctly"),
    ("beacon hash", _set((1, "beaconHash"), BEACON[::-1]), "BEACON key (tauG1_s) is not generated correctly"),
    ("last tauG1", _set((1, "tauG1"), G1X), "INVALID tau*G1. contribution"),
    ("last tauG2", _set((1, "tauG2"), G2X), "INVALID tau*G2. contribution"),
    ("last alphaG1", _set((1, "alphaG1"), G1X), "INVALID alpha*G1. contribution"),
    ("last betaG1", _set((1, "betaG1"), G1X), "INVALID beta*G1. contribution"),
    ("last betaG2", _set((1, "betaG2"), G2X), "INVALID beta*G2. contribution"),
    ("last G1 point off the curve", _set((1, "alphaG1"), (5, 5)), "contribution 1: a G1 point is not on the curve"),
    ("first nextChallenge", _set((0, "nextChallenge"), bytes(64)), "BEACON key (tauG2_spx) is not generated correctly"),
    ("last nextChallenge", _set((1, "nextChallenge"), bytes(64)), pm.HASH_MSG),
    ("last partialHash", _set((1, "partialHash"), pm.Blake2b512().update(b"x").export_state()), pm.HASH_MSG),
    ("first key tau g1_sx", _set((0, "key", "tau", "g1_sx"), G1X), "INVALID key (tau)"),
    ("first key alpha g1_s", _set((0, "key", "alpha", "g1_s"), G1X), "INVALID key (alpha)"),
    ("first key beta g2_spx", _set((0, "key", "beta", "g2_spx"), G2X), "INVALID key (beta)"),
    ("first tauG2", _set((0, "tauG2"), G2X), "INVALID tau*G2. contribution"),
]
BEFORE_THE_SECTIONS = {m[0] for m in RECORD_MUTATIONS[:11]}


@pytest.mark.parametrize("name,fn,message", RECORD_MUTATIONS, ids=[m[0] for m in RECORD_MUTATIONS])
def test_rejects_a_record_mutation_with_its_message(name, fn, message):
    bad = mutated(ceremony()[2], fn)
    assert pm.verify(bad, SEED) == (False, message)
    if name in BEFORE_THE_SECTIONS:  # the library decides these on the host
        assert library_verdict(bad) == (0, False, message)


def test_a_type_0_record_is_not_redrawn():
    """the contribution's key is not a function of public data: only the ratios are checked"""
    pt = pm.Ptau.read(ceremony()[2])
    assert pt.contributions[0]["type"] == 0 and pm.verify(ceremony()[1], SEED) == (True, "OK")


def test_sections_that_lag_the_records_fail_the_ties():
    stages = ceremony()
    one, two = pm.Ptau.read(stages[1]), pm.Ptau.read(stages[2])
    lag = pm.Ptau(2, 2, one.sections, two.contributions).write()
    want = (False, "Second element of tau*G1 section does not match the one in the contribution section")
    assert pm.verify(lag, SEED) == want
    assert library_verdict(lag) == (0,) + want
    for sid, what in ((3, "Second element of tau*G2 section"), (4, "First element of alpha*tau*G1 section"),
                      (5, "First element of beta*tau*G1 section"), (6, "beta*G2")):
        secs = dict(two.sections)
        secs[sid] = one.sections[sid]
        bad = pm.Ptau(2, 2, secs, two.contributions).write()
        want = (False, what + " does not match the one in the contribution section")
        assert pm.verify(bad, SEED) == want
        assert library_verdict(bad) == (0,) + want


def test_section_mutations_reach_the_section_checks():
    stages = ceremony()
    pt = pm.Ptau.read(stages[2])
    secs = dict(pt.sections)
    secs[2] = pt.sections[2][:6] + [G1X]
    assert pm.verify(pm.Ptau(2, 2, secs, pt.contributions).write(), SEED) == (False, "tauG1 section. Powers do not match")
    secs = dict(pt.sections)
    secs[4] = pt.sections[4][:3] + [G1X]
    assert pm.verify(pm.Ptau(2, 2, secs, pt.contributions).write(), SEED) == (False, "alphaTauG1 section. Powers do not match")
    # a truncated ceremony: the next challenge cannot be recomputed and is not checked
    cut = pm.Ptau(2, 3, pt.sections, pt.contributions)
    cut.contributions = copy.deepcopy(pt.contributions)
    cut.contributions[1]["nextChallenge"] = bytes(64)
    assert pm.verify(cut.write(), SEED)[1] != pm.HASH_MSG


def test_the_library_reads_the_models_records():
    stages = ceremony()
    assert library_verdict(stages[0]) == (0, False, pm.NO_CONTRIBUTION)
    # a valid file passes every host check and gets as far as the device
    st, ok, msg = library_verdict(stages[2])
    assert st not in (0, 1, 3, 5) and not ok
    # malformed section 7
    _, secs = pm.binfile.read_binfile(stages[2], b"ptau", 1)
    raw = {sid: bytes(stages[2][v[0][0]:v[0][0] + v[0][1]]) for sid, v in secs.items()}

    def with7(sec7):
        return pm.binfile.write_binfile(b"ptau", 1, sorted({**raw, 7: sec7}.items()))

    rec0 = 4 + 1504
    plen0 = struct.unpack_from("<I", raw[7], rec0 - 4)[0]
    for bad7 in (raw[7][:-1], raw[7] + b"\0", raw[7][:700],
                 raw[7][:rec0 - 4] + struct.pack("<I", 1 << 20) + raw[7][rec0:],        # a length past the end
                 raw[7][:4 + 1216 + 72] + struct.pack("<Q", 1) + raw[7][4 + 1216 + 80:],   # partialHash: f set
                 raw[7][:4 + 1216 + 208] + struct.pack("<Q", 129) + raw[7][4 + 1216 + 216:],  # fill 129
                 raw[7][:4] + bytes([0xFF] * 32) + raw[7][36:]):                          # a coordinate >= p
        st, ok, msg = library_verdict(with7(bad7))
        assert st == 3 and not ok and msg == ""
        assert "section 7" in zkp_amd.load_library().zkp_last_error().decode()
    assert plen0 > 0
    # a beacon whose exponent is above 63 is a format error
    pt = copy.deepcopy(pm.Ptau.read(stages[2]))
    pt.contributions[1]["numIterationsExp"] = 64
    st, ok, msg = library_verdict(pt.write())
    assert st == 3 and "numIterationsExp" in zkp_amd.load_library().zkp_last_error().decode()
