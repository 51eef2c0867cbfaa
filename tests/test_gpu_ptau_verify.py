"""`powersoftau verify` on the GPU, the point sections (zkp_ptau_verify_sections, csrc/ptau_verify.hip):
the oracle's known-tau files are accepted under several coefficient seeds, with and without their Lagrange
sections and across chunk boundaries; every class of tampering is rejected with its message under every
seed; and the device parts are pinned on their own: the G2 subgroup kernel against points of the twist
outside G2 (one of order 10069), the pair sums against a Python sum over the same ChaCha coefficients."""
import os
import sys

import pytest

from oracle import binfile, bn254, mpc
from oracle.beacon import ChaCha
from test_gpu_ptau_prepare import _oracle_ptau, _sections
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import g2_twist  # noqa: E402

pytestmark = pytest.mark.gpu

P, R = bn254.P, bn254.R
SEEDS = [bytes(range(100, 132)), bytes(range(3, 35)), bytes(255 - i for i in range(32))]
OK = (True, "OK")
G1X = bn254.g1_mul(bn254.G1_GEN, 999)  # "another subgroup point"
G2X = bn254.g2_mul(bn254.G2_GEN, 999)
ENC = {False: bn254.g1_to_lem, True: bn254.g2_to_lem}
DEC = {False: bn254.g1_from_lem, True: bn254.g2_from_lem}


def _g2(sid):
    return sid in (3, 6, 13)


def _file(secs):
    return binfile.write_binfile(b"ptau", 1, sorted(secs.items()))


def _get(secs, sid, i):
    pb = 128 if _g2(sid) else 64
    return DEC[_g2(sid)](secs[sid][i * pb:(i + 1) * pb])


def _put(secs, sid, edits):
    """a copy of secs with points {index: point} of section sid replaced"""
    pb = 128 if _g2(sid) else 64
    raw = bytearray(secs[sid])
    for i, pt in edits.items():
        raw[i * pb:(i + 1) * pb] = ENC[_g2(sid)](pt)
    out = dict(secs)
    out[sid] = bytes(raw)
    return out


def _verify_all_seeds(buf):
    return [zkp_amd.ptau_verify_sections(buf, seed=s) for s in SEEDS]


# ------------------------------------------------------------------ valid files

@pytest.mark.parametrize("power", [1, 2, 5, 7])
def test_accepts_the_oracles_file_with_and_without_lagrange_sections(power):
    full = _oracle_ptau(power)
    assert _verify_all_seeds(full) == [OK] * 3
    t = zkp_amd.ptau_verify_timings()
    assert t["total"] > 0 and t["subgroup_check"] > 0 and t["accumulate_pairs"] > 0 and t["accumulate_lagrange"] > 0
    assert t["accumulate_tau"] > 0 and t["ntt_scalar_fold"] > 0 and t["chunks"] >= 6
    secs = _sections(full)
    assert _verify_all_seeds(_file({sid: secs[sid] for sid in range(1, 8)})) == [OK] * 3
    assert zkp_amd.ptau_verify_timings()["accumulate_lagrange"] == 0
    assert zkp_amd.ptau_verify_sections(full) == OK  # the OS seed


def test_chunk_boundaries_inside_levels_and_between_pair_bases(monkeypatch):
    """Power 13 with 1000 points per chunk: tauG1's 16382 pairs are 16 chunks and a ragged one, each run
    against the section at offsets 0 and 1; the Lagrange sections' chunk boundaries fall inside levels 10-13;
    levels 10-13 take the NTT's multi-pass path.  The file comes from the closed form on the device."""
    from zkp_amd import synth
    full = synth.ptau(13, 0xC0FFEE, device=0).bytes()
    monkeypatch.setenv("ZKP_VERIFY_CHUNK", "1000")
    assert _verify_all_seeds(full) == [OK] * 3
    assert zkp_amd.ptau_verify_timings()["chunks"] == 17 + 3 * 9 + 17 + 9
    secs = _sections(full)
    n = 1 << 13
    # a point of the last, ragged chunk of the pairs, and one behind a chunk boundary inside level 12
    bad = _file(_put(secs, 2, {2 * n - 2: G1X}))
    assert _verify_all_seeds(bad) == [(False, "tauG1 section. Powers do not match")] * 3
    i = (1 << 12) - 1 + 1000 - ((1 << 12) - 1) % 1000
    assert (1 << 12) - 1 < i < (1 << 13) - 1 and i % 1000 == 0
    bad = _file(_put(secs, 14, {i: G1X}))
    assert _verify_all_seeds(bad) == [(False, "Lagrange section 14 does not match section 4 at level 12")] * 3
    monkeypatch.delenv("ZKP_VERIFY_CHUNK")
    assert zkp_amd.ptau_verify_sections(bad, seed=SEEDS[0]) == (False, "Lagrange section 14 does not match section 4 at level 12")


# ------------------------------------------------------------------ mutations of the power-5 file

N5 = 32


def _mutations():
    """name -> (mutate(secs) -> secs, message)"""
    T = g2_twist.t_point
    pw = "%s section. Powers do not match"
    lag = "Lagrange section %d does not match section %d at level %d"
    m = {
        "tauG1 adjacent swapped": (lambda s: _put(s, 2, {10: _get(s, 2, 11), 11: _get(s, 2, 10)}), pw % "tauG1"),
        "tauG1 last replaced": (lambda s: _put(s, 2, {2 * N5 - 2: G1X}), pw % "tauG1"),
        "tauG1[0] not the generator": (lambda s: _put(s, 2, {0: G1X}), "First element of tau*G1 section must be the generator"),
        "tauG2[0] not the generator": (lambda s: _put(s, 3, {0: G2X}), "First element of tau*G2 section must be the generator"),
        "tauG2 replaced": (lambda s: _put(s, 3, {7: G2X}), pw % "tauG2"),
        "tauG2 last replaced": (lambda s: _put(s, 3, {N5 - 1: G2X}), pw % "tauG2"),
        "alphaTauG1 replaced": (lambda s: _put(s, 4, {N5 - 1: G1X}), pw % "alphaTauG1"),
        "betaTauG1 replaced": (lambda s: _put(s, 5, {3: G1X}), pw % "betaTauG1"),
        "betaG2 replaced": (lambda s: _put(s, 6, {0: G2X}), "betaG2 does not match betaTauG1"),
        "tauG1[1..] infinity": (lambda s: _put(s, 2, {i: None for i in range(1, 2 * N5 - 1)}),
                                "Second element of tau*G1 section is the point at infinity"),
        "tauG2[1] infinity": (lambda s: _put(s, 3, {1: None}), "Second element of tau*G2 section is the point at infinity"),
        "alphaTauG1[0] infinity": (lambda s: _put(s, 4, {0: None}), "First element of alpha*tau*G1 section is the point at infinity"),
        "betaTauG1[0] infinity": (lambda s: _put(s, 5, {0: None}), "First element of beta*tau*G1 section is the point at infinity"),
        "betaG2 infinity": (lambda s: _put(s, 6, {0: None}), "beta*G2 is the point at infinity"),
        "tauG2[k] + T": (lambda s: _put(s, 3, {9: bn254.g2_add(_get(s, 3, 9), T())}), "section 3 point 9 is not in the subgroup"),
        "lTauG2[i] + T": (lambda s: _put(s, 13, {40: bn254.g2_add(_get(s, 13, 40), T())}), "section 13 point 40 is not in the subgroup"),
        "betaG2 + T": (lambda s: _put(s, 6, {0: bn254.g2_add(_get(s, 6, 0), T())}), "section 6 point 0 is not in the subgroup"),
        "Q in tauG2": (lambda s: _put(s, 3, {N5 - 1: g2_twist.q_point()}), "section 3 point 31 is not in the subgroup"),
        "two bad G2 points: the smallest index": (lambda s: _put(s, 3, {20: T(), 4: g2_twist.q_point()}),
                                                  "section 3 point 4 is not in the subgroup"),
    }
    for sid, tid in ((12, 2), (13, 3), (14, 4), (15, 5)):
        X = G2X if sid == 13 else G1X
        m["section %d level 0" % sid] = (lambda s, sid=sid, X=X: _put(s, sid, {0: X}), lag % (sid, tid, 0))
        m["section %d level 3 swapped" % sid] = (
            lambda s, sid=sid: _put(s, sid, {8: _get(s, sid, 9), 9: _get(s, sid, 8)}), lag % (sid, tid, 3))
        m["section %d top level last" % sid] = (lambda s, sid=sid, X=X: _put(s, sid, {2 * N5 - 2: X}), lag % (sid, tid, 5))
    return m


def _plus_p(secs, sid, idx, coord):
    pb = 128 if _g2(sid) else 64
    raw = bytearray(secs[sid])
    at = idx * pb + 32 * coord
    x = int.from_bytes(raw[at:at + 32], "little")
    assert x + P < 1 << 256
    raw[at:at + 32] = (x + P).to_bytes(32, "little")
    out = dict(secs)
    out[sid] = bytes(raw)
    return out


MUTATIONS = sorted([
    "tauG1 adjacent swapped", "tauG1 last replaced", "tauG1[0] not the generator", "tauG2[0] not the generator",
    "tauG2 replaced", "tauG2 last replaced", "alphaTauG1 replaced", "betaTauG1 replaced", "betaG2 replaced",
    "tauG1[1..] infinity", "tauG2[1] infinity", "alphaTauG1[0] infinity", "betaTauG1[0] infinity", "betaG2 infinity",
    "tauG2[k] + T", "lTauG2[i] + T", "betaG2 + T", "Q in tauG2", "two bad G2 points: the smallest index"] + [
    "section %d %s" % (sid, what) for sid in (12, 13, 14, 15) for what in ("level 0", "level 3 swapped", "top level last")])


def test_the_mutation_list_is_complete():
    assert MUTATIONS == sorted(_mutations())


@pytest.mark.parametrize("name", MUTATIONS)
def test_rejects_a_mutated_file_under_every_seed(name):
    mutate, message = _mutations()[name]
    secs = _sections(_oracle_ptau(5))
    bad = mutate(secs)
    assert bad != secs
    assert _verify_all_seeds(_file(bad)) == [(False, message)] * 3


@pytest.mark.parametrize("sid,idx,coord", [(2, 62, 0), (3, 5, 3), (4, 0, 1), (5, 31, 0), (6, 0, 2), (12, 17, 1), (13, 62, 0),
                                           (14, 1, 0), (15, 30, 1)])
def test_rejects_a_non_canonical_coordinate(sid, idx, coord):
    secs = _sections(_oracle_ptau(5))
    bad = _file(_plus_p(secs, sid, idx, coord))
    assert _verify_all_seeds(bad) == [(False, "section %d point %d is not on the curve" % (sid, idx))] * 3


def test_the_first_bad_section_is_named():
    secs = _sections(_oracle_ptau(5))
    bad = _plus_p(_plus_p(secs, 13, 3, 0), 4, 9, 0)
    bad = _put(bad, 3, {2: g2_twist.t_point()})  # on the curve: the curve message of section 4 comes first
    assert zkp_amd.ptau_verify_sections(_file(bad), seed=SEEDS[0]) == (False, "section 4 point 9 is not on the curve")
    (x, (y0, y1)) = _get(secs, 3, 6)
    off = _put(secs, 3, {6: (x, ((y0 + 1) % P, y1))})
    assert zkp_amd.ptau_verify_sections(_file(off), seed=SEEDS[0]) == (False, "section 3 point 6 is not on the curve")


# ------------------------------------------------------------------ zkp_g2_subgroup_check

def _g2_multiples(n):
    pts, acc = [], None
    for _ in range(n):
        acc = bn254.g2_add(acc, bn254.G2_GEN)
        pts.append(acc)
    return pts


_G2M = None


def _multiples(n):
    global _G2M
    if _G2M is None:
        _G2M = _g2_multiples(257)
    return list(_G2M[:n])


def _lem2(pts):
    return b"".join(bn254.g2_to_lem(p) for p in pts)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_g2_subgroup_check(n):
    t = g2_twist.t_point()
    pts = _multiples(n)
    if n > 1:
        pts[n // 2] = None  # infinity is accepted
    assert zkp_amd.g2_subgroup_check(_lem2(pts)) == (0, None)
    assert zkp_amd.g2_subgroup_check(_lem2([None] * n)) == (0, None)
    for where in ([0], [n - 1], sorted({n - 1, n // 3})):
        bad = list(pts)
        for i in where:
            bad[i] = t if bad[i] is None else bn254.g2_add(bad[i], t)
        assert zkp_amd.g2_subgroup_check(_lem2(bad)) == (len(where), where[0])
    assert zkp_amd.g2_subgroup_check(b"") == (0, None)


def test_g2_subgroup_check_of_twist_points_and_across_chunks(monkeypatch):
    q, t = g2_twist.q_point(), g2_twist.t_point()
    pts = [q, t, g2_twist.mul_any(t, 2), g2_twist.mul_any(q, R), bn254.G2_GEN, bn254.g2_mul(bn254.G2_GEN, R - 1)]
    assert zkp_amd.g2_subgroup_check(_lem2(pts)) == (4, 0)
    assert zkp_amd.g2_subgroup_check(_lem2(pts[4:] + pts[3:4])) == (1, 2)
    monkeypatch.setenv("ZKP_VERIFY_CHUNK", "5")
    bad = _multiples(23)
    bad[5], bad[22] = t, q
    assert zkp_amd.g2_subgroup_check(_lem2(bad)) == (2, 5)
    bad[5] = bn254.G2_GEN
    assert zkp_amd.g2_subgroup_check(_lem2(bad)) == (1, 22)


# ------------------------------------------------------------------ zkp_rlc_pairs

def _coeffs(seed, first, n):
    rng = ChaCha(mpc.seed_words(seed))
    words = [rng.next_u32() for _ in range(4 * (first + n))]
    return [sum(words[4 * i + j] << (32 * j) for j in range(4)) for i in range(first, first + n)]


def _lincomb(pts, co, g2):
    add, mul = (bn254.g2_add, bn254.g2_mul) if g2 else (bn254.g1_add, bn254.g1_mul)
    acc = None
    for p, c in zip(pts, co):
        if p is not None:
            acc = add(acc, mul(p, c))
    return acc


def _pair_points(n, g2):
    """distinct points with an infinity, a repeated point and a pair P, -P"""
    gen, mul, neg = (bn254.G2_GEN, bn254.g2_mul, bn254.g2_neg) if g2 else (bn254.G1_GEN, bn254.g1_mul, bn254.g1_neg)
    pts = [mul(gen, 3 * i + 1) for i in range(n)]
    if n >= 8:
        pts[1] = None
        pts[4] = pts[3]
        pts[6] = neg(pts[5])
    return pts


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n,first,chunk", [(0, 0, None), (1, 0, None), (2, 0, None), (2, 7, None), (15, 0, None),
                                           (15, 5, None), (15, 5, "5"), (15, 0, "1")])
def test_rlc_pairs_match_a_python_sum(monkeypatch, g2, n, first, chunk):
    if chunk:
        monkeypatch.setenv("ZKP_VERIFY_CHUNK", chunk)
    pts = _pair_points(n, g2)
    co = _coeffs(SEEDS[0], first, max(n - 1, 0))
    got = zkp_amd.rlc_pairs(SEEDS[0], first, b"".join(ENC[g2](p) for p in pts), g2=g2)
    assert got == (_lincomb(pts[:-1], co, g2), _lincomb(pts[1:], co, g2))
    if n <= 1:
        assert got == (None, None)


def test_rlc_pairs_refuse_a_point_off_the_curve():
    pts = _pair_points(4, False)
    pts[2] = (pts[2][0], (pts[2][1] + 1) % P)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.rlc_pairs(SEEDS[0], 0, b"".join(bn254.g1_to_lem(p) for p in pts))
    assert e.value.status == 1 and "point 2" in e.value.message


# ------------------------------------------------------------------ zkp_ptau_verify: the contribution chain too

import ctypes  # noqa: E402

import ptau_model as pm  # noqa: E402
from test_ptau_model import _set, ceremony, mutated  # noqa: E402


def _both(buf):
    """the library's verdict, which must be the model's"""
    got = zkp_amd.ptau_verify(buf, seed=SEEDS[0])
    assert got == pm.verify(buf, SEEDS[0])
    return got


def test_full_verify_accepts_the_models_ceremony():
    final = ceremony(3, None, 2)[-1]  # power 3 = ceremonyPower: two contributions and a beacon
    assert _both(final) == OK
    t = zkp_amd.ptau_verify_timings()
    assert t["contributions"] > 0 and t["first_challenge"] > 0 and t["next_challenge"] > 0
    assert t["subgroup_check"] > 0 and t["total"] >= t["contributions"]
    assert zkp_amd.ptau_verify(final) == OK  # the OS seed
    assert zkp_amd.ptau_verify_sections(final, seed=SEEDS[1]) == OK
    # every earlier stage is a valid file of its own
    assert zkp_amd.ptau_verify(ceremony(3, None, 2)[1], seed=SEEDS[0]) == OK


def test_full_verify_of_a_truncated_ceremony_skips_the_next_challenge():
    final = ceremony(3, 4, 2)[-1]  # ceremonyPower 4: the first challenge is hashed at 4
    assert zkp_amd.ptau_verify(final, seed=SEEDS[0]) == OK
    assert zkp_amd.ptau_verify_timings()["next_challenge"] == 0
    bad = mutated(final, _set((2, "nextChallenge"), bytes(64)))
    assert zkp_amd.ptau_verify(bad, seed=SEEDS[0]) == OK
    # the same records under ceremonyPower 3 answer another first challenge
    pt = pm.Ptau.read(final)
    pt.ceremony_power = 3
    assert zkp_amd.ptau_verify(pt.write(), seed=SEEDS[0])[0] is False


def test_full_verify_rejects_a_file_without_contributions():
    assert _both(ceremony(3, None, 2)[0]) == (False, pm.NO_CONTRIBUTION)
    assert zkp_amd.ptau_verify(_oracle_ptau(2), seed=SEEDS[0]) == (False, pm.NO_CONTRIBUTION)


FULL_MUTATIONS = [
    ("a key point", _set((1, "key", "alpha", "g1_sx"), G1X), "INVALID key (alpha)"),
    ("a record point", _set((1, "tauG1"), G1X), "INVALID tau*G1. contribution"),
    ("the beacon exponent", _set((2, "numIterationsExp"), 6), "BEACON key (tauG1_s) is not generated correctly"),
    ("the last nextChallenge", _set((2, "nextChallenge"), bytes(range(64))), pm.HASH_MSG),
    ("the first contribution's key", _set((0, "key", "tau", "g2_spx"), G2X), "INVALID key (tau)"),
]


@pytest.mark.parametrize("name,fn,message", FULL_MUTATIONS, ids=[m[0] for m in FULL_MUTATIONS])
def test_full_verify_rejects_with_the_models_message(name, fn, message):
    assert _both(mutated(ceremony(3, None, 2)[-1], fn)) == (False, message)


def test_full_verify_ties_the_sections_to_the_last_record():
    stages = ceremony(3, None, 2)
    before, final = pm.Ptau.read(stages[2]), pm.Ptau.read(stages[3])
    lag = pm.Ptau(3, 3, before.sections, final.contributions).write()
    assert _both(lag) == (False, "Second element of tau*G1 section does not match the one in the contribution section")
    # a section point behind the singular ones: the section checks name it
    secs = dict(final.sections)
    secs[5] = final.sections[5][:7] + [G1X]
    assert _both(pm.Ptau(3, 3, secs, final.contributions).write()) == (False, "betaTauG1 section. Powers do not match")


def test_prepare_phase2_then_full_verify():
    final = ceremony(3, None, 2)[-1]
    prepared = zkp_amd.ptau_prepare_phase2(final)
    assert sorted(_sections(prepared)) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert zkp_amd.ptau_verify(prepared, seed=SEEDS[0]) == OK
    assert zkp_amd.ptau_verify_timings()["accumulate_lagrange"] > 0
    secs = _sections(prepared)
    bad = _file(_put(secs, 13, {14: G2X}))
    assert zkp_amd.ptau_verify(bad, seed=SEEDS[0]) == (False, "Lagrange section 13 does not match section 3 at level 3")


def test_message_truncation():
    lib = zkp_amd.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    buf = _file(_put(_sections(_oracle_ptau(2)), 2, {0: G1X}))
    full = "First element of tau*G1 section must be the generator"
    for cap in (1, 2, 10, len(full), len(full) + 1, 100):
        ok, msg = ctypes.c_int(5), ctypes.create_string_buffer(b"\xff" * 128, 129)
        assert lib.zkp_ptau_verify_sections(0, ctypes.cast(ctypes.c_char_p(buf), u8p), len(buf), None, ctypes.byref(ok),
                                            msg, cap) == 0
        assert ok.value == 0 and msg.value.decode() == full[:cap - 1]
        assert msg.raw[cap:] == b"\xff" * (128 - cap) + b"\0"  # nothing written past the capacity
