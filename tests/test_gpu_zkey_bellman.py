"""`zkey export bellman | zkey bellman contribute | zkey import bellman` on the GPU (zkp_zkey_export_bellman,
zkp_zkey_bellman_contribute, zkp_zkey_import_bellman; csrc/zkey_bellman.hip), the forward group FFT they rest on
(zkp_group_fft) and the H rule of `zkey verify` that accepts an imported key.  The export of a fresh key must hash
to the csHash that `zkey new` computed from the ptau's tau powers (an independent path), every file must equal
tests/helpers/bellman_model.py, the three commands in a row must equal one `zkey contribute` except in section 9,
the imported key must verify and prove, and each refusal names what it refuses."""
import copy
import functools
import hashlib
import os
import struct
import sys

import pytest

from oracle import binfile, bn254, mpc, setup
from test_gpu_zkey_verify import BEACON, H_MSG, L_MSG, RAND64, SEED, SEED_B, TAU, _chain, _section
from test_setup_new import _case as _setup_case
import zkp_amd
from zkp_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bellman_model as bm  # noqa: E402

pytestmark = pytest.mark.gpu

P, R = bn254.P, bn254.R
OK = (True, "OK")
FORMAT = 3  # ZKP_ERR_FORMAT
RAND_B = bytes((29 * i + 5) & 0xFF for i in range(64))
ENTROPY = "bellman entropy"
NAME = "outside contributor"
G1B = bn254.FixedBase(bn254.G1_GEN)


def _blake(b):
    return hashlib.blake2b(b, digest_size=64).digest()


def _deltas():
    """delta of k0, k1, k2 of _chain: the secrets are the first draw of each contribution's rng"""
    k1 = mpc.fr_from_rng(mpc.entropy_rng(RAND64, "some entropy text"))
    k2 = mpc.fr_from_rng(mpc.beacon_rng(BEACON, 10))
    return [1, k1, k1 * k2 % R]


@functools.lru_cache(maxsize=None)
def _export(name, i):
    return zkp_amd.zkey_export_bellman(_chain(name)[2 + i])


@functools.lru_cache(maxsize=None)
def _three(name, i=1):
    """export -> bellman contribute -> import on key i of the chain: (challenge, response, hash, new key)"""
    key = _chain(name)[2 + i]
    challenge = _export(name, i)
    response, h = zkp_amd.zkey_bellman_contribute(challenge, ENTROPY, rand64=RAND_B, with_hash=True)
    return challenge, response, h, zkp_amd.zkey_import_bellman(key, response, name=NAME)


def _sections(buf):
    _, secs = binfile.read_binfile(buf, b"zkey", 1)
    return {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items()}


def _refused(fn, *text):
    with pytest.raises(zkp_amd.ZkpError) as e:
        fn()
    assert e.value.status == FORMAT
    for t in text:
        assert t in e.value.message, e.value.message
    return e.value.message


# ------------------------------------------------------------------ export

@pytest.mark.parametrize("name", ["tiny", "small"])
def test_export_of_a_fresh_key_hashes_to_its_cs_hash(name):
    k0 = _chain(name)[2]
    f = _export(name, 0)
    assert f[-68:-4] == binfile.read_zkey(k0).extra["mpc"]["cs_hash"] and f[-4:] == bytes(4)
    assert _blake(f[:-68]) == f[-68:-4]


def test_export_hashes_to_the_cs_hash_at_two_global_stages():
    """domain 2^11: the smallest G1 size whose top level takes the tiled path with two global stages"""
    c = synth.Circuit(1500, 1800, 3, 77)
    assert c.domain_size == 2048
    k0 = zkp_amd.zkey_new(c.r1cs(), synth.ptau(12, 77))
    f = zkp_amd.zkey_export_bellman(k0)
    assert zkp_amd.mpcparams_info(f) == {"n_public": 3, "domain_size": 2048, "n_vars": 1500, "n_contributions": 0}
    off, ln = _section(k0, 10)
    assert f[-68:-4] == k0[off:off + 64]
    assert _blake(f[:-68]) == f[-68:-4]


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_export_equals_the_model(name):
    for i, delta in enumerate(_deltas()):
        z = binfile.read_zkey(_chain(name)[2 + i])
        assert _export(name, i) == bm.export_model(z, TAU, delta), "key %d" % i


# ------------------------------------------------------------------ the three commands

@pytest.mark.parametrize("name", ["tiny", "small"])
def test_three_commands_equal_one_contribute_except_section_9(name):
    k1 = _chain(name)[3]
    challenge, response, h, new = _three(name)
    direct = zkp_amd.zkey_contribute_entropy(k1, ENTROPY, rand64=RAND_B, name=NAME)
    got, want = _sections(new), _sections(direct)
    assert sorted(got) == sorted(want) and len(new) == len(direct)
    assert [s for s in want if s != 9 and got[s] != want[s]] == []
    assert got[9] != want[9]
    # the two keys are the same MPCParams file, and it is the response
    assert zkp_amd.zkey_export_bellman(new) == zkp_amd.zkey_export_bellman(direct) == response
    assert h == _blake(response[-384:]) and len(response) == len(challenge) + 384
    assert zkp_amd.mpcparams_info(response)["n_contributions"] == 2


def test_response_equals_the_model():
    z = binfile.read_zkey(zkp_amd.zkey_contribute_entropy(_chain("tiny")[3], ENTROPY, rand64=RAND_B, name=NAME))
    k = mpc.fr_from_rng(mpc.entropy_rng(RAND_B, ENTROPY))
    assert _three("tiny")[1] == bm.export_model(z, TAU, _deltas()[1] * k % R)


def test_imported_h_is_the_defining_sum_and_has_no_w_component():
    _, response, _, new = _three("tiny")
    h = binfile.read_zkey(new).h
    assert h == bm.h_from_b(bm.parse(response)["h"], 16)
    assert bm.w_direction_sum(h) is None
    # a direct contribution's section has such a component: that is all the two differ by
    direct = binfile.read_zkey(zkp_amd.zkey_contribute_entropy(_chain("tiny")[3], ENTROPY, rand64=RAND_B, name=NAME)).h
    t = bm.w_direction_sum(direct)
    assert t is not None
    w, ninv = setup.ROOTS[4], bn254.inv(16, R)
    assert h == [bn254.g1_add(direct[j], bn254.g1_neg(bn254.g1_mul(t, ninv * pow(w, j, R) % R))) for j in range(16)]


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_the_imported_key_verifies_and_proves(name):
    r1cs, ptau, k0 = _chain(name)[:3]
    new = _three(name)[3]
    assert zkp_amd.zkey_verify_frominit(k0, new, seed=SEED) == OK
    assert zkp_amd.zkey_verify_frominit(k0, new, seed=SEED_B) == OK
    assert zkp_amd.zkey_verify(r1cs, ptau, new, seed=SEED) == OK
    assert zkp_amd.zkey_verify(r1cs, ptau, new, seed=SEED_B) == OK
    w = _setup_case(name)[1]
    (a, b, c), pub = zkp_amd.Prover(new).prove_raw(binfile.write_wtns(w))
    assert zkp_amd.proof_verify(new, (a, b, c), pub)


def test_the_relaxed_rule_is_what_accepts_an_imported_key():
    """the oracle's rule (an independent coefficient for every H point) rejects the key; the helper's restatement
    of the relaxed rule accepts it, with the coefficients of the device's stream"""
    k0, new = _chain("tiny")[2], _three("tiny")[3]
    assert mpc.zkey_verify(new, k0) == (False, H_MSG)
    z, z0 = binfile.read_zkey(new), binfile.read_zkey(k0)
    r = zkp_amd.rlc_coeffs(SEED, len(z.c), 16)
    assert bm.relaxed_h_check(z0.h, z.h, r, z.delta2, z0.delta2)


def test_beacon_after_import_and_the_old_records_survive():
    k0, k2 = _chain("tiny")[2], _chain("tiny")[4]
    response = zkp_amd.zkey_bellman_contribute(_export("tiny", 2), ENTROPY, rand64=RAND_B)
    new = zkp_amd.zkey_import_bellman(k2, response, name=NAME)
    assert zkp_amd.zkey_verify_frominit(k0, new, seed=SEED) == OK
    final = zkp_amd.zkey_beacon(new, BEACON, 10, name="after the import")
    assert zkp_amd.zkey_verify_frominit(k0, final, seed=SEED) == OK
    old = binfile.read_zkey(k2).extra["mpc"]["contributions"]
    cons = binfile.read_zkey(final).extra["mpc"]["contributions"]
    assert cons[:2] == old and [c.get("name") for c in cons] == ["first contribution", "Final Beacon phase2", NAME,
                                                                 "after the import"]
    assert [c["type"] for c in cons] == [0, 1, 0, 1]
    assert cons[1]["beaconHash"] == BEACON and cons[1]["numIterationsExp"] == 10
    # no name is recorded without one
    unnamed = binfile.read_zkey(zkp_amd.zkey_import_bellman(k2, response)).extra["mpc"]["contributions"][-1]
    assert "name" not in unnamed and unnamed["type"] == 0


# ------------------------------------------------------------------ refusals

OTHER_G1 = mpc.g1_u(G1B.mul(5))
OTHER_G2 = mpc.g2_u(bn254.g2_mul(bn254.G2_GEN, 5))


def _put(buf, at, b):
    out = bytearray(buf)
    out[at:at + len(b)] = b
    return bytes(out)


@pytest.mark.parametrize("sec,label", [("ic", "IC"), ("a", "A"), ("b1", "B1"), ("b2", "B2")])
def test_import_refuses_a_changed_point_of_a_copied_section(sec, label):
    k1, response = _chain("tiny")[3], _three("tiny")[1]
    f = bm.parse(response)
    pb, other = (128, OTHER_G2) if sec == "b2" else (64, OTHER_G1)
    for idx in (0, len(f[sec]) - 1):
        bad = _put(response, f["at"][sec] + pb * idx, other)
        _refused(lambda: zkp_amd.zkey_import_bellman(k1, bad), "mpcparams: %s point %d is not the key's" % (label, idx))


def test_import_refuses_what_is_not_the_next_contribution_to_the_key():
    k0, k1, k2 = _chain("tiny")[2:5]
    challenge, response = _three("tiny")[:2]
    at = bm.parse(response)["at"]
    imp = zkp_amd.zkey_import_bellman
    _refused(lambda: imp(k1, _put(response, at["cs_hash"] + 9, bytes([response[at["cs_hash"] + 9] ^ 1]))),
             "mpcparams: csHash is not the key's")
    # a response to another first contribution: its earlier contribution is not k1's
    other = zkp_amd.zkey_contribute_entropy(k0, "another first", rand64=RAND_B)
    foreign = zkp_amd.zkey_bellman_contribute(zkp_amd.zkey_export_bellman(other), ENTROPY, rand64=RAND_B)
    _refused(lambda: imp(k1, foreign), "mpcparams: contribution 0 is not the key's")
    # two contributions at once, none at all, and a response to a later key of the chain
    twice = zkp_amd.zkey_bellman_contribute(response, "again", rand64=RAND_B)
    _refused(lambda: imp(k1, twice), "mpcparams: contributions: the response has 3, the key has 1")
    _refused(lambda: imp(k1, challenge), "mpcparams: contributions: the response has 1, the key has 1")
    _refused(lambda: imp(k0, response), "mpcparams: contributions: the response has 2, the key has 0")
    _refused(lambda: imp(k1, _put(response, at["delta1"], OTHER_G1)),
             "mpcparams: delta1 is not the new contribution's deltaAfter")
    for hdr, other in (("alpha1", OTHER_G1), ("beta1", OTHER_G1), ("beta2", OTHER_G2), ("gamma2", OTHER_G2)):
        _refused(lambda: imp(k1, _put(response, at[hdr], other)), "mpcparams: %s is not the key's" % hdr)
    # another circuit's counts
    _refused(lambda: imp(k1, _three("small")[1]), "mpcparams: IC has 27 points, the key wants 3")


@pytest.mark.parametrize("sec,label,idx", [("h", "H", 4), ("l", "L", 8), ("h", "H", 14), ("l", "L", 0)])
def test_a_point_off_the_curve_is_named_by_section_and_index(monkeypatch, sec, label, idx):
    """ZKP_PTAU_CHUNK = 4: points 4 and 8 sit just after a chunk border, 14 in a ragged last chunk"""
    k1 = _chain("tiny")[3]
    challenge, response = _three("tiny")[:2]
    text = "mpcparams: %s point %d is not on the curve" % (label, idx)
    monkeypatch.setenv("ZKP_PTAU_CHUNK", "4")
    for f, call in ((challenge, lambda b: zkp_amd.zkey_bellman_contribute(b, ENTROPY, rand64=RAND_B)),
                    (response, lambda b: zkp_amd.zkey_import_bellman(k1, b))):
        m = bm.parse(f)
        x, y = m[sec][idx]
        bad = _put(f, m["at"][sec] + 64 * idx, mpc.g1_u((x, (y + 1) % P)))
        _refused(lambda: call(bad), text)
        # a coordinate that is not canonical (x + p names the same residue) is refused in the same words, and of two
        # bad points the smaller index is named
        if x + P < 1 << 256:
            two = _put(bad, m["at"][sec] + 64 * idx, (x + P).to_bytes(32, "big") + y.to_bytes(32, "big"))
            last = len(m[sec]) - 1
            if last != idx:
                two = _put(two, m["at"][sec] + 64 * last, mpc.g1_u((x, (y + 1) % P)))
            _refused(lambda: call(two), "mpcparams: %s point %d is not on the curve" % (label, min(idx, last)))


def test_contribute_refuses_bad_points_of_the_copied_sections():
    challenge = _three("tiny")[0]
    m = bm.parse(challenge)
    call = lambda b: zkp_amd.zkey_bellman_contribute(b, ENTROPY, rand64=RAND_B)  # noqa: E731
    x, y = m["a"][1]
    _refused(lambda: call(_put(challenge, m["at"]["a"] + 64, mpc.g1_u((x, (y + 1) % P)))),
             "mpcparams: A point 1 is not on the curve")
    j = max(i for i, q in enumerate(m["b2"]) if q is not None)
    (x0, x1), (y0, y1) = m["b2"][j]
    _refused(lambda: call(_put(challenge, m["at"]["b2"] + 128 * j, mpc.g2_u(((x0, x1), ((y0 + 1) % P, y1))))),
             "mpcparams: B2 point %d is not on the curve" % j)
    x, y = m["delta1"]
    _refused(lambda: call(_put(challenge, m["at"]["delta1"], mpc.g1_u((x, (y + 1) % P)))),
             "mpcparams: delta1 is not on the curve")


def test_truncated_files_and_wrong_counts():
    k1 = _chain("tiny")[3]
    challenge, response = _three("tiny")[:2]
    at = bm.parse(response)["at"]
    for cut in (100, 575, 577, at["h"] + 3, at["cs_hash"] + 63, -1):
        _refused(lambda: zkp_amd.zkey_import_bellman(k1, response[:cut]), "mpcparams: the file ends inside")
        _refused(lambda: zkp_amd.zkey_bellman_contribute(challenge[:cut], ENTROPY, rand64=RAND_B),
                 "mpcparams: the file ends inside")
    _refused(lambda: zkp_amd.zkey_import_bellman(k1, response + b"\0"), "mpcparams: 1 trailing bytes")
    # a count that says one point more than the file holds
    more = _put(response, at["ic"] - 4, struct.pack(">I", 4))
    _refused(lambda: zkp_amd.zkey_import_bellman(k1, more), "mpcparams:")
    # a truncated key is refused by export and by import
    _refused(lambda: zkp_amd.zkey_export_bellman(k1[:-5]), "")
    _refused(lambda: zkp_amd.zkey_import_bellman(k1[:-5], response), "")


# ------------------------------------------------------------------ verify on an imported key

def _tampered(edit):
    z = copy.deepcopy(binfile.read_zkey(_three("tiny")[3]))
    edit(z)
    return binfile.write_zkey(z)


def test_verify_still_catches_tampering_of_an_imported_key():
    k0 = _chain("tiny")[2]

    def h_point(z):
        z.h[3] = bn254.g1_mul(z.h[3], 2)

    def h_last(z):
        z.h[-1] = bn254.g1_mul(z.h[-1], 2)

    def l_point(z):
        z.c[4] = bn254.g1_mul(z.c[4], 2)

    def pok(z):
        c = z.extra["mpc"]["contributions"][-1]
        c["g1_sx"] = bn254.g1_mul(c["g1_sx"], 2)

    for edit, text in ((h_point, H_MSG), (h_last, H_MSG), (l_point, L_MSG), (pok, "INVALID(1): inconsistent transcript")):
        for seed in (SEED, SEED_B):
            assert zkp_amd.zkey_verify_frominit(k0, _tampered(edit), seed=seed) == (False, text)


def test_verify_does_not_see_the_w_direction():
    """H' + (w^j T)_j for a fixed point T is accepted: no prover's sum over H has a component there"""
    k0 = _chain("tiny")[2]
    w, t = setup.ROOTS[4], G1B.mul(0xC0FFEE)

    def shift(z):
        z.h = [bn254.g1_add(h, bn254.g1_mul(t, pow(w, j, R))) for j, h in enumerate(z.h)]

    key = _tampered(shift)
    assert key != _three("tiny")[3]
    assert zkp_amd.zkey_verify_frominit(k0, key, seed=SEED) == OK
    assert zkp_amd.zkey_verify_frominit(k0, key, seed=SEED_B) == OK
    # and a proof made with such a key is the proof the imported key gives
    wt = binfile.write_wtns(_setup_case("tiny")[1])
    assert zkp_amd.Prover(key).prove_raw(wt, r=11, s=13) == zkp_amd.Prover(_three("tiny")[3]).prove_raw(wt, r=11, s=13)

    def shift_other(z):  # the same multiples along another vector: caught
        z.h = [bn254.g1_add(h, bn254.g1_mul(t, pow(w, 2 * j, R))) for j, h in enumerate(z.h)]

    assert zkp_amd.zkey_verify_frominit(k0, _tampered(shift_other), seed=SEED) == (False, H_MSG)


@pytest.mark.parametrize("chunk", [1, 5])
def test_verify_chunk_borders_do_not_show_in_the_h_rule(monkeypatch, chunk):
    """ZKP_VERIFY_CHUNK: the power sum takes each chunk's offset w^start; the last point alone in its chunk"""
    k0, new = _chain("tiny")[2], _three("tiny")[3]
    monkeypatch.setenv("ZKP_VERIFY_CHUNK", str(chunk))
    assert zkp_amd.zkey_verify_frominit(k0, new, seed=SEED) == OK
    assert zkp_amd.zkey_verify_frominit(k0, _chain("tiny")[4], seed=SEED) == OK

    def h_point(z):
        z.h[7] = bn254.g1_mul(z.h[7], 3)

    assert zkp_amd.zkey_verify_frominit(k0, _tampered(h_point), seed=SEED) == (False, H_MSG)


# ------------------------------------------------------------------ chunks, timings

@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_chunk_borders_do_not_show(monkeypatch, chunk):
    k1 = _chain("tiny")[3]
    want = _three("tiny")
    monkeypatch.setenv("ZKP_PTAU_CHUNK", str(chunk))
    challenge = zkp_amd.zkey_export_bellman(k1)
    assert zkp_amd.zkey_bellman_timings()["chunks"] == sum(-(-c // chunk) for c in (3, 15, 9, 12, 12, 12))
    response, h = zkp_amd.zkey_bellman_contribute(challenge, ENTROPY, rand64=RAND_B, with_hash=True)
    new = zkp_amd.zkey_import_bellman(k1, response, name=NAME)
    assert (challenge, response, h, new) == want


def test_timings_of_each_command():
    k1 = _chain("small")[3]
    challenge = zkp_amd.zkey_export_bellman(k1)
    t = zkp_amd.zkey_bellman_timings()
    assert t["transform"] > 0 and t["coset_scale"] > 0 and t["encode"] > 0 and t["point_check"] > 0 and t["total"] > 0
    assert t["chunks"] == 6 and t["scale"] == 0 and t["decode"] == 0
    response = zkp_amd.zkey_bellman_contribute(challenge, ENTROPY, rand64=RAND_B)
    t = zkp_amd.zkey_bellman_timings()
    assert t["decode"] > 0 and t["scale"] > 0 and t["point_check"] > 0 and t["transform"] == 0 and t["coset_scale"] == 0
    zkp_amd.zkey_import_bellman(k1, response)
    t = zkp_amd.zkey_bellman_timings()
    assert t["transform"] > 0 and t["coset_scale"] > 0 and t["decode"] > 0 and t["chunks"] == 6 and t["total"] > 0


# ------------------------------------------------------------------ group_fft, kernel level

def _points(g2, log_n, seed):
    """2^log_n zkey-layout points, some of them infinity from 4 points on"""
    n = 1 << log_n
    pb = 128 if g2 else 64
    pts = bytearray(synth.points(synth.scalars(seed, 3, n), g2=g2))
    if n >= 4:
        for j in (1, n - 1, n // 2):
            pts[pb * j:pb * (j + 1)] = bytes(pb)
    return bytes(pts)


def _decode(buf, g2):
    pb, dec = (128, bn254.g2_from_lem) if g2 else (64, bn254.g1_from_lem)
    return [dec(buf[pb * i:pb * (i + 1)]) for i in range(len(buf) // pb)]


@pytest.mark.parametrize("g2,log_n", [(False, 0), (False, 1), (False, 4), (False, 9), (False, 11), (True, 2), (True, 8),
                                      (True, 10)])
def test_group_fft_flip_identity_and_round_trip(g2, log_n):
    n = 1 << log_n
    x = _points(g2, log_n, 40 + log_n)
    fwd = zkp_amd.group_fft(x, log_n, g2=g2)
    assert zkp_amd.group_ifft(fwd, log_n, g2=g2) == x
    inv = _decode(zkp_amd.group_ifft(x, log_n, g2=g2), g2)
    mul = bn254.g2_mul if g2 else bn254.g1_mul
    want = [mul(inv[(n - i) % n], n) if inv[(n - i) % n] is not None else None for i in range(n)]
    assert _decode(fwd, g2) == want


def test_group_fft_of_special_vectors():
    w = setup.ROOTS[4]
    p = G1B.mul(77)
    lem = bn254.g1_to_lem
    assert _decode(zkp_amd.group_fft(lem(p) * 16, 4), False) == [G1B.mul(77 * 16)] + [None] * 15
    one = b"".join(lem(p) if j == 5 else bytes(64) for j in range(16))
    assert _decode(zkp_amd.group_fft(one, 4), False) == [G1B.mul(77 * pow(w, 5 * c, R) % R) for c in range(16)]
    assert zkp_amd.group_fft(bytes(64 * 16), 4) == bytes(64 * 16)
    # against the definition, with infinities among the points
    k = [0 if j in (2, 9) else 1000 + 37 * j for j in range(16)]
    x = b"".join(lem(G1B.mul(v)) if v else bytes(64) for v in k)
    want = [sum(pow(w, c * j, R) * k[j] for j in range(16)) % R for c in range(16)]
    assert _decode(zkp_amd.group_fft(x, 4), False) == [G1B.mul(v) if v else None for v in want]
