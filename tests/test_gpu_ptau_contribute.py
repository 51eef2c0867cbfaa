"""`powersoftau new | contribute | beacon` on the GPU (zkp_ptau_contribute, zkp_ptau_beacon, csrc/ptau_contribute.hip)
and its kernel on its own (zkp_points_scale_powers): every point times its own scalar against bn254.g1_mul /
g2_mul, the files byte for byte against tests/helpers/ptau_model.py, across chunk boundaries, and a whole
phase-1 chain through zkp_ptau_prepare_phase2 and zkp_ptau_verify."""
import functools
import os
import sys

import pytest

from oracle import binfile, bn254, mpc
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

P, R = bn254.P, bn254.R
OK = (True, "OK")
RAND64 = bytes((37 * i + 11) & 0xFF for i in range(64))
RAND64_B = bytes((91 * i + 5) & 0xFF for i in range(64))
SEEDS = [bytes(range(100, 132)), bytes(range(3, 35))]
# the hash of the reference script (generate_keys_phase1.sh:18): 31 bytes
BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
FIRST = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % R
RATIO = 0x2b1f3c5d7e9a0b1c2d3e4f5061728394a5b6c7d8e9fa0b1c2d3e4f5061728394 % R
ENC = {False: bn254.g1_to_lem, True: bn254.g2_to_lem}
DEC = {False: bn254.g1_from_lem, True: bn254.g2_from_lem}
MUL = {False: bn254.g1_mul, True: bn254.g2_mul}


def _g2(sid):
    return sid in (3, 6, 13)


def _sections(buf):
    _, secs = binfile.read_binfile(buf, b"ptau", 1)
    return {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items()}


def _file(secs):
    return binfile.write_binfile(b"ptau", 1, sorted(secs.items()))


# ------------------------------------------------------------------ zkp_points_scale_powers

@functools.lru_cache(maxsize=None)
def _base_points(g2):
    """64 distinct points of the group"""
    base = bn254.FixedBase(bn254.G2_GEN, g2=True) if g2 else bn254.FixedBase(bn254.G1_GEN)
    return tuple(base.mul(5 + 11 * j) for j in range(64))


def _inputs(g2, n):
    """n points: the 64 tiled (so points repeat), infinity at 1 and at every 17th index"""
    pts = [_base_points(g2)[j % 64] for j in range(n)]
    if n > 2:
        pts[2] = pts[1]
    for j in range(1, n, 17):
        pts[j] = None
    return pts


@functools.lru_cache(maxsize=None)
def _expected(g2, j, s):
    p = _inputs(g2, 257)[j]
    if p is None or s == 0:
        return None
    if s == R - 1:  # -P by negating y: a reference that shares nothing with a ladder
        return (p[0], ((-p[1][0]) % P, (-p[1][1]) % P)) if g2 else (p[0], (-p[1]) % P)
    return MUL[g2](p, s)


CASES = [("random", FIRST, RATIO), ("one", 1, 1), ("minus_one", 1, R - 1), ("ratio_zero", FIRST, 0), ("first_zero", 0, RATIO)]


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("case,first,ratio", CASES, ids=[c[0] for c in CASES])
def test_scale_powers_against_the_oracle(g2, n, case, first, ratio):
    pts = _inputs(g2, 257)[:n]
    got = zkp_amd.points_scale_powers(b"".join(ENC[g2](p) for p in pts), first, ratio, g2=g2)
    pb = 128 if g2 else 64
    assert len(got) == n * pb
    s = first
    for j in range(n):
        # the random scalars differ at every index: check a spread of them, every index of the other cases
        if case != "random" or j < 4 or j % 16 in (0, 1, 15) or j >= n - 3:
            assert got[j * pb:(j + 1) * pb] == ENC[g2](_expected(g2, j, s)), (case, j)
        s = s * ratio % R
    if case == "ratio_zero" and n > 1:
        assert got[pb:] == bytes((n - 1) * pb) and got[:pb] != bytes(pb)
    if case == "first_zero":
        assert got == bytes(n * pb)
    if case == "minus_one" and n >= 64:  # alternating P, -P
        assert got[4 * pb:5 * pb] == ENC[g2](pts[4]) and got[3 * pb:4 * pb] != ENC[g2](pts[3])
        assert DEC[g2](got[3 * pb:4 * pb])[0] == pts[3][0]


def test_scale_powers_across_chunks(monkeypatch):
    n = 4097
    pts = [_base_points(False)[j % 64] for j in range(n)]
    raw = b"".join(bn254.g1_to_lem(p) for p in _base_points(False)) * 65
    raw = raw[:n * 64]
    monkeypatch.setenv("ZKP_PTAU_CHUNK", "1000")
    got = zkp_amd.points_scale_powers(raw, FIRST, RATIO)
    monkeypatch.delenv("ZKP_PTAU_CHUNK")
    assert zkp_amd.points_scale_powers(raw, FIRST, RATIO) == got
    sample = sorted({0, 1, 2, 63, 64, 999, 1000, 1001, 1999, 2000, 2001, 2999, 3000, 3001, 3999, 4000, 4001, 4095, 4096}
                    | {(j * 211 + 17) % n for j in range(22)})
    assert len(sample) >= 40
    for j in sample:
        want = bn254.g1_mul(pts[j], FIRST * pow(RATIO, j, R) % R)
        assert got[j * 64:(j + 1) * 64] == bn254.g1_to_lem(want), j


def test_scale_powers_refuses_an_off_curve_point():
    pts = list(_base_points(False)[:5])
    pts[3] = (pts[3][0], (pts[3][1] + 1) % P)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.points_scale_powers(b"".join(bn254.g1_to_lem(p) for p in pts), 1, 2)
    assert e.value.status == 1 and "point 3" in e.value.message


# ------------------------------------------------------------------ contribute / beacon against the model

@functools.lru_cache(maxsize=None)
def _model_stage(power, stage):
    """stage 0: new; 1: contributed (RAND64, "first", name "alice"); 2: contributed again (no name)"""
    if stage == 0:
        return pm.new(power)
    if stage == 1:
        return pm.contribute(_model_stage(power, 0), mpc.entropy_rng(RAND64, "first"), "alice")
    return pm.contribute(_model_stage(power, 1), mpc.entropy_rng(RAND64_B, "second"), None)


@pytest.mark.parametrize("power", [1, 2, 3, 5])
def test_contribute_to_a_new_file_equals_the_model(power):
    fresh = zkp_amd.ptau_new(power)
    assert fresh == _model_stage(power, 0)
    got = zkp_amd.ptau_contribute(fresh, "first", rand64=RAND64, name="alice")
    assert got == _model_stage(power, 1)
    t = zkp_amd.ptau_contribute_timings()
    assert t["chunks"] == 5 and t["g1_scale"] > 0 and t["g2_scale"] > 0 and t["encode"] > 0
    assert t["total"] >= t["partial_hash"] > 0 and t["next_challenge"] > 0


@pytest.mark.parametrize("power", [1, 3])
def test_contribute_to_a_contributed_file_equals_the_model(power):
    got = zkp_amd.ptau_contribute(_model_stage(power, 1), "second", rand64=RAND64_B)
    assert got == _model_stage(power, 2)


def test_beacon_equals_the_model():
    got = zkp_amd.ptau_beacon(_model_stage(3, 2), BEACON, 10, name="final beacon")
    assert got == pm.beacon(_model_stage(3, 2), BEACON, 10, "final beacon")
    assert zkp_amd.ptau_beacon(_model_stage(3, 1), BEACON, 10) == pm.beacon(_model_stage(3, 1), BEACON, 10)


def test_chunk_boundaries_inside_every_section(monkeypatch):
    want = _model_stage(3, 2)
    monkeypatch.setenv("ZKP_PTAU_CHUNK", "5")
    got = zkp_amd.ptau_contribute(_model_stage(3, 1), "second", rand64=RAND64_B)
    assert zkp_amd.ptau_contribute_timings()["chunks"] == 3 + 2 + 2 + 2 + 1
    monkeypatch.delenv("ZKP_PTAU_CHUNK")
    assert got == want == zkp_amd.ptau_contribute(_model_stage(3, 1), "second", rand64=RAND64_B)


def test_one_bit_window_gives_the_same_file(monkeypatch):
    monkeypatch.setenv("ZKP_PTAU_WINDOW", "1")
    assert zkp_amd.ptau_contribute(_model_stage(3, 1), "second", rand64=RAND64_B) == _model_stage(3, 2)
    pts = _inputs(True, 65)
    got = zkp_amd.points_scale_powers(b"".join(ENC[True](p) for p in pts), FIRST, RATIO, g2=True)
    monkeypatch.delenv("ZKP_PTAU_WINDOW")
    assert got == zkp_amd.points_scale_powers(b"".join(ENC[True](p) for p in pts), FIRST, RATIO, g2=True)
    monkeypatch.setenv("ZKP_PTAU_WINDOW", "3")
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_contribute(_model_stage(3, 1), "second", rand64=RAND64_B)
    assert e.value.status == 1 and "ZKP_PTAU_WINDOW" in e.value.message


# ------------------------------------------------------------------ the chain

def test_phase1_chain_verifies():
    a = zkp_amd.ptau_contribute(zkp_amd.ptau_new(3), "first", rand64=RAND64, name="alice")
    b = zkp_amd.ptau_contribute(a, "second", rand64=RAND64_B)
    c = zkp_amd.ptau_beacon(b, BEACON, 10, name="final beacon")
    final = zkp_amd.ptau_prepare_phase2(c)
    for seed in SEEDS:
        assert zkp_amd.ptau_verify(final, seed=seed) == OK
    assert pm.verify(c, SEEDS[0]) == OK
    # the sections are tied to the record: another curve point in section 4 is refused
    secs = _sections(a)
    other = bn254.g1_to_lem(bn254.g1_mul(bn254.G1_GEN, 999))
    assert secs[4][:64] != other
    secs[4] = other + secs[4][64:]
    assert zkp_amd.ptau_verify(_file(secs), seed=SEEDS[0])[0] is False


# ------------------------------------------------------------------ input handling

def test_lagrange_sections_are_dropped():
    prepared = zkp_amd.ptau_prepare_phase2(_model_stage(2, 1))
    assert sorted(_sections(prepared)) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    got = zkp_amd.ptau_contribute(prepared, "second", rand64=RAND64_B)
    assert sorted(_sections(got)) == [1, 2, 3, 4, 5, 6, 7]
    assert got == pm.contribute(_model_stage(2, 1), mpc.entropy_rng(RAND64_B, "second"), None)


@pytest.mark.parametrize("chunk", [None, "4"], ids=["default", "chunk4"])
def test_off_curve_point_names_its_section_and_index(monkeypatch, chunk):
    """chunk 4: section 2 is four chunks and section 3 point 5 is local index 1 of that section's second chunk, on
    the odd slot; the refusal is thrown with a chunk in flight on the other slot and the hashing thread live"""
    if chunk:
        monkeypatch.setenv("ZKP_PTAU_CHUNK", chunk)
    secs = _sections(_model_stage(3, 1))
    x = bytearray(secs[3])
    x[5 * 128 + 64] ^= 1  # y.c0 of point 5
    secs[3] = bytes(x)
    y = bytearray(secs[5])
    y[2 * 64 + 32] ^= 1
    secs[5] = bytes(y)
    for call in (lambda b: zkp_amd.ptau_contribute(b, "e", rand64=RAND64), lambda b: zkp_amd.ptau_beacon(b, BEACON, 10)):
        with pytest.raises(zkp_amd.ZkpError) as e:
            call(_file(secs))
        assert e.value.status == 3 and e.value.message == "ptau: section 3 point 5 is not on the curve"


def test_os_randomness_gives_different_files_that_verify():
    fresh = zkp_amd.ptau_new(2)
    a = zkp_amd.ptau_contribute(fresh, "same entropy")
    b = zkp_amd.ptau_contribute(fresh, "same entropy")
    assert a != b and len(a) == len(b)
    for f in (a, b):
        assert zkp_amd.ptau_verify(f, seed=SEEDS[0]) == OK
