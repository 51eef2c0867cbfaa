"""`powersoftau export challenge | challenge contribute | import response` on the GPU (zkp_ptau_export_challenge,
zkp_ptau_challenge_contribute, zkp_ptau_import_response; csrc/ptau_challenge.hip) and their kernels on their own
(zkp_points_decompress, zkp_points_from_uncompressed, zkp_field_sqrt).  The three commands in a row must equal
zkp_ptau_contribute byte for byte (the merged code, not only this feature's own model), each intermediate file
must equal tests/helpers/ptau_challenge_model.py, chunk borders must not show, and each refusal names what it
refuses."""
import functools
import os
import sys

import pytest

from oracle import binfile, bn254, mpc
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_challenge_model as cm  # noqa: E402
import ptau_decompress_cases as dc  # noqa: E402
import ptau_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

P = bn254.P
OK = (True, "OK")
RAND = [bytes((37 * i + 11 + 50 * k) & 0xFF for i in range(64)) for k in range(3)]
SEED = bytes(range(100, 132))
BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f")
NAME = "Third contribution name"
SIZES = [1, 63, 64, 65, 257]


@functools.lru_cache(maxsize=None)
def _stage(power, prior):
    """a file with `prior` contributions: alice's, then a beacon"""
    if prior == 0:
        return pm.new(power)
    if prior == 1:
        return pm.contribute(_stage(power, 0), mpc.entropy_rng(RAND[0], "first"), "alice")
    return pm.beacon(_stage(power, 1), BEACON, 10, "a beacon")


@functools.lru_cache(maxsize=None)
def _model_chain(power, prior):
    f = _stage(power, prior)
    challenge = cm.export_challenge(f)
    response = cm.challenge_contribute(challenge, mpc.entropy_rng(RAND[2], "third"))
    return challenge, response, cm.import_response(f, response, NAME)


def _gpu_chain(f):
    challenge = zkp_amd.ptau_export_challenge(f)
    response = zkp_amd.ptau_challenge_contribute(challenge, "third", rand64=RAND[2])
    return challenge, response, zkp_amd.ptau_import_response(f, response, name=NAME)


def _sections(buf):
    _, secs = binfile.read_binfile(buf, b"ptau", 1)
    return {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items()}


# ------------------------------------------------------------------ the three commands against the merged code

@pytest.mark.parametrize("power", [2, 3])
@pytest.mark.parametrize("prior", [0, 1, 2])
def test_three_commands_equal_one_contribute(power, prior):
    f, n = _stage(power, prior), 1 << power
    challenge, response, new = _gpu_chain(f)
    assert new == zkp_amd.ptau_contribute(f, "third", rand64=RAND[2], name=NAME)
    want = _model_chain(power, prior)
    assert len(challenge) == 384 * n + 128 and len(response) == 192 * n + 864
    assert (challenge, response, new) == want
    assert zkp_amd.ptau_verify(new, seed=SEED) == OK


def test_timings_of_each_command():
    f = _stage(2, 1)
    challenge = zkp_amd.ptau_export_challenge(f)
    t = zkp_amd.ptau_challenge_timings()
    assert t["chunks"] == 5 and t["encode"] > 0 and t["hash_threads"] > 0 and t["total"] > 0
    response = zkp_amd.ptau_challenge_contribute(challenge, "third", rand64=RAND[2])
    t = zkp_amd.ptau_challenge_timings()
    assert t["chunks"] == 5 and t["decode"] > 0 and t["g1_scale"] > 0 and t["g2_scale"] > 0 and t["challenge_hash"] > 0
    zkp_amd.ptau_import_response(f, response)
    t = zkp_amd.ptau_challenge_timings()
    assert t["chunks"] == 5 and t["g1_decompress"] > 0 and t["g2_decompress"] > 0 and t["hash_threads"] > 0


@pytest.mark.parametrize("chunk", [3, 5])
def test_chunk_borders_inside_every_section(monkeypatch, chunk):
    """borders inside every section and off the 128-byte Blake2b blocks (32-byte compressed G1 records)"""
    f = _stage(3, 2)
    monkeypatch.setenv("ZKP_PTAU_CHUNK", str(chunk))
    got = _gpu_chain(f)
    assert zkp_amd.ptau_challenge_timings()["chunks"] == sum(-(-c // chunk) for c in (15, 8, 8, 8, 1))
    monkeypatch.delenv("ZKP_PTAU_CHUNK")
    assert got == _gpu_chain(f) == _model_chain(3, 2)


def test_no_name_is_recorded_without_one():
    f = _stage(2, 0)
    _, response, _ = _model_chain(2, 0)
    got = zkp_amd.ptau_import_response(f, response)
    assert got == cm.import_response(f, response, None)
    assert "name" not in pm.Ptau.read(got).contributions[-1]


def test_lagrange_sections_are_dropped():
    f = _stage(2, 1)
    prepared = zkp_amd.ptau_prepare_phase2(f)
    assert sorted(_sections(prepared)) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert _gpu_chain(prepared) == _model_chain(2, 1)


# ------------------------------------------------------------------ the kernels on their own

def _tiled(g2, n):
    return [dc.points(g2)[j % 65] for j in range(n)]


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_decompress_and_decode_good_points(g2, n):
    pts = _tiled(g2, n)
    want = b"".join(dc.lem(p, g2) for p in pts)
    assert zkp_amd.points_decompress(b"".join(dc.comp(p, g2) for p in pts), g2=g2) == (want, 0, None)
    assert zkp_amd.points_from_uncompressed(b"".join(dc.unc(p, g2) for p in pts), g2=g2) == (want, 0, None)


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_each_bad_kind_at_two_indices(g2, n):
    pts = _tiled(g2, n)
    pb = 128 if g2 else 64
    for fn, kinds, enc in ((zkp_amd.points_decompress, dc.bad_compressed(g2), dc.comp),
                           (zkp_amd.points_from_uncompressed, dc.bad_uncompressed(g2), dc.unc)):
        for k, (kind, raw) in enumerate(sorted(kinds.items())):
            where = sorted({(n - 1 - 3 * k) % n, (n // 2 + k) % n})
            rec = [enc(p, g2) for p in pts]
            want = [dc.lem(p, g2) for p in pts]
            for at in where:
                rec[at], want[at] = raw, bytes(pb)
            assert fn(b"".join(rec), g2=g2) == (b"".join(want), len(where), where[0]), (kind, where)


def test_g2_point_outside_the_subgroup_decompresses():
    """on the twist, not of order r: decompression does not complain; the subgroup check is verify's"""
    x = 1
    while True:
        x += 1
        xx = (x, 1)
        y = mpc.f2_sqrt(bn254.f2_add(bn254.f2_mul(bn254.f2_sqr(xx), xx), bn254.B2))
        if y is not None and mpc.g2_mul_full((xx, y), bn254.R) is not None:
            break
    pt = (xx, y)
    assert bn254.g2_on_curve(pt)
    lem = bn254.g2_to_lem(pt)
    assert zkp_amd.points_decompress(pm.g2_c(pt), g2=True) == (lem, 0, None)
    assert zkp_amd.g2_subgroup_check(lem) == (1, 0)


@pytest.mark.parametrize("fq2", [False, True])
def test_field_sqrt(fq2):
    els = dc.fq2_elements() if fq2 else dc.fq_elements()
    roots, sq = zkp_amd.field_sqrt(b"".join((dc.fq2_bytes if fq2 else dc.fq_bytes)(a) for a in els), fq2=fq2)
    dc.check_roots(fq2, els, roots, sq)


# ------------------------------------------------------------------ refusals that need the device

@pytest.mark.parametrize("chunk", [None, "4"], ids=["default", "chunk4"])
def test_challenge_with_an_off_curve_point_names_it(monkeypatch, chunk):
    """chunk 4: section 3 point 5 is local index 1 of that section's second chunk, on the odd slot, and the other
    slot is busy when the refusal is thrown"""
    if chunk:
        monkeypatch.setenv("ZKP_PTAU_CHUNK", chunk)
    challenge = bytearray(_model_chain(3, 1)[0])
    n = 8
    at = 64 + 64 * (2 * n - 1) + 128 * 5  # section 3, point 5
    challenge[at + 127] ^= 1  # y.c0
    later = 64 + 64 * (2 * n - 1) + 128 * n + 64 * n + 64 * 2  # section 5, point 2
    challenge[later + 63] ^= 1
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_challenge_contribute(bytes(challenge), "e", rand64=RAND[0])
    assert (e.value.status, e.value.message) == (3, "challenge: section 3 point 5 is not on the curve")
    # a coordinate of p is refused by the decoding, under the same words
    challenge = bytearray(_model_chain(3, 1)[0])
    challenge[at:at + 32] = P.to_bytes(32, "big")
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_challenge_contribute(bytes(challenge), "e", rand64=RAND[0])
    assert (e.value.status, e.value.message) == (3, "challenge: section 3 point 5 is not on the curve")


@pytest.mark.parametrize("chunk", [None, "4"], ids=["default", "chunk4"])
def test_response_with_a_non_residue_x_names_it(monkeypatch, chunk):
    """chunk 4: section 4 point 6 is in that section's second chunk; the other slot is busy and the hashing thread
    live when the refusal is thrown"""
    if chunk:
        monkeypatch.setenv("ZKP_PTAU_CHUNK", chunk)
    f = _stage(3, 1)
    response = bytearray(_model_chain(3, 1)[1])
    n = 8
    at = 64 + 32 * (2 * n - 1) + 64 * n + 32 * 6  # section 4, point 6
    response[at:at + 32] = dc.non_residue_x(False)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_import_response(f, bytes(response))
    assert (e.value.status, e.value.message) == (3, "response: section 4 point 6 is not a point of the curve")


def test_response_made_for_another_file():
    _, response, _ = _model_chain(3, 1)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_import_response(_stage(3, 2), response)
    assert (e.value.status, e.value.message) == (3, "response: this contribution is not based on the previous hash")


def test_exported_file_must_hash_to_the_chain():
    secs = _sections(_stage(2, 1))
    other = bn254.g1_to_lem(bn254.g1_mul(bn254.G1_GEN, 999))
    secs[4] = other + secs[4][64:]
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.ptau_export_challenge(binfile.write_binfile(b"ptau", 1, sorted(secs.items())))
    assert (e.value.status, e.value.message) == (3, "ptau: sections 2-6 do not hash to the last contribution's nextChallenge")


def test_import_leaves_the_contribution_checks_to_verify():
    """tauG1[1] replaced by another valid compressed point: import accepts it, verify refuses the contribution"""
    f = _stage(3, 1)
    response = bytearray(_model_chain(3, 1)[1])
    other = pm.g1_c(bn254.g1_mul(bn254.G1_GEN, 12345))
    assert bytes(response[64 + 32:64 + 64]) != other
    response[64 + 32:64 + 64] = other
    new = zkp_amd.ptau_import_response(f, bytes(response), name=NAME)
    assert len(pm.Ptau.read(new).contributions) == 2
    assert zkp_amd.ptau_verify(new, seed=SEED) == (False, "INVALID tau*G1. contribution")
