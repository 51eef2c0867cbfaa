"""`powersoftau export challenge | challenge contribute | import response` through the C ABI, host side only (no
device): the header declares the entry points, the built library exports them, the Python binding sets their
signatures, and null arguments, a challenge of a length no power gives, a response one byte short, a response
for another challenge, a truncated ptau, a malformed ZKP_PTAU_CHUNK and a key point off its curve fail with
their status and message, with no buffer handed out, before any device work."""
import ctypes
import functools
import os
import re
import sys

import pytest

from oracle import mpc
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_challenge_model as cm  # noqa: E402
import ptau_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT = 1, 3
NAMES = ("zkp_ptau_export_challenge", "zkp_ptau_challenge_contribute", "zkp_ptau_import_response",
         "zkp_ptau_challenge_timings", "zkp_points_decompress", "zkp_points_from_uncompressed", "zkp_field_sqrt")
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
u8p = ctypes.POINTER(ctypes.c_uint8)
RAND64 = bytes((37 * i + 11) & 0xFF for i in range(64))


def _ptr(buf):
    return ctypes.cast(ctypes.c_char_p(buf), u8p)


@functools.lru_cache(maxsize=None)
def _chain():
    """(ptau of power 1 with one contribution, its challenge, a response to it) from the model"""
    f = pm.contribute(pm.new(1), mpc.entropy_rng(RAND64, "first"), "alice")
    challenge = cm.export_challenge(f)
    return f, challenge, cm.challenge_contribute(challenge, mpc.entropy_rng(RAND64, "second"))


def _export(buf):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    st = lib.zkp_ptau_export_challenge(NO_DEVICE, _ptr(buf), len(buf), ctypes.byref(out), ctypes.byref(n))
    assert not out
    return st, lib.zkp_last_error().decode()


def _contribute(buf):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    st = lib.zkp_ptau_challenge_contribute(NO_DEVICE, _ptr(buf), len(buf), _ptr(RAND64), b"entropy", ctypes.byref(out),
                                           ctypes.byref(n))
    assert not out
    return st, lib.zkp_last_error().decode()


def _import(ptau, response, name=None):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    st = lib.zkp_ptau_import_response(NO_DEVICE, _ptr(ptau), len(ptau), _ptr(response), len(response), name, ctypes.byref(out),
                                      ctypes.byref(n))
    assert not out
    return st, lib.zkp_last_error().decode()


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    assert re.search(r"zkp_status\s+zkp_ptau_export_challenge\(int device, const uint8_t\* ptau, size_t len, uint8_t\*\* out, "
                     r"size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_challenge_contribute\(int device, const uint8_t\* challenge, size_t len,\s*"
                     r"const uint8_t\* rand64[^,]*, const char\* entropy, uint8_t\*\* out,\s*size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_import_response\(int device, const uint8_t\* ptau, size_t len, "
                     r"const uint8_t\* response, size_t response_len,\s*const char\* name, uint8_t\*\* out, size_t\* out_len\);",
                     text)
    assert re.search(r"zkp_status\s+zkp_ptau_challenge_timings\(double\* ms, int n\);", text)
    for fn, arg in (("zkp_points_decompress", "compressed"), ("zkp_points_from_uncompressed", "bytes")):
        assert re.search(r"zkp_status\s+%s\(int device, int g2, const uint8_t\* %s, size_t n, uint8_t\* out_lem, "
                         r"uint64_t\* n_bad,\s*uint64_t\* first_bad\);" % (fn, arg), text)
    assert re.search(r"zkp_status\s+zkp_field_sqrt\(int device, int fq2, const uint8_t\* in, size_t n, uint8_t\* out, "
                     r"uint8_t\* is_square\);", text)
    assert "generate_keys_phase1.sh:12-14" in text
    assert "left for later" not in text
    # what the header must say about the division of labour
    assert "same-ratio checks of the contribution are NOT run here" in text
    assert "snarkjs only logs this" in text


def test_library_exports_and_binding_signatures():
    lib = zkp_amd.load_library()
    sz, pp, psz = ctypes.c_size_t, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    want = {
        "zkp_ptau_export_challenge": [ctypes.c_int, u8p, sz, pp, psz],
        "zkp_ptau_challenge_contribute": [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, pp, psz],
        "zkp_ptau_import_response": [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_char_p, pp, psz],
        "zkp_ptau_challenge_timings": [ctypes.POINTER(ctypes.c_double), ctypes.c_int],
        "zkp_points_decompress": [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u64p, u64p],
        "zkp_points_from_uncompressed": [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u64p, u64p],
        "zkp_field_sqrt": [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u8p],
    }
    for name in NAMES:
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want[name]
    for name in ("ptau_export_challenge", "ptau_challenge_contribute", "ptau_import_response", "ptau_challenge_timings",
                 "points_decompress", "points_from_uncompressed", "field_sqrt"):
        assert callable(getattr(zkp_amd, name))


def test_timings_have_fourteen_entries():
    t = zkp_amd.ptau_challenge_timings()
    assert list(t) == ["total", "parse_point_check", "challenge_hash", "key", "upload", "decode", "g1_decompress",
                       "g2_decompress", "g1_scale", "g2_scale", "encode", "download", "hash_threads", "chunks"]
    lib = zkp_amd.load_library()
    v = (ctypes.c_double * 15)(*([-1.0] * 15))
    assert lib.zkp_ptau_challenge_timings(v, 15) == 0
    assert v[14] == -1.0 and all(x >= 0 for x in list(v)[:14])
    assert lib.zkp_ptau_challenge_timings(None, 14) == INVALID_ARG


def test_null_arguments_are_invalid():
    lib = zkp_amd.load_library()
    f, ch, rs = _chain()
    fp, cp, rp, e64 = _ptr(f), _ptr(ch), _ptr(rs), _ptr(RAND64)
    out, n = u8p(), ctypes.c_size_t()
    o, ln = ctypes.byref(out), ctypes.byref(n)
    assert lib.zkp_ptau_export_challenge(NO_DEVICE, None, len(f), o, ln) == INVALID_ARG
    assert lib.zkp_ptau_export_challenge(NO_DEVICE, fp, 0, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_export_challenge(NO_DEVICE, fp, len(f), None, ln) == INVALID_ARG
    assert lib.zkp_ptau_export_challenge(NO_DEVICE, fp, len(f), o, None) == INVALID_ARG
    assert lib.zkp_ptau_challenge_contribute(NO_DEVICE, None, len(ch), e64, b"e", o, ln) == INVALID_ARG
    assert lib.zkp_ptau_challenge_contribute(NO_DEVICE, cp, 0, e64, b"e", o, ln) == INVALID_ARG
    assert lib.zkp_ptau_challenge_contribute(NO_DEVICE, cp, len(ch), e64, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_challenge_contribute(NO_DEVICE, cp, len(ch), e64, b"e", None, ln) == INVALID_ARG
    assert lib.zkp_ptau_challenge_contribute(NO_DEVICE, cp, len(ch), e64, b"e", o, None) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, None, len(f), rp, len(rs), None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, fp, 0, rp, len(rs), None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, fp, len(f), None, len(rs), None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, fp, len(f), rp, 0, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, fp, len(f), rp, len(rs), None, None, ln) == INVALID_ARG
    assert lib.zkp_ptau_import_response(NO_DEVICE, fp, len(f), rp, len(rs), None, o, None) == INVALID_ARG
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    b, fi = ctypes.byref(bad), ctypes.byref(first)
    for fn in (lib.zkp_points_decompress, lib.zkp_points_from_uncompressed):
        assert fn(NO_DEVICE, 0, None, 1, fp, b, fi) == INVALID_ARG
        assert fn(NO_DEVICE, 0, cp, 1, None, b, fi) == INVALID_ARG
        assert fn(NO_DEVICE, 0, cp, 1, fp, None, fi) == INVALID_ARG
        assert fn(NO_DEVICE, 0, cp, 1, fp, b, None) == INVALID_ARG
        assert fn(NO_DEVICE, 1, None, 0, None, b, fi) == 0 and bad.value == 0  # nothing to do: no device
    assert lib.zkp_field_sqrt(NO_DEVICE, 0, None, 1, fp, fp) == INVALID_ARG
    assert lib.zkp_field_sqrt(NO_DEVICE, 0, cp, 1, None, fp) == INVALID_ARG
    assert lib.zkp_field_sqrt(NO_DEVICE, 0, cp, 1, fp, None) == INVALID_ARG
    assert lib.zkp_field_sqrt(NO_DEVICE, 1, None, 0, None, None) == 0
    assert not out


def test_field_sqrt_refuses_a_coordinate_of_p_before_the_device():
    lib = zkp_amd.load_library()
    buf = (5).to_bytes(32, "little") + pm.P.to_bytes(32, "little")
    out = ctypes.create_string_buffer(64)
    for fq2, n in ((0, 2), (1, 1)):
        assert lib.zkp_field_sqrt(NO_DEVICE, fq2, _ptr(buf), n, ctypes.cast(out, u8p), ctypes.cast(out, u8p)) == INVALID_ARG
        assert ">= p" in lib.zkp_last_error().decode()


@pytest.mark.parametrize("length", [384 * 3 + 128, 384 * 2 + 127, 384 + 128, 128, 64, 384 * 6 + 128])
def test_challenge_length_must_give_a_power(length):
    st, err = _contribute(bytes(length))
    assert st == FORMAT and err.startswith("challenge: a file of %d bytes" % length)


def test_response_one_byte_short():
    f, _, rs = _chain()
    assert _import(f, rs[:-1]) == (FORMAT, "response: size of the contribution is invalid")
    assert _import(f, rs + b"\0") == (FORMAT, "response: size of the contribution is invalid")


def test_response_for_another_challenge():
    f, _, rs = _chain()
    for at in (0, 63):
        bad = bytearray(rs)
        bad[at] ^= 1
        assert _import(f, bytes(bad)) == (FORMAT, "response: this contribution is not based on the previous hash")
    # a file without contributions answers the first challenge of its ceremony
    assert _import(pm.new(1), rs) == (FORMAT, "response: this contribution is not based on the previous hash")


def test_truncated_file_is_refused():
    _, _, rs = _chain()
    trunc = pm.new(2, 5)
    assert _export(trunc) == (INVALID_ARG, "ptau: cannot export the challenge of a truncated file")
    assert _import(trunc, rs) == (INVALID_ARG, "ptau: cannot import a response into a truncated file")


def test_malformed_old_file_is_refused():
    f, _, rs = _chain()
    for call in (_export, lambda b: _import(b, rs)):
        st, err = call(f[:-3])
        assert st == FORMAT and err
        st, err = call(b"xxxx" + f[4:])
        assert st == FORMAT and err


@pytest.mark.parametrize("value", ["0", "abc", "", "-4", "12x", "99999999999"])
def test_malformed_chunk_variable_is_invalid(monkeypatch, value):
    f, ch, rs = _chain()
    monkeypatch.setenv("ZKP_PTAU_CHUNK", value)
    for st, err in (_export(f), _contribute(ch), _import(f, rs)):
        assert st == INVALID_ARG and "ZKP_PTAU_CHUNK" in err
    lib = zkp_amd.load_library()
    bad, first = ctypes.c_uint64(), ctypes.c_uint64()
    out = ctypes.create_string_buffer(128)
    for fn in (lib.zkp_points_decompress, lib.zkp_points_from_uncompressed):
        assert fn(NO_DEVICE, 0, _ptr(ch), 1, ctypes.cast(out, u8p), ctypes.byref(bad), ctypes.byref(first)) == INVALID_ARG
    assert lib.zkp_field_sqrt(NO_DEVICE, 0, _ptr(bytes(32)), 1, ctypes.cast(out, u8p), ctypes.cast(out, u8p)) == INVALID_ARG


@pytest.mark.parametrize("k", range(9))
def test_key_point_off_its_curve(k):
    f, _, rs = _chain()
    at = len(rs) - 768 + (64 * k if k < 6 else 384 + 128 * (k - 6))
    size = 64 if k < 6 else 128
    bad = bytearray(rs)
    bad[at + size - 1] ^= 1  # the last byte of y (G2: of y.c0)
    assert _import(f, bytes(bad)) == (FORMAT, "response: key point %d is not on the curve" % k)
    bad = bytearray(rs)
    bad[at:at + 32] = pm.P.to_bytes(32, "big")
    assert _import(f, bytes(bad)) == (FORMAT, "response: key point %d is not canonical" % k)
    bad = bytearray(rs)
    bad[at] |= 0x40
    assert _import(f, bytes(bad)) == (FORMAT, "response: key point %d is not canonical" % k)


def test_well_formed_inputs_get_as_far_as_the_device():
    f, ch, rs = _chain()
    for st, err in (_export(f), _contribute(ch), _import(f, rs)):
        assert st not in (0, INVALID_ARG, FORMAT), err
