"""The `MPCParams` codec and the bellman entry points through the C ABI, host side only (no device):
zkp_mpcparams_info on files that tests/helpers/bellman_model.py writes (accepted with the right counts; a short
file, a count that overruns, n - 1 not of the form 2^p - 1, sections that disagree and trailing bytes refused with
ZKP_ERR_FORMAT), the header's declarations, the library's exports, the binding's signatures, and what the three
commands and zkp_group_fft refuse before any device work."""
import ctypes
import functools
import os
import re
import struct
import sys

import pytest

from oracle import binfile, bn254
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bellman_model as bm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT = 1, 3
NAMES = ("zkp_group_fft", "zkp_mpcparams_info", "zkp_zkey_export_bellman", "zkp_zkey_bellman_contribute",
         "zkp_zkey_import_bellman", "zkp_zkey_bellman_timings")
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
u8p = ctypes.POINTER(ctypes.c_uint8)
RAND64 = bytes((37 * i + 11) & 0xFF for i in range(64))


def _ptr(buf):
    return ctypes.cast(ctypes.c_char_p(buf), u8p)


@functools.lru_cache(maxsize=None)
def _key():
    return open(os.path.join(ROOT, "tests", "golden", "circuit_tiny.zkey"), "rb").read()


@functools.lru_cache(maxsize=None)
def _file(contributions=0):
    """a file of the model for the golden tiny key (any n - 1 points serve as its H section here)"""
    z = binfile.read_zkey(_key())
    g = bn254.G1_GEN
    c = {"deltaAfter": g, "g1_s": g, "g1_sx": bn254.g1_mul(g, 2), "g2_spx": bn254.G2_GEN, "transcript": bytes(range(64))}
    z.extra["mpc"] = {"cs_hash": bytes(range(64, 128)), "contributions": [c] * contributions}
    return bm.file_bytes(z, z.h[:z.domain_size - 1])


def _info(buf):
    lib = zkp_amd.load_library()
    v = [ctypes.c_uint32(0xFFFFFFFF) for _ in range(4)]
    st = lib.zkp_mpcparams_info(_ptr(buf), len(buf), *[ctypes.byref(x) for x in v])
    return st, lib.zkp_last_error().decode(), [x.value for x in v]


def test_info_accepts_the_models_files():
    z = binfile.read_zkey(_key())
    assert (z.n_public, z.domain_size, z.n_vars) == (2, 16, 12)
    for nc in (0, 1, 3):
        f = _file(nc)
        assert len(f) == 576 + 6 * 4 + 64 * (3 + 15 + 9 + 12 + 12) + 128 * 12 + 64 + 4 + 384 * nc
        assert _info(f) == (0, "", [2, 16, 12, nc])
        assert zkp_amd.mpcparams_info(f) == {"n_public": 2, "domain_size": 16, "n_vars": 12, "n_contributions": nc}
    assert bm.parse(_file(1))["contributions"][0]["transcript"] == bytes(range(64))


def test_info_refuses_a_short_file():
    f = _file(1)
    at = bm.parse(f)["at"]
    for cut, where in ((0, "the header"), (575, "the header"), (576, "IC"), (at["ic"] + 64 * 3 - 1, "IC"), (at["h"] - 1, "H"),
                       (at["l"] + 5, "L"), (at["a"], "A"), (at["b1"] + 64 * 12 - 1, "B1"), (at["b2"] + 1, "B2"),
                       (at["cs_hash"] + 63, "csHash"), (at["contributions"] + 3, "the contributions"),
                       (len(f) - 1, "the contributions")):
        st, err, v = _info(f[:cut])
        assert (st, err) == (FORMAT, "mpcparams: the file ends inside " + where), cut
        assert v == [0xFFFFFFFF] * 4
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.mpcparams_info(f[:-1])
    assert e.value.status == FORMAT


def _with_count(f, sec, n):
    at = bm.parse(f)["at"][sec] - (0 if sec == "contributions" else 4)
    return f[:at] + struct.pack(">I", n) + f[at + 4:]


def test_info_refuses_counts_that_do_not_fit():
    f = _file(1)
    st, err, _ = _info(_with_count(f, "contributions", 2))
    assert (st, err) == (FORMAT, "mpcparams: the file ends inside the contributions")
    assert _info(_with_count(f, "contributions", 0))[:2] == (FORMAT, "mpcparams: 384 trailing bytes")
    st, err, _ = _info(_with_count(f, "b2", 0x7FFFFFFF))  # a count that overruns the file by far
    assert (st, err) == (FORMAT, "mpcparams: the file ends inside B2")
    st, err, _ = _info(_with_count(f, "ic", 0xFFFFFFFF))
    assert (st, err) == (FORMAT, "mpcparams: the file ends inside IC")
    assert _info(f + b"\0")[:2] == (FORMAT, "mpcparams: 1 trailing bytes")
    assert _info(f + f[-384:])[:2] == (FORMAT, "mpcparams: 384 trailing bytes")


def _resized(f, sec, points, pb=64):
    """section `sec` with `points` points (cut, or extended with copies of its first point)"""
    m = bm.parse(f)
    names = ["ic", "h", "l", "a", "b1", "b2", "cs_hash"]
    at, end = m["at"][sec], m["at"][names[names.index(sec) + 1]] - (0 if sec == "b2" else 4)
    body = (f[at:at + pb] * points)[:pb * points] if points > len(m[sec]) else f[at:at + pb * points]
    return f[:at - 4] + struct.pack(">I", points) + body + f[end:]


@pytest.mark.parametrize("points", [14, 16, 17, 0xFFFE])
def test_info_refuses_an_h_section_that_is_no_domain(points):
    st, err, _ = _info(_resized(_file(), "h", points))
    assert (st, err) == (FORMAT, "mpcparams: H has %d points, which is not 2^p - 1 with p <= 27" % points)


def test_info_accepts_other_domains_and_refuses_sections_that_disagree():
    f = _file()
    assert _info(_resized(f, "h", 31)) == (0, "", [2, 32, 12, 0])
    assert _info(_resized(f, "h", 0)) == (0, "", [2, 1, 12, 0])
    assert _info(_resized(f, "b1", 11))[:2] == (FORMAT, "mpcparams: A, B1 and B2 differ in their point counts")
    assert _info(_resized(f, "b2", 13, 128))[:2] == (FORMAT, "mpcparams: A, B1 and B2 differ in their point counts")
    assert _info(_resized(f, "l", 10))[:2] == (FORMAT, "mpcparams: L has 10 points where A and IC want 9")
    assert _info(_resized(f, "ic", 4))[:2] == (FORMAT, "mpcparams: L has 9 points where A and IC want 8")
    assert _info(_resized(_resized(f, "ic", 0), "l", 12))[:2] == (FORMAT, "mpcparams: IC has no point")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    assert re.search(r"zkp_status\s+zkp_group_fft\(int device, int g2, const uint8_t\* points, int log_n, uint8_t\* out\);", text)
    assert re.search(r"zkp_status\s+zkp_mpcparams_info\(const uint8_t\* buf, size_t len, uint32_t\* n_public, "
                     r"uint32_t\* domain_size, uint32_t\* n_vars,\s*uint32_t\* n_contributions\);", text)
    assert re.search(r"zkp_status\s+zkp_zkey_export_bellman\(int device, const uint8_t\* zkey, size_t len, uint8_t\*\* out, "
                     r"size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_zkey_bellman_contribute\(int device, const uint8_t\* challenge, size_t len,\s*"
                     r"const uint8_t\* rand64[^,]*, const char\* entropy, uint8_t\*\* out,\s*size_t\* out_len, "
                     r"uint8_t\* hash64[^)]*\);", text)
    assert re.search(r"zkp_status\s+zkp_zkey_import_bellman\(int device, const uint8_t\* old_zkey, size_t len, "
                     r"const uint8_t\* response,\s*size_t response_len, const char\* name, uint8_t\*\* out, size_t\* out_len\);",
                     text)
    assert re.search(r"zkp_status\s+zkp_zkey_bellman_timings\(double\* ms, int n\);", text)
    # the format's label, the division of labour, and the verify rule
    assert "Formats restated from snarkjs 0.4.22 (parity unpinned); tests/helpers/bellman_model.py" in text
    assert "same-ratio checks are NOT run here" in text
    assert "r' = -w sum_(j<n-1) r_j w^j" in text


def test_library_exports_and_binding_signatures():
    lib = zkp_amd.load_library()
    sz, pp, psz = ctypes.c_size_t, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    want = {
        "zkp_group_fft": [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_int, u8p],
        "zkp_mpcparams_info": [u8p, sz, u32p, u32p, u32p, u32p],
        "zkp_zkey_export_bellman": [ctypes.c_int, u8p, sz, pp, psz],
        "zkp_zkey_bellman_contribute": [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, pp, psz, u8p],
        "zkp_zkey_import_bellman": [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_char_p, pp, psz],
        "zkp_zkey_bellman_timings": [ctypes.POINTER(ctypes.c_double), ctypes.c_int],
    }
    for name in NAMES:
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want[name]
    for name in ("group_fft", "mpcparams_info", "zkey_export_bellman", "zkey_bellman_contribute", "zkey_import_bellman",
                 "zkey_bellman_timings"):
        assert callable(getattr(zkp_amd, name))


def test_timings_have_eleven_entries():
    t = zkp_amd.zkey_bellman_timings()
    assert list(t) == ["total", "parse", "upload", "decode", "point_check", "scale", "transform", "coset_scale", "encode",
                       "download", "chunks"]
    lib = zkp_amd.load_library()
    v = (ctypes.c_double * 12)(*([-1.0] * 12))
    assert lib.zkp_zkey_bellman_timings(v, 12) == 0
    assert v[11] == -1.0 and all(x >= 0 for x in list(v)[:11])
    assert lib.zkp_zkey_bellman_timings(None, 11) == INVALID_ARG


def _export(key):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    st = lib.zkp_zkey_export_bellman(NO_DEVICE, _ptr(key), len(key), ctypes.byref(out), ctypes.byref(n))
    assert not out
    return st, lib.zkp_last_error().decode()


def _contribute(buf):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    h = ctypes.create_string_buffer(64)
    st = lib.zkp_zkey_bellman_contribute(NO_DEVICE, _ptr(buf), len(buf), _ptr(RAND64), b"entropy", ctypes.byref(out),
                                         ctypes.byref(n), ctypes.cast(h, u8p))
    assert not out
    return st, lib.zkp_last_error().decode()


def _import(key, response, name=None):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t(7)
    st = lib.zkp_zkey_import_bellman(NO_DEVICE, _ptr(key), len(key), _ptr(response), len(response), name, ctypes.byref(out),
                                     ctypes.byref(n))
    assert not out
    return st, lib.zkp_last_error().decode()


def test_null_arguments_are_invalid():
    lib = zkp_amd.load_library()
    k, f = _key(), _file(1)
    kp, fp, e64 = _ptr(k), _ptr(f), _ptr(RAND64)
    out, n = u8p(), ctypes.c_size_t()
    o, ln = ctypes.byref(out), ctypes.byref(n)
    v = [ctypes.byref(ctypes.c_uint32()) for _ in range(4)]
    assert lib.zkp_mpcparams_info(None, len(f), *v) == INVALID_ARG
    for i in range(4):
        assert lib.zkp_mpcparams_info(fp, len(f), *[None if j == i else v[j] for j in range(4)]) == INVALID_ARG
    assert lib.zkp_zkey_export_bellman(NO_DEVICE, None, len(k), o, ln) == INVALID_ARG
    assert lib.zkp_zkey_export_bellman(NO_DEVICE, kp, 0, o, ln) == INVALID_ARG
    assert lib.zkp_zkey_export_bellman(NO_DEVICE, kp, len(k), None, ln) == INVALID_ARG
    assert lib.zkp_zkey_export_bellman(NO_DEVICE, kp, len(k), o, None) == INVALID_ARG
    assert lib.zkp_zkey_bellman_contribute(NO_DEVICE, None, len(f), e64, b"e", o, ln, None) == INVALID_ARG
    assert lib.zkp_zkey_bellman_contribute(NO_DEVICE, fp, 0, e64, b"e", o, ln, None) == INVALID_ARG
    assert lib.zkp_zkey_bellman_contribute(NO_DEVICE, fp, len(f), e64, None, o, ln, None) == INVALID_ARG
    assert lib.zkp_zkey_bellman_contribute(NO_DEVICE, fp, len(f), e64, b"e", None, ln, None) == INVALID_ARG
    assert lib.zkp_zkey_bellman_contribute(NO_DEVICE, fp, len(f), e64, b"e", o, None, None) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, None, len(k), fp, len(f), None, o, ln) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, kp, 0, fp, len(f), None, o, ln) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, kp, len(k), None, len(f), None, o, ln) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, kp, len(k), fp, 0, None, o, ln) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, kp, len(k), fp, len(f), None, None, ln) == INVALID_ARG
    assert lib.zkp_zkey_import_bellman(NO_DEVICE, kp, len(k), fp, len(f), None, o, None) == INVALID_ARG
    bp = ctypes.cast(ctypes.create_string_buffer(64), u8p)
    assert lib.zkp_group_fft(NO_DEVICE, 0, None, 0, bp) == INVALID_ARG
    assert lib.zkp_group_fft(NO_DEVICE, 0, bp, 0, None) == INVALID_ARG
    assert lib.zkp_group_fft(NO_DEVICE, 0, bp, 29, bp) == INVALID_ARG
    assert lib.zkp_group_fft(NO_DEVICE, 0, bp, -1, bp) == INVALID_ARG
    assert "group FFT: log_n must be within 0..28" in lib.zkp_last_error().decode()
    assert not out


def test_malformed_inputs_are_refused_before_the_device():
    k, f = _key(), _file(1)
    for call in (_export, lambda b: _import(b, f)):
        st, err = call(k[:-3])
        assert st == FORMAT and err
        st, err = call(b"xxxx" + k[4:])
        assert st == FORMAT and err
    assert _contribute(f[:-1]) == (FORMAT, "mpcparams: the file ends inside the contributions")
    assert _import(k, f + b"\0") == (FORMAT, "mpcparams: 1 trailing bytes")
    # against the golden key (no contribution): a file with the wrong csHash, then with two contributions
    z = binfile.read_zkey(k)
    assert _import(k, f) == (FORMAT, "mpcparams: csHash is not the key's")
    g = bn254.G1_GEN
    c = {"deltaAfter": g, "g1_s": g, "g1_sx": g, "g2_spx": bn254.G2_GEN, "transcript": bytes(64)}
    z.extra["mpc"] = dict(z.extra["mpc"], contributions=[c, c])
    two = bm.file_bytes(z, z.h[:15])
    st, err = _import(k, two)
    assert st == FORMAT and err.startswith("mpcparams: contributions: the response has 2, the key has 0")
    # header points and contribution points off their curves are the host's to refuse
    at = bm.parse(f)["at"]
    bad = bytearray(f)
    bad[at["delta1"] + 63] ^= 1
    assert _contribute(bytes(bad)) == (FORMAT, "mpcparams: delta1 is not on the curve")
    bad = bytearray(f)
    bad[at["contributions"] + 4 + 128 + 63] ^= 1
    assert _contribute(bytes(bad)) == (FORMAT, "mpcparams: contribution 0 g1_sx is not on the curve")
    bad = bytearray(f)
    bad[at["beta2"]:at["beta2"] + 32] = bn254.P.to_bytes(32, "big")
    assert _contribute(bytes(bad)) == (FORMAT, "mpcparams: beta2 is not on the curve")


@pytest.mark.parametrize("value", ["0", "abc", "", "-4"])
def test_malformed_chunk_variable_is_invalid(monkeypatch, value):
    monkeypatch.setenv("ZKP_PTAU_CHUNK", value)
    z = binfile.read_zkey(_key())
    f0 = bm.file_bytes(z, z.h[:15])
    for st, err in (_export(_key()), _contribute(f0)):
        assert st == INVALID_ARG and "ZKP_PTAU_CHUNK" in err


def test_well_formed_inputs_get_as_far_as_the_device():
    z = binfile.read_zkey(_key())
    g = bn254.G1_GEN
    c = {"deltaAfter": z.delta1, "g1_s": g, "g1_sx": g, "g2_spx": bn254.G2_GEN, "transcript": bytes(64)}
    z.extra["mpc"] = dict(z.extra["mpc"], contributions=[c])
    one = bm.file_bytes(z, z.h[:15])
    for st, err in (_export(_key()), _contribute(_file(1)), _import(_key(), one)):
        assert st not in (0, INVALID_ARG, FORMAT), err
