"""`powersoftau new | contribute | beacon` through the C ABI, host side only (no device): the header declares
the entry points, the built library exports them, the Python binding sets their signatures, zkp_ptau_new
equals the model byte for byte, and null arguments, malformed files, a truncated file, a beacon exponent of
64 and a malformed ZKP_PTAU_CHUNK fail with their status before any device work."""
import ctypes
import os
import re
import struct
import sys

import pytest

from oracle import binfile, bn254
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT, CURVE = 1, 3, 5
NAMES = ("zkp_ptau_new", "zkp_ptau_contribute", "zkp_ptau_beacon", "zkp_ptau_contribute_timings", "zkp_points_scale_powers")
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
u8p = ctypes.POINTER(ctypes.c_uint8)
BEACON = bytes(range(1, 33))


def _sections(buf):
    _, secs = binfile.read_binfile(buf, b"ptau", 1)
    return {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items()}


def _file(secs, magic=b"ptau", version=1):
    return binfile.write_binfile(magic, version, sorted(secs.items()))


def _ptr(buf):
    return ctypes.cast(ctypes.c_char_p(buf), u8p)


def _both(buf, exp=10):
    """(status, message) of zkp_ptau_contribute; zkp_ptau_beacon must fail the same way"""
    lib = zkp_amd.load_library()
    res = []
    for beacon in (False, True):
        out, n = u8p(), ctypes.c_size_t(7)
        if beacon:
            st = lib.zkp_ptau_beacon(NO_DEVICE, _ptr(buf), len(buf), _ptr(BEACON), 32, exp, None, ctypes.byref(out), ctypes.byref(n))
        else:
            st = lib.zkp_ptau_contribute(NO_DEVICE, _ptr(buf), len(buf), _ptr(bytes(64)), b"entropy", None, ctypes.byref(out),
                                         ctypes.byref(n))
        assert not out
        res.append((st, lib.zkp_last_error().decode()))
    assert res[0] == res[1]
    return res[0]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    assert re.search(r"zkp_status\s+zkp_ptau_new\(uint32_t power, uint32_t ceremony_power[^,]*,\s*uint8_t\*\* out, size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_contribute\(int device, const uint8_t\* ptau, size_t len, const uint8_t\* rand64[^,]*,"
                     r"\s*const char\* entropy, const char\* name, uint8_t\*\* out, size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_beacon\(int device, const uint8_t\* ptau, size_t len, const uint8_t\* beacon, "
                     r"size_t beacon_len,\s*uint32_t num_iterations_exp, const char\* name, uint8_t\*\* out, size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_contribute_timings\(double\* ms, int n\);", text)
    assert re.search(r"zkp_status\s+zkp_points_scale_powers\(int device, int g2, const uint8_t\* points, size_t n, "
                     r"const uint8_t\* first32,\s*const uint8_t\* ratio32, uint8_t\* out\);", text)
    assert "generate_keys_phase1.sh:6,8,10,18" in text
    # the header states the truncated-file refusal and names the three commands left for later
    assert "truncated file (power < ceremonyPower) is refused" in text
    for cmd in ("export challenge", "challenge contribute", "import"):
        assert cmd in text


def test_library_exports_and_binding_signatures():
    lib = zkp_amd.load_library()
    sz, pp, psz = ctypes.c_size_t, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)
    want = {
        "zkp_ptau_new": [ctypes.c_uint32, ctypes.c_uint32, pp, psz],
        "zkp_ptau_contribute": [ctypes.c_int, u8p, sz, u8p, ctypes.c_char_p, ctypes.c_char_p, pp, psz],
        "zkp_ptau_beacon": [ctypes.c_int, u8p, sz, u8p, sz, ctypes.c_uint32, ctypes.c_char_p, pp, psz],
        "zkp_ptau_contribute_timings": [ctypes.POINTER(ctypes.c_double), ctypes.c_int],
        "zkp_points_scale_powers": [ctypes.c_int, ctypes.c_int, u8p, sz, u8p, u8p, u8p],
    }
    for name in NAMES:
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want[name]
    for name in ("ptau_new", "ptau_contribute", "ptau_beacon", "ptau_contribute_timings", "points_scale_powers"):
        assert callable(getattr(zkp_amd, name))


@pytest.mark.parametrize("power,ceremony", [(1, 0), (2, 0), (3, 0), (4, 0), (2, 5), (3, 3)])
def test_new_equals_the_model(power, ceremony):
    assert zkp_amd.ptau_new(power, ceremony) == pm.new(power, ceremony or None)


def test_new_refuses_powers_out_of_range():
    lib = zkp_amd.load_library()
    for power, ceremony in ((0, 0), (29, 0), (29, 29), (3, 2), (0, 4)):
        out, n = u8p(), ctypes.c_size_t()
        assert lib.zkp_ptau_new(power, ceremony, ctypes.byref(out), ctypes.byref(n)) == INVALID_ARG
        assert not out and lib.zkp_last_error()
    out, n = u8p(), ctypes.c_size_t()
    assert lib.zkp_ptau_new(2, 0, None, ctypes.byref(n)) == INVALID_ARG
    assert lib.zkp_ptau_new(2, 0, ctypes.byref(out), None) == INVALID_ARG


def test_null_arguments_are_invalid():
    lib = zkp_amd.load_library()
    buf = pm.new(1)
    bp, e64 = _ptr(buf), _ptr(bytes(64))
    out, n = u8p(), ctypes.c_size_t()
    o, ln = ctypes.byref(out), ctypes.byref(n)
    assert lib.zkp_ptau_contribute(NO_DEVICE, None, len(buf), e64, b"e", None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_contribute(NO_DEVICE, bp, 0, e64, b"e", None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_contribute(NO_DEVICE, bp, len(buf), e64, None, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_contribute(NO_DEVICE, bp, len(buf), e64, b"e", None, None, ln) == INVALID_ARG
    assert lib.zkp_ptau_contribute(NO_DEVICE, bp, len(buf), e64, b"e", None, o, None) == INVALID_ARG
    assert lib.zkp_ptau_beacon(NO_DEVICE, None, len(buf), e64, 32, 10, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_beacon(NO_DEVICE, bp, 0, e64, 32, 10, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_beacon(NO_DEVICE, bp, len(buf), None, 32, 10, None, o, ln) == INVALID_ARG
    assert lib.zkp_ptau_beacon(NO_DEVICE, bp, len(buf), e64, 32, 10, None, None, ln) == INVALID_ARG
    assert lib.zkp_ptau_beacon(NO_DEVICE, bp, len(buf), e64, 32, 10, None, o, None) == INVALID_ARG
    assert lib.zkp_ptau_contribute_timings(None, 12) == INVALID_ARG
    assert lib.zkp_points_scale_powers(NO_DEVICE, 0, None, 1, e64, e64, bp) == INVALID_ARG
    assert lib.zkp_points_scale_powers(NO_DEVICE, 0, bp, 1, None, e64, bp) == INVALID_ARG
    assert lib.zkp_points_scale_powers(NO_DEVICE, 0, bp, 1, e64, None, bp) == INVALID_ARG
    assert lib.zkp_points_scale_powers(NO_DEVICE, 0, bp, 1, e64, e64, None) == INVALID_ARG
    assert lib.zkp_points_scale_powers(NO_DEVICE, 1, None, 0, e64, e64, None) == 0  # nothing to scale: no device
    assert not out


def test_timings_have_twelve_entries():
    t = zkp_amd.ptau_contribute_timings()
    assert list(t) == ["total", "parse_point_check", "challenge", "key_draw", "upload", "g1_scale", "g2_scale", "encode",
                       "download", "partial_hash", "next_challenge", "chunks"]
    lib = zkp_amd.load_library()
    v = (ctypes.c_double * 13)(*([-1.0] * 13))
    assert lib.zkp_ptau_contribute_timings(v, 13) == 0
    assert v[12] == -1.0 and all(x >= 0 for x in list(v)[:12])


def test_malformed_files_fail_before_the_device():
    secs = _sections(pm.new(2))
    assert sorted(secs) == [1, 2, 3, 4, 5, 6, 7]
    st, err = _both(_file(secs, b"xxxx"))
    assert st == FORMAT and err
    st, err = _both(_file(secs, version=2))
    assert st == FORMAT and "Version" in err
    for sid in range(1, 8):
        st, err = _both(_file({k: v for k, v in secs.items() if k != sid}))
        assert st == FORMAT and "missing section %d" % sid in err, err
    for sid, cut in ((2, 64), (3, 128), (4, 64), (5, 64), (6, 1)):
        bad = dict(secs)
        bad[sid] = bad[sid][:-cut]
        st, err = _both(_file(bad))
        assert st == FORMAT and "section %d" % sid in err, err
        bad[sid] = secs[sid] + bytes(cut)
        st, err = _both(_file(bad))
        assert st == FORMAT and "section %d" % sid in err, err
    hdr = lambda n8, prime, power, cp: struct.pack("<I", n8) + bn254.int_to_le(prime) + struct.pack("<II", power, cp)
    bad = dict(secs)
    bad[1] = hdr(32, bn254.R, 2, 2)
    st, err = _both(_file(bad))
    assert st == CURVE and err == "ptau: curve is not bn128"
    for h in (hdr(48, bn254.P, 2, 2), hdr(32, bn254.P, 29, 29), hdr(32, bn254.P, 2, 1), secs[1][:39]):
        bad[1] = h
        st, err = _both(_file(bad))
        assert st == FORMAT and "section 1" in err, err
    st, err = _both(_file(secs)[:-3])
    assert st == FORMAT and err
    # a well-formed file gets as far as the device
    st, err = _both(_file(secs))
    assert st not in (0, INVALID_ARG, FORMAT, CURVE), err


def test_cut_short_section_7_names_it():
    secs = _sections(pm.new(1))
    for sec7 in (b"\0\0", struct.pack("<I", 1), struct.pack("<I", 1) + bytes(1503), struct.pack("<I", 0) + b"\0"):
        bad = dict(secs)
        bad[7] = sec7
        st, err = _both(_file(bad))
        assert st == FORMAT and "section 7" in err, err


def test_truncated_file_is_refused():
    st, err = _both(pm.new(2, 5))
    assert (st, err) == (INVALID_ARG, "ptau: cannot contribute to a truncated file")


def test_beacon_exponent_64_is_invalid():
    lib = zkp_amd.load_library()
    buf = pm.new(1)
    out, n = u8p(), ctypes.c_size_t()
    for exp in (64, 255, 1 << 20):
        assert lib.zkp_ptau_beacon(NO_DEVICE, _ptr(buf), len(buf), _ptr(BEACON), 32, exp, None, ctypes.byref(out),
                                   ctypes.byref(n)) == INVALID_ARG
        assert "numIterationsExp" in lib.zkp_last_error().decode()
    big = bytes(256)
    assert lib.zkp_ptau_beacon(NO_DEVICE, _ptr(buf), len(buf), _ptr(big), 256, 10, None, ctypes.byref(out),
                               ctypes.byref(n)) == INVALID_ARG


@pytest.mark.parametrize("value", ["0", "abc", "", "-4", "12x", "99999999999"])
def test_malformed_chunk_variable_is_invalid(monkeypatch, value):
    monkeypatch.setenv("ZKP_PTAU_CHUNK", value)
    st, err = _both(pm.new(1))
    assert st == INVALID_ARG and "ZKP_PTAU_CHUNK" in err
    lib = zkp_amd.load_library()
    p = _ptr(bn254.g1_to_lem(bn254.G1_GEN))
    assert lib.zkp_points_scale_powers(NO_DEVICE, 0, p, 1, _ptr(bytes(32)), _ptr(bytes(32)), p) == INVALID_ARG
