"""`powersoftau verify` (the point sections) through the C ABI, host side only (no device): the header
declares the entry points, the built library exports them, the Python binding sets their signatures, and
null arguments and malformed files fail with their status and a message that names the section before
any device work."""
import ctypes
import os
import re
import struct

from oracle import binfile, bn254, setup
import zkp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT, CURVE = 1, 3, 5
NAMES = ("zkp_ptau_verify", "zkp_ptau_verify_sections", "zkp_ptau_verify_timings", "zkp_g2_subgroup_check", "zkp_rlc_pairs")
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
u8p = ctypes.POINTER(ctypes.c_uint8)
_cache = {}


def _sections():
    if not _cache:
        buf = setup.ptau_known_tau(1, 5, 6, 7)
        _, secs = binfile.read_binfile(buf, b"ptau", 1)
        _cache["s"] = {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items()}
    return dict(_cache["s"])


def _file(secs, magic=b"ptau", version=1):
    return binfile.write_binfile(magic, version, sorted(secs.items()))


def _verify(buf, cap=256):
    """status and message of zkp_ptau_verify_sections; zkp_ptau_verify must fail the same way"""
    lib = zkp_amd.load_library()
    res = []
    for fn in (lib.zkp_ptau_verify, lib.zkp_ptau_verify_sections):
        ok, msg = ctypes.c_int(7), ctypes.create_string_buffer(cap)
        st = fn(NO_DEVICE, ctypes.cast(ctypes.c_char_p(buf), u8p), len(buf), None, ctypes.byref(ok), msg, cap)
        assert ok.value == 0
        res.append((st, lib.zkp_last_error().decode()))
    if res[1][0] in (FORMAT, CURVE):
        assert res[0] == res[1]
    return res[1]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    assert re.search(r"zkp_status\s+zkp_ptau_verify_sections\(int device, const uint8_t\* ptau, size_t len, const uint8_t\* "
                     r"seed32[^,]*,\s*int\* valid, char\* msg, size_t msg_cap\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_verify\(int device, const uint8_t\* ptau, size_t len, const uint8_t\* "
                     r"seed32[^,]*,\s*int\* valid, char\* msg, size_t msg_cap\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_verify_timings\(double\* ms, int n\);", text)
    assert re.search(r"zkp_status\s+zkp_g2_subgroup_check\(int device, const uint8_t\* points, size_t n, uint64_t\* n_bad, "
                     r"uint64_t\* first_bad\);", text)
    assert re.search(r"zkp_status\s+zkp_rlc_pairs\(int device, int g2, const uint8_t\* seed32, uint64_t first_index, "
                     r"const uint8_t\* points, size_t n,\s*uint8_t\* out_a, int\* inf_a, uint8_t\* out_b, int\* inf_b\);", text)
    assert "generate_keys_phase1.sh:16" in text and "generate_keys_phase2_groth16.sh:3" in text


def test_library_exports_and_binding_signatures():
    lib = zkp_amd.load_library()
    sz, ip, u64p = ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)
    want = {
        "zkp_ptau_verify": [ctypes.c_int, u8p, sz, u8p, ip, ctypes.c_char_p, sz],
        "zkp_ptau_verify_sections": [ctypes.c_int, u8p, sz, u8p, ip, ctypes.c_char_p, sz],
        "zkp_ptau_verify_timings": [ctypes.POINTER(ctypes.c_double), ctypes.c_int],
        "zkp_g2_subgroup_check": [ctypes.c_int, u8p, sz, u64p, u64p],
        "zkp_rlc_pairs": [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_uint64, u8p, sz, u8p, ip, u8p, ip],
    }
    for name in NAMES:
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want[name]
    for name in ("ptau_verify", "ptau_verify_sections", "ptau_verify_timings", "g2_subgroup_check", "rlc_pairs"):
        assert callable(getattr(zkp_amd, name))


def test_null_arguments_are_invalid():
    lib = zkp_amd.load_library()
    buf = _file(_sections())
    bp = ctypes.cast(ctypes.c_char_p(buf), u8p)
    ok, msg = ctypes.c_int(), ctypes.create_string_buffer(64)
    n64, i = ctypes.c_uint64(), ctypes.c_int()
    for fn in (lib.zkp_ptau_verify_sections, lib.zkp_ptau_verify):
        assert fn(NO_DEVICE, None, len(buf), None, ctypes.byref(ok), msg, 64) == INVALID_ARG
        assert fn(NO_DEVICE, bp, 0, None, ctypes.byref(ok), msg, 64) == INVALID_ARG
        assert fn(NO_DEVICE, bp, len(buf), None, None, msg, 64) == INVALID_ARG
    assert lib.zkp_ptau_verify_timings(None, 14) == INVALID_ARG
    assert lib.zkp_g2_subgroup_check(NO_DEVICE, None, 1, ctypes.byref(n64), ctypes.byref(n64)) == INVALID_ARG
    assert lib.zkp_g2_subgroup_check(NO_DEVICE, bp, 1, None, ctypes.byref(n64)) == INVALID_ARG
    assert lib.zkp_g2_subgroup_check(NO_DEVICE, bp, 1, ctypes.byref(n64), None) == INVALID_ARG
    args = [bp, 0, bp, 2, bp, ctypes.byref(i), bp, ctypes.byref(i)]
    for k in (0, 2, 4, 5, 6, 7):
        a = list(args)
        a[k] = None
        assert lib.zkp_rlc_pairs(NO_DEVICE, 0, *a) == INVALID_ARG
    # nothing to sum: no device is needed
    out = (ctypes.c_uint8 * 64)(*([1] * 64))
    o = ctypes.cast(out, u8p)
    for n in (0, 1):
        i.value = 0
        assert lib.zkp_rlc_pairs(NO_DEVICE, 0, bp, 0, bp, n, o, ctypes.byref(i), o, ctypes.byref(i)) == 0
        assert i.value == 1 and bytes(out) == bytes(64)
    assert lib.zkp_g2_subgroup_check(NO_DEVICE, None, 0, ctypes.byref(n64), ctypes.byref(n64)) == 0


def test_timings_have_seventeen_entries():
    t = zkp_amd.ptau_verify_timings()
    assert list(t) == ["total", "parse", "upload", "point_check", "subgroup_check", "coeff_gen", "ntt_scalar_fold", "plan",
                       "accumulate_pairs", "accumulate_lagrange", "accumulate_tau", "host_fold", "host_pairings", "chunks",
                       "contributions", "first_challenge", "next_challenge"]


def test_malformed_files_fail_before_the_device():
    secs = _sections()
    assert sorted(secs) == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    st, err = _verify(_file(secs, b"xxxx"))
    assert st == FORMAT and err
    st, err = _verify(_file(secs, version=2))
    assert st == FORMAT and "Version" in err
    for sid in range(1, 8):
        st, err = _verify(_file({k: v for k, v in secs.items() if k != sid}))
        assert st == FORMAT and "missing section %d" % sid in err, err
    for sid, cut in ((2, 64), (3, 128), (4, 64), (5, 64), (6, 1), (12, 64), (13, 128), (14, 1), (15, 64)):
        bad = dict(secs)
        bad[sid] = bad[sid][:-cut]
        st, err = _verify(_file(bad))
        assert st == FORMAT and "section %d" % sid in err, err
        bad[sid] = secs[sid] + bytes(cut)
        st, err = _verify(_file(bad))
        assert st == FORMAT and "section %d" % sid in err, err
    # sections 12-15 present only in part
    for sid in (12, 13, 14, 15):
        st, err = _verify(_file({k: v for k, v in secs.items() if k != sid}))
        assert st == FORMAT and "missing section %d" % sid in err, err
    hdr = lambda n8, prime, power, cp: struct.pack("<I", n8) + bn254.int_to_le(prime) + struct.pack("<II", power, cp)
    bad = dict(secs)
    bad[1] = hdr(32, bn254.R, 1, 1)
    st, err = _verify(_file(bad))
    assert st == CURVE and err == "ptau: curve is not bn128"
    for h in (hdr(48, bn254.P, 1, 1), hdr(32, bn254.P, 29, 29), hdr(32, bn254.P, 0, 0), hdr(32, bn254.P, 1, 0), secs[1][:39]):
        bad[1] = h
        st, err = _verify(_file(bad))
        assert st == FORMAT and "section 1" in err, err
    bad = dict(secs)
    bad[7] = b"\0\0"
    st, err = _verify(_file(bad))
    assert st == FORMAT and "section 7" in err
    st, err = _verify(_file(secs)[:-5])
    assert st == FORMAT and err
    # a well-formed file, with or without its Lagrange sections, gets as far as the device
    for s in (secs, {k: v for k, v in secs.items() if k <= 7}):
        st, err = _verify(_file(s))
        assert st not in (0, INVALID_ARG, FORMAT, CURVE), err


def test_message_buffer_is_optional_and_cleared():
    lib = zkp_amd.load_library()
    buf = _file({k: v for k, v in _sections().items() if k != 4})
    bp = ctypes.cast(ctypes.c_char_p(buf), u8p)
    ok = ctypes.c_int(5)
    assert lib.zkp_ptau_verify_sections(NO_DEVICE, bp, len(buf), None, ctypes.byref(ok), None, 0) == FORMAT
    msg = ctypes.create_string_buffer(b"junk", 8)
    assert lib.zkp_ptau_verify_sections(NO_DEVICE, bp, len(buf), None, ctypes.byref(ok), msg, 8) == FORMAT
    assert ok.value == 0 and msg.value == b""
