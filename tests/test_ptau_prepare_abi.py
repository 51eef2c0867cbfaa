"""`powersoftau prepare phase2` through the C ABI, host side only (no device): the header declares the
three entry points, the built library exports them, the Python binding sets their signatures, and
null arguments and malformed files fail with their status and a message before any device work."""
import ctypes
import os
import re
import struct

import pytest

from oracle import binfile, bn254, setup
import zkp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT, CURVE = 1, 3, 5
NAMES = ("zkp_ptau_prepare_phase2", "zkp_ptau_prepare_timings", "zkp_group_ifft")
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
u8p = ctypes.POINTER(ctypes.c_uint8)
_cache = {}


def _sections():
    if not _cache:
        buf = setup.ptau_known_tau(1, 5, 6, 7)
        _, secs = binfile.read_binfile(buf, b"ptau", 1)
        _cache["s"] = {sid: bytes(buf[off:off + ln]) for sid, ((off, ln),) in secs.items() if sid <= 7}
    return dict(_cache["s"])


def _file(secs, magic=b"ptau"):
    return binfile.write_binfile(magic, 1, sorted(secs.items()))


def _prepare(buf):
    lib = zkp_amd.load_library()
    out, n = u8p(), ctypes.c_size_t()
    st = lib.zkp_ptau_prepare_phase2(NO_DEVICE, ctypes.cast(ctypes.c_char_p(buf), u8p), len(buf), ctypes.byref(out),
                                     ctypes.byref(n))
    return st, lib.zkp_last_error().decode()


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    assert re.search(r"zkp_status\s+zkp_ptau_prepare_phase2\(int device, const uint8_t\* ptau, size_t len, uint8_t\*\* out,\s*"
                     r"size_t\* out_len\);", text)
    assert re.search(r"zkp_status\s+zkp_ptau_prepare_timings\(double\* ms, int n\);", text)
    assert re.search(r"zkp_status\s+zkp_group_ifft\(int device, int g2, const uint8_t\* points, int log_n, uint8_t\* out\);",
                     text)
    assert "generate_keys_phase1.sh:20" in text and "generate_keys_phase2_groth16.sh:7" in text


def test_library_exports_and_binding_signatures():
    lib = zkp_amd.load_library()
    sz = ctypes.c_size_t
    want = {
        "zkp_ptau_prepare_phase2": [ctypes.c_int, u8p, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)],
        "zkp_ptau_prepare_timings": [ctypes.POINTER(ctypes.c_double), ctypes.c_int],
        "zkp_group_ifft": [ctypes.c_int, ctypes.c_int, u8p, ctypes.c_int, u8p],
    }
    for name in NAMES:
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == want[name]
    for name in ("ptau_prepare_phase2", "ptau_prepare_timings", "group_ifft"):
        assert callable(getattr(zkp_amd, name))


def test_null_arguments_are_invalid():
    lib = zkp_amd.load_library()
    buf = _file(_sections())
    bp = ctypes.cast(ctypes.c_char_p(buf), u8p)
    out, n = u8p(), ctypes.c_size_t()
    assert lib.zkp_ptau_prepare_phase2(NO_DEVICE, None, 0, ctypes.byref(out), ctypes.byref(n)) == INVALID_ARG
    assert lib.zkp_ptau_prepare_phase2(NO_DEVICE, bp, len(buf), None, ctypes.byref(n)) == INVALID_ARG
    assert lib.zkp_ptau_prepare_phase2(NO_DEVICE, bp, len(buf), ctypes.byref(out), None) == INVALID_ARG
    assert lib.zkp_ptau_prepare_timings(None, 8) == INVALID_ARG
    assert lib.zkp_group_ifft(NO_DEVICE, 0, None, 0, bp) == INVALID_ARG
    assert lib.zkp_group_ifft(NO_DEVICE, 0, bp, 0, None) == INVALID_ARG
    assert lib.zkp_group_ifft(NO_DEVICE, 0, bp, 29, bp) == INVALID_ARG
    assert lib.zkp_group_ifft(NO_DEVICE, 0, bp, -1, bp) == INVALID_ARG
    with pytest.raises(ValueError):
        zkp_amd.group_ifft(bytes(64), 1)


def test_timings_have_eight_entries():
    t = zkp_amd.ptau_prepare_timings()
    assert list(t) == ["total", "parse_point_check", "upload", "g1_ifft", "g2_ifft", "affine", "download", "launches"]


def test_malformed_files_fail_before_the_device():
    secs = _sections()
    st, err = _prepare(_file(secs, b"xxxx"))
    assert st == FORMAT and err
    for sid in range(1, 8):
        st, err = _prepare(_file({k: v for k, v in secs.items() if k != sid}))
        assert st == FORMAT and "missing section %d" % sid in err
    for sid, cut in ((2, 64), (3, 128), (4, 64), (5, 64), (6, 1)):
        bad = dict(secs)
        bad[sid] = bad[sid][:-cut]
        st, err = _prepare(_file(bad))
        assert st == FORMAT and "section %d" % sid in err, err
    bad = dict(secs)
    bad[1] = struct.pack("<I", 32) + bn254.int_to_le(bn254.R) + secs[1][36:]
    st, err = _prepare(_file(bad))
    assert st == CURVE and err == "ptau: curve is not bn128"
    bad[1] = struct.pack("<I", 48) + secs[1][4:]
    assert _prepare(_file(bad))[0] == FORMAT
    st, err = _prepare(_file(secs)[:-5])
    assert st == FORMAT and err
    # a well-formed file gets as far as the device
    st, err = _prepare(_file(secs))
    assert st not in (0, INVALID_ARG, FORMAT, CURVE), err
