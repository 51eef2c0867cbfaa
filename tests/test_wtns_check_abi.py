"""`wtns check` through the C ABI, host side only (no device): the header declares the entry points and
the library exports them, null and empty arguments are ZKP_ERR_INVALID_ARG, and malformed .r1cs / .wtns
files fail with ZKP_ERR_FORMAT / _CURVE / _WITNESS_LENGTH and a message before any device work (the calls
name a device no machine has: one that reached it would answer ZKP_ERR_DEVICE)."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

from oracle import binfile, bn254, circuit
import zkp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, FORMAT, CURVE, WITNESS_LENGTH, DEVICE = 1, 3, 5, 6, 7
NO_DEVICE = 1 << 20
ENTRY_POINTS = ["zkp_checker_load", "zkp_checker_info", "zkp_checker_check", "zkp_checker_check_staged",
                "zkp_checker_free", "zkp_wtns_check", "zkp_wtns_check_timings"]
u8p = ctypes.POINTER(ctypes.c_uint8)


def _files():
    r1cs, w = circuit.gen_circuit(12, 10, 2, 11)
    return binfile.write_r1cs(r1cs), binfile.write_wtns(w)


def _arg(b):
    return (None, 0) if b is None else (ctypes.cast(ctypes.c_char_p(b or b"\0"), u8p), len(b))


def _one_shot(r1cs, wtns, with_res=True):
    """(status, valid, msg, last error) of zkp_wtns_check on a device no machine has"""
    lib = zkp_amd.load_library()
    (rp, rl), (wp, wl) = _arg(r1cs), _arg(wtns)
    res = zkp_amd._CheckResult()
    res.valid = -1
    msg = ctypes.create_string_buffer(256)
    st = lib.zkp_wtns_check(NO_DEVICE, rp, rl, wp, wl, ctypes.byref(res) if with_res else None, msg, 256)
    return st, res.valid, msg.value.decode(), lib.zkp_last_error().decode()


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "zkp_amd.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", zkp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in exported, name
    assert "typedef struct zkp_checker zkp_checker;" in hdr
    # the result struct as the issue states it, and the binding's mirror of it
    assert re.search(r"int valid;\s*uint64_t n_bad, first_bad, n_constraints;\s*uint32_t n_listed;\s*uint64_t bad\[16\];", hdr)
    assert ctypes.sizeof(zkp_amd._CheckResult) == 8 + 3 * 8 + 8 + 16 * 8


def test_null_and_empty_arguments_are_invalid_arguments():
    r1cs, wtns = _files()
    lib = zkp_amd.load_library()
    for r, w in ((None, wtns), (r1cs, None), (b"", wtns), (r1cs, b"")):
        st, _, _, err = _one_shot(r, w)
        assert st == INVALID_ARG and err
    assert _one_shot(r1cs, wtns, with_res=False)[0] == INVALID_ARG
    h = ctypes.c_void_p()
    rp, rl = _arg(r1cs)
    assert lib.zkp_checker_load(NO_DEVICE, None, rl, ctypes.byref(h)) == INVALID_ARG
    assert lib.zkp_checker_load(NO_DEVICE, rp, 0, ctypes.byref(h)) == INVALID_ARG
    assert lib.zkp_checker_load(NO_DEVICE, rp, rl, None) == INVALID_ARG
    res = zkp_amd._CheckResult()
    wp, wl = _arg(wtns)
    assert lib.zkp_checker_info(None, None, None, None, None) == INVALID_ARG
    assert lib.zkp_checker_check(None, wp, wl, ctypes.byref(res), None, 0) == INVALID_ARG
    assert lib.zkp_checker_check_staged(None, None, 0, 0, ctypes.byref(res), None, 0) == INVALID_ARG
    assert lib.zkp_wtns_check_timings(None, 5) == INVALID_ARG
    lib.zkp_checker_free(None)  # a no-op


def test_a_sound_pair_reaches_the_device():
    """the control of the cases below: with both files sound the call goes on to the device it names"""
    r1cs, wtns = _files()
    st, valid, msg, err = _one_shot(r1cs, wtns)
    assert st == DEVICE and valid == 0 and msg == "" and err


def _r1cs_sections(buf):
    _, secs = binfile.read_binfile(buf, b"r1cs", 1)
    return {sid: off for sid, ((off, ln),) in secs.items()}, {sid: ln for sid, ((off, ln),) in secs.items()}


def test_malformed_r1cs_fails_before_the_device():
    r1cs, wtns = _files()
    off, ln = _r1cs_sections(r1cs)
    cases = []
    m = bytearray(r1cs)
    struct.pack_into("<I", m, off[2] + 4, 12)           # a wire index = nWires
    cases.append((m, FORMAT, "wire"))
    cases.append((r1cs[:off[2] + ln[2] - 1], FORMAT, "truncated"))   # a truncated section
    cases.append((r1cs[:40], FORMAT, "truncated"))
    m = bytearray(r1cs)
    struct.pack_into("<I", m, off[1], 48)               # n8 != 32
    cases.append((m, CURVE, "n8"))
    m = bytearray(r1cs)
    m[off[1] + 4:off[1] + 36] = bn254.int_to_le(bn254.P)  # the base field's prime
    cases.append((m, CURVE, "prime"))
    m = bytearray(r1cs)
    struct.pack_into("<I", m, off[2], 0xFFFFFFFF)       # a term count past the section (and past u32 with the next)
    cases.append((m, FORMAT, "truncated"))
    m = bytearray(r1cs)
    struct.pack_into("<I", m, off[1] + 36 + 24, 0x7FFFFFFF)  # nConstraints the section cannot hold
    cases.append((m, FORMAT, "truncated"))
    cases.append((b"zkey" + r1cs[4:], FORMAT, "Invalid File format"))
    for buf, want, word in cases:
        st, valid, msg, err = _one_shot(bytes(buf), wtns)
        assert st == want and valid == 0 and msg == "" and word in err, (want, word, st, err)
    # the loader alone answers the same
    lib = zkp_amd.load_library()
    h = ctypes.c_void_p()
    rp, rl = _arg(r1cs[:40])
    assert lib.zkp_checker_load(NO_DEVICE, rp, rl, ctypes.byref(h)) == FORMAT and not h.value


def test_malformed_wtns_fails_before_the_device():
    r1cs, wtns = _files()
    r, w = circuit.gen_circuit(12, 10, 2, 11)
    short = binfile.write_wtns(w[:-1])
    st, _, _, err = _one_shot(r1cs, short)
    assert st == WITNESS_LENGTH and err == "Invalid witness length. Circuit: 12, witness: 11"
    st, _, _, err = _one_shot(r1cs, wtns[:-1])
    assert st == FORMAT and err
    other = bytearray(wtns)
    _, secs = binfile.read_binfile(wtns, b"wtns", 2)
    (o, _), = secs[1]
    other[o + 4:o + 36] = bn254.int_to_le(bn254.P)
    st, _, _, err = _one_shot(r1cs, bytes(other))
    assert st == CURVE and err
    st, _, _, err = _one_shot(r1cs, r1cs)
    assert st == FORMAT and err


def test_python_wrapper_raises_on_malformed_input():
    r1cs, wtns = _files()
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.wtns_check(r1cs[:100], wtns, device=NO_DEVICE)
    assert e.value.status == FORMAT
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.WitnessChecker(r1cs[:100], device=NO_DEVICE)
    assert e.value.status == FORMAT
