"""`zkey verify` through the C ABI, host side only (no device): the argument checks of
zkp_zkey_verify_frominit / zkp_zkey_verify and of the kernel-level entry points, and malformed keys
(section 10 is attacker-controlled: every length is bounded before it is read), which fail with
ZKP_ERR_FORMAT and a message before any device work."""
import ctypes
import struct

import pytest

from oracle import binfile, circuit, mpc, setup
import zkp_amd

INVALID_ARG, FORMAT = 1, 3
TAU, ALPHA, BETA = 0x1234567890ABCDEF1122334455667788 % mpc.R, 987654321987654321, 555555555555
BEACON = bytes.fromhex("0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20")
RAND64 = bytes(range(7, 71))
# a device ordinal no machine has: a call that reached the device would fail with ZKP_ERR_DEVICE
NO_DEVICE = 1 << 20
_cache = {}


def _keys():
    if not _cache:
        r1cs, _ = circuit.gen_circuit(12, 10, 2, 11)
        z0 = setup.zkey_new(r1cs, TAU, ALPHA, BETA)
        z0.extra["mpc"] = {"cs_hash": mpc.cs_hash(z0, TAU), "contributions": []}
        z1, _ = mpc.contribute_entropy(z0, RAND64, "some entropy text", name="first contribution")
        z2, _ = mpc.beacon(z1, BEACON, 10, name="Final Beacon phase2")
        _cache["k"] = (binfile.write_zkey(z0), binfile.write_zkey(z2))
    return _cache["k"]


def _sections(buf):
    _, secs = binfile.read_binfile(buf, b"zkey", 1)
    return [(sid, bytes(buf[off:off + ln])) for sid, ((off, ln),) in sorted(secs.items())]


def _with_section10(key, sec10):
    return binfile.write_binfile(b"zkey", 1, [(sid, sec10 if sid == 10 else p) for sid, p in _sections(key)])


def _frominit(init, key, seed=bytes(32)):
    """(status, valid, msg, last error) of the raw call; None is a NULL pointer."""
    lib = zkp_amd.load_library()
    u8p = ctypes.POINTER(ctypes.c_uint8)

    def arg(b):
        return (None, 0) if b is None else (ctypes.cast(ctypes.c_char_p(b or b"\0"), u8p), len(b))
    (ip, il), (kp, kl) = arg(init), arg(key)
    sp = None if seed is None else ctypes.cast(ctypes.c_char_p(seed), u8p)
    ok = ctypes.c_int(-1)
    msg = ctypes.create_string_buffer(256)
    st = lib.zkp_zkey_verify_frominit(NO_DEVICE, ip, il, kp, kl, sp, ctypes.byref(ok), msg, 256)
    return st, ok.value, msg.value.decode(), lib.zkp_last_error().decode()


def test_null_pointers_and_zero_lengths_are_invalid_arguments():
    init, key = _keys()
    lib = zkp_amd.load_library()
    for i, k in ((None, key), (init, None), (b"", key), (init, b"")):
        st, _, _, err = _frominit(i, k)
        assert st == INVALID_ARG and err
    u8p = ctypes.POINTER(ctypes.c_uint8)
    kp = ctypes.cast(ctypes.c_char_p(key), u8p)
    ip = ctypes.cast(ctypes.c_char_p(init), u8p)
    assert lib.zkp_zkey_verify_frominit(NO_DEVICE, ip, len(init), kp, len(key), None, None, None, 0) == INVALID_ARG
    ok = ctypes.c_int()
    # zkp_zkey_verify: r1cs, ptau and key each null or empty
    for r, rl, p, pl, k, kl in ((None, 0, ip, 4, kp, len(key)), (ip, 4, None, 0, kp, len(key)), (ip, 4, ip, 4, None, 0),
                                (ip, 0, ip, 4, kp, len(key)), (ip, 4, ip, 0, kp, len(key)), (ip, 4, ip, 4, kp, 0)):
        assert lib.zkp_zkey_verify(NO_DEVICE, r, rl, p, pl, k, kl, None, ctypes.byref(ok), None, 0) == INVALID_ARG
    assert lib.zkp_zkey_verify(NO_DEVICE, ip, 4, ip, 4, kp, len(key), None, None, None, 0) == INVALID_ARG
    # the kernel-level entry points
    out = (ctypes.c_uint8 * 64)()
    o = ctypes.cast(out, u8p)
    n64 = ctypes.c_uint64()
    inf = ctypes.c_int()
    assert lib.zkp_rlc_coeffs(NO_DEVICE, None, 0, 1, o) == INVALID_ARG
    assert lib.zkp_rlc_coeffs(NO_DEVICE, kp, 0, 1, None) == INVALID_ARG
    assert lib.zkp_points_check(NO_DEVICE, 0, None, 1, ctypes.byref(n64), ctypes.byref(n64)) == INVALID_ARG
    assert lib.zkp_points_check(NO_DEVICE, 0, kp, 1, None, ctypes.byref(n64)) == INVALID_ARG
    assert lib.zkp_rlc_g1(NO_DEVICE, None, 0, kp, kp, 1, o, ctypes.byref(inf), o, ctypes.byref(inf)) == INVALID_ARG
    assert lib.zkp_rlc_g1(NO_DEVICE, kp, 0, None, kp, 1, o, ctypes.byref(inf), o, ctypes.byref(inf)) == INVALID_ARG
    assert lib.zkp_rlc_g1(NO_DEVICE, kp, 0, kp, kp, 1, None, ctypes.byref(inf), o, ctypes.byref(inf)) == INVALID_ARG
    assert lib.zkp_zkey_verify_timings(None, 4) == INVALID_ARG


def test_python_wrappers_check_the_seed():
    init, key = _keys()
    with pytest.raises(ValueError):
        zkp_amd.zkey_verify_frominit(init, key, seed=b"short")
    with pytest.raises(ValueError):
        zkp_amd.rlc_g1(bytes(32), 0, bytes(64), bytes(128))


@pytest.mark.parametrize("cut", [8, 200, -1])
def test_truncated_key_is_a_format_error(cut):
    init, key = _keys()
    st, ok, msg, err = _frominit(init, key[:cut])
    assert st == FORMAT and ok == 0 and msg == "" and err


def test_key_without_section_10_is_a_format_error():
    init, key = _keys()
    bare = binfile.write_binfile(b"zkey", 1, [(sid, p) for sid, p in _sections(key) if sid != 10])
    st, ok, _, err = _frominit(init, bare)
    assert st == FORMAT and ok == 0 and "section 10" in err
    st, ok, _, err = _frominit(bare, key)
    assert st == FORMAT and "section 10" in err


def test_section_10_lengths_are_bounded():
    init, key = _keys()
    sec10 = dict(_sections(key))[10]
    # the contribution count runs past the end of the section
    more = sec10[:64] + struct.pack("<I", 3) + sec10[68:]
    huge = sec10[:64] + struct.pack("<I", 0xFFFFFFFF) + sec10[68:]
    # the first contribution's parameter length runs past the end of the section
    o = 68 + 384 + 4
    plen = sec10[:o] + struct.pack("<I", 0x7FFFFFF0) + sec10[o + 4:]
    # a parameter's own length byte runs past the parameters (id 1: name, then its length byte)
    assert sec10[o + 4] == 1
    inner = sec10[:o + 5] + bytes([250]) + sec10[o + 6:]
    short = sec10[:40]
    for bad in (more, huge, plen, inner, short):
        st, ok, _, err = _frominit(init, _with_section10(key, bad))
        assert st == FORMAT and ok == 0 and "section 10" in err, err
    # and the same section in the initial key
    st, _, _, err = _frominit(_with_section10(init, more), key)
    assert st == FORMAT and "section 10" in err
