"""The per-lane bodies of `powersoftau contribute` (csrc/ptau_scale_kernels.hpp: power table, lane scalar,
ladder, affine conversion, the three encodings) replayed on the host by tools/hosttest/ptau_scale_emu as one
launch of k_scale_powers, and compared with host_ec (inside the replay), with bn254.g1_mul / g2_mul and with
the Python encodings (bn254.g1_to_lem, mpc.g1_u, ptau_model.g1_c and their G2 forms).  CPU-only: this is the
coverage of the kernels' arithmetic on a machine without a GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from oracle import bn254, mpc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")
R = bn254.R
N = 65
START = (1 << 27) + 5
RANDOM = 0x2b1f3c5d7e9a0b1c2d3e4f5061728394a5b6c7d8e9fa0b1c2d3e4f5061728394 % R
FIRST = 0x1d2c3b4a59687766554433221100ffeeddccbbaa99887766554433221100abcd % R
ENC = {"g1": (bn254.g1_to_lem, mpc.g1_u, ptau_model.g1_c, bn254.g1_mul),
       "g2": (bn254.g2_to_lem, mpc.g2_u, ptau_model.g2_c, bn254.g2_mul)}
_points = {}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("emu") / "ptau_scale_emu")
    subprocess.run([hipcc, "-O1", "-std=c++17", os.path.join(HT, "ptau_scale_emu.cpp"), os.path.join(CSRC, "host_ec.cpp"),
                    "-o", out], check=True, timeout=300)
    return out


def _inputs(curve):
    """65 points: distinct multiples of the generator, a repeated one, and three at infinity"""
    if curve not in _points:
        base = bn254.FixedBase(bn254.G1_GEN) if curve == "g1" else bn254.FixedBase(bn254.G2_GEN, g2=True)
        pts = [base.mul(3 + 7 * j) for j in range(N)]
        pts[9] = pts[8]
        for j in (2, 31, 64):
            pts[j] = None
        _points[curve] = pts
    return _points[curve]


def _run(emu, tmp_path, curve, pts, first, ratio, start):
    to_lem = ENC[curve][0]
    f = tmp_path / ("in_%s.bin" % curve)
    f.write_bytes(b"".join(to_lem(p) for p in pts))
    out = subprocess.run([emu, curve, str(f), str(len(pts)), "%x" % first, "%x" % ratio, str(start), "--reencode"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [tuple(bytes.fromhex(h) for h in ln.split()) for ln in out.stdout.strip().split("\n")]


@pytest.mark.parametrize("curve", ["g1", "g2"])
@pytest.mark.parametrize("first,ratio,start", [(1, RANDOM, 0), (FIRST, RANDOM, START), (1, 0, 0), (FIRST, 0, 0), (FIRST, 0, START),
                                               (1, 1, 0), (FIRST, 1, START), (1, R - 1, 0), (FIRST, R - 1, START),
                                               (R - 1, R - 1, 1)])
def test_scaled_points_and_their_three_encodings(emu, tmp_path, curve, first, ratio, start):
    to_lem, unc, comp, mul = ENC[curve]
    pts = _inputs(curve)
    got = _run(emu, tmp_path, curve, pts, first, ratio, start)
    assert len(got) == N
    s = first * pow(ratio, start, R) % R
    seen_inf = seen_pt = 0
    for j, p in enumerate(pts):
        want = None if p is None or s == 0 else mul(p, s)
        assert got[j] == (to_lem(want), unc(want), comp(want)), (j, s)
        seen_inf += want is None
        seen_pt += want is not None
        s = s * ratio % R
    assert seen_inf >= 3
    if ratio or not start:
        assert seen_pt >= 1


@pytest.mark.parametrize("curve", ["g1", "g2"])
def test_compressed_flag_of_both_roots(emu, tmp_path, curve):
    """P and -P (ratio r - 1) differ in the compressed form by the 0x80 flag alone"""
    _, _, comp, _ = ENC[curve]
    P = _inputs(curve)[5]
    got = _run(emu, tmp_path, curve, [P, P], 1, R - 1, 0)
    a, b = got[0][2], got[1][2]
    assert a[1:] == b[1:] and a[0] ^ b[0] == 0x80
    assert a == comp(P)
