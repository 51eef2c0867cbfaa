"""The G2 subgroup check's per-thread body (csrc/g2_subgroup_kernels.hpp, what ptau_verify.hip's k_g2_subgroup
runs per point) compiled for the host by tools/hosttest/g2_subgroup_emu and compared with host::g2_in_subgroup
and with the oracle's arithmetic: points of G2, infinity, and points of the twist outside G2, one of them of
the small order 10069 that a sum-only check would miss with probability 1 / 10069.  CPU-only."""
import os
import shutil
import subprocess
import sys

import pytest

from oracle import bn254

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import g2_twist  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")
R = bn254.R


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("emu") / "g2_subgroup_emu")
    subprocess.run([hipcc, "-O1", "-std=c++17", os.path.join(HT, "g2_subgroup_emu.cpp"), os.path.join(CSRC, "host_ec.cpp"),
                    os.path.join(CSRC, "host_pairing.cpp"), "-o", out], check=True, timeout=600)
    return out


def _run(emu, tmp_path, pts):
    f = tmp_path / "pts.bin"
    f.write_bytes(b"".join(bn254.g2_to_lem(p) for p in pts))
    lines = subprocess.run([emu, str(f), "--events"], capture_output=True, text=True, check=True,
                           timeout=300).stdout.strip().split("\n")
    assert len(lines) == len(pts) + 1
    ev = tuple(int(x) for x in lines[-1].split()[1:5])
    return [tuple(int(x) for x in ln.split()) for ln in lines[:-1]], ev


def test_the_small_order_point_is_what_it_claims():
    q, t = g2_twist.q_point(), g2_twist.t_point()
    assert bn254.g2_on_curve(q) and g2_twist.mul_any(q, R) is not None
    assert g2_twist.mul_any(t, 10069) is None and g2_twist.mul_any(t, R) is not None


def test_kernel_body_agrees_with_the_host_and_the_oracle(emu, tmp_path):
    G = bn254.G2_GEN
    q, t = g2_twist.q_point(), g2_twist.t_point()
    inside = [bn254.g2_mul(G, k) for k in (1, 2, 3, 12345, R - 1, 0x1234567890ABCDEF1122334455667788 % R)]
    outside = [q, t, bn254.g2_add(bn254.g2_mul(G, 12345), t), g2_twist.mul_any(t, 2), g2_twist.mul_any(q, R)]
    pts = inside + [None] + outside
    want = [1] * (len(inside) + 1) + [0] * len(outside)
    for p, w in zip(pts, want):  # the oracle's own verdict: [r]P = infinity
        assert (p is None or g2_twist.mul_any(p, R) is None) == bool(w)
    got, ev = _run(emu, tmp_path, pts)
    assert [g[0] for g in got] == want  # the kernel's body
    assert [g[1] for g in got] == want  # host::g2_in_subgroup
    # every good finite point ends its ladder in a cancellation ([r - 1]P + P); the accumulators start at infinity
    assert ev[1] >= len(inside) and ev[2] >= len(pts) - 1
