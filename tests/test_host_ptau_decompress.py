"""The per-lane bodies of `powersoftau challenge contribute` / `import response`
(csrc/ptau_decompress_kernels.hpp: square roots in Fq and Fq2, point decompression, decoding of uncompressed
points) replayed on the host by tools/hosttest/ptau_decompress_emu, and compared with host_ec (inside the
replay), with bn254.fq_sqrt / mpc.f2_sqrt and with the Python encodings.  CPU-only: this is the coverage of the
kernels' arithmetic on a machine without a GPU."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_decompress_cases as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("emu") / "ptau_decompress_emu")
    subprocess.run([hipcc, "-O1", "-std=c++17", os.path.join(HT, "ptau_decompress_emu.cpp"),
                    os.path.join(CSRC, "host_ec.cpp"), "-o", out], check=True, timeout=300)
    return out


def _run(emu, tmp_path, mode, what, data, n):
    f = tmp_path / ("%s_%s.bin" % (mode, what))
    f.write_bytes(data)
    out = subprocess.run([emu, mode, what, str(f), str(n)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == n
    return [ln.split() for ln in lines]


@pytest.mark.parametrize("fq2", [False, True])
def test_square_roots(emu, tmp_path, fq2):
    els = dc.fq2_elements() if fq2 else dc.fq_elements()
    data = b"".join((dc.fq2_bytes if fq2 else dc.fq_bytes)(a) for a in els)
    got = _run(emu, tmp_path, "sqrt", "fq2" if fq2 else "fq", data, len(els))
    dc.check_roots(fq2, els, b"".join(bytes.fromhex(g[0]) for g in got), bytes(int(g[1]) for g in got))


@pytest.mark.parametrize("g2", [False, True])
def test_decompression_of_good_points(emu, tmp_path, g2):
    pts = dc.points(g2)
    assert len(pts) == 65 and pts[2] is None and pts[1] == dc.neg_point(pts[0], g2)
    got = _run(emu, tmp_path, "decompress", "g2" if g2 else "g1", b"".join(dc.comp(p, g2) for p in pts), len(pts))
    flags = set()
    for j, p in enumerate(pts):
        assert got[j] == ["0", dc.lem(p, g2).hex(), dc.unc(p, g2).hex()], j
        flags.add(dc.comp(p, g2)[0] & 0xC0)
    assert flags == {0, 0x40, 0x80}
    # the uncompressed form decodes to the same zkey layout
    got = _run(emu, tmp_path, "decode", "g2" if g2 else "g1", b"".join(dc.unc(p, g2) for p in pts), len(pts))
    for j, p in enumerate(pts):
        assert got[j] == ["0", dc.lem(p, g2).hex()], j


@pytest.mark.parametrize("g2", [False, True])
def test_bad_inputs_count_at_their_index(emu, tmp_path, g2):
    pts = dc.points(g2)
    pb = 128 if g2 else 64
    for mode, kinds, enc, cb in (("decompress", dc.bad_compressed(g2), dc.comp, pb // 2),
                                 ("decode", dc.bad_uncompressed(g2), dc.unc, pb)):
        rec = [enc(p, g2) for p in pts[:12]]
        where = {}
        for at, (kind, raw) in zip(range(1, 12), sorted(kinds.items())):
            assert len(raw) == cb, kind
            rec[at], where[at] = raw, kind
        got = _run(emu, tmp_path, mode, "g2" if g2 else "g1", b"".join(rec), len(rec))
        for j in range(len(rec)):
            if j in where:
                assert got[j][0] == "1" and got[j][1] == bytes(pb).hex(), (mode, where[j])
            else:
                assert got[j][:2] == ["0", dc.lem(pts[j], g2).hex()], (mode, j)
