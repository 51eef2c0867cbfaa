"""The general XYZZ addition (csrc/curve.hpp xyzz_add) in its doubling and cancellation branches, in every
stage after the buckets are filled: the designed inputs of tests/helpers/msm_designs.py replayed on the host
by tools/hosttest/msm_emu, which adds in the device's order (the shuffle butterfly and the workgroup trees
included) and counts, per stage, how often an addition took an exceptional branch (curve.hpp ZKP_XYZZ_EVENT).

For every design, curve and width: the replay equals the oracle's MSM, the engine's geometry is the one the
design was computed for, and the event table holds the (stage, level, kind) the design aims at -- which
certifies the inputs that tests/test_gpu_xyzz_events.py runs on the GPU.  Every stage and level is aimed at
by some design, for G1 and G2.  Three mutants of xyzz_add (built from a copy of the headers with one exact
text replaced) must make every design that aims at the mutated branch disagree with the oracle.  CPU-only."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import msm_designs as md  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")
CURVES = ["g1", "g2"]

MUTANTS = {
    # name: (old text in curve.hpp, new text, the kind a design must aim at to be judged (None: every design))
    "dbl_returns_infinity": ("      ZKP_XYZZ_EVENT(XYZZ_EV_DBL);\n      acc = xyzz_dbl(acc);",
                             "      ZKP_XYZZ_EVENT(XYZZ_EV_DBL);\n      acc = xyzz_inf<F>();", "dbl"),
    "cancel_doubles": ("    } else {\n      ZKP_XYZZ_EVENT(XYZZ_EV_CANCEL);\n      acc = xyzz_inf<F>();",
                       "    } else {\n      ZKP_XYZZ_EVENT(XYZZ_EV_CANCEL);\n      acc = xyzz_dbl(acc);", "cancel"),
    # every design is certified below to add an infinity to a running sum in some stage after the accumulation
    "q_inf_not_skipped": ("  if (xyzz_is_inf(q)) {\n    ZKP_XYZZ_EVENT(XYZZ_EV_Q_INF);\n    return;\n  }",
                          "  if (xyzz_is_inf(q)) {\n    ZKP_XYZZ_EVENT(XYZZ_EV_Q_INF);\n  }", None),
}


def _start_build(hipcc, root, out):
    return subprocess.Popen([hipcc, "-O1", "-std=c++17", os.path.join(root, "tools", "hosttest", "msm_emu.cpp"),
                             os.path.join(root, "zk-p2p-onramp_amd", "csrc", "host_ec.cpp"), "-o", out],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    """the replay and its three mutants, built side by side: {name: executable}, the replay under None"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    base = tmp_path_factory.mktemp("xyzz_emu")
    exe = {None: str(base / "msm_emu")}
    procs = {None: _start_build(hipcc, ROOT, exe[None])}
    for name, (old, new, _) in MUTANTS.items():
        root = base / name
        csrc = root / "zk-p2p-onramp_amd" / "csrc"
        os.makedirs(csrc)
        os.makedirs(root / "tools" / "hosttest")
        for f in os.listdir(CSRC):
            if f.endswith(".hpp") or f == "host_ec.cpp":
                shutil.copy(os.path.join(CSRC, f), csrc)
        shutil.copy(os.path.join(HT, "msm_emu.cpp"), root / "tools" / "hosttest")
        txt = open(csrc / "curve.hpp").read()
        assert txt.count(old) == 1, "the mutation must match exactly once: " + name
        open(csrc / "curve.hpp", "w").write(txt.replace(old, new))
        exe[name] = str(base / ("msm_emu_" + name))
        procs[name] = _start_build(hipcc, str(root), exe[name])
    for name, p in procs.items():
        out = p.communicate(timeout=1800)[0]
        assert p.returncode == 0, "building %s failed:\n%s" % (name or "msm_emu", out[-3000:])
    return exe


def _run(exe, tmp_path, pts, design, geo, events=True):
    p, s, n = pts.encode(design, geo.c)
    f = tmp_path / "design.bin"
    f.write_bytes(p + s)
    out = subprocess.run([exe, pts.curve, str(f), str(n)] + geo.emu_args() + (["--events"] if events else []),
                         capture_output=True, text=True, check=True, timeout=300).stdout
    return md.parse_emu(out)


POINTS = {}


def _points(curve):
    if curve not in POINTS:
        POINTS[curve] = md.Points(curve)
    return POINTS[curve]


REPLAYS = {}   # (curve, config) -> [(design, result, events)]: replayed once, shared by the tests below


def _replays(emus, tmp_path, curve, cfg):
    if (curve, cfg) not in REPLAYS:
        geo, pts, rows = md.Geometry(*cfg), _points(curve), []
        for d in md.designs(geo):
            line, res, ev = _run(emus[None], tmp_path, pts, d, geo)
            assert line == geo.line(len(d.entries)), "the engine's geometry moved: the designs no longer collide"
            rows.append((d, res, ev))
        REPLAYS[curve, cfg] = rows
    return REPLAYS[curve, cfg]


@pytest.mark.parametrize("cfg", md.CONFIGS, ids=["c%d-d%d-seg%d" % c for c in md.CONFIGS])
@pytest.mark.parametrize("curve", CURVES)
def test_designs_reach_their_branches(emus, tmp_path, curve, cfg):
    geo, pts = md.Geometry(*cfg), _points(curve)
    for d, res, ev in _replays(emus, tmp_path, curve, cfg):
        assert res == pts.expected(d, geo.c), (d.name, "the replay differs from the oracle")
        for stage, kind in d.targets:
            assert ev.get(stage, {}).get(kind, 0) >= 1, (d.name, stage, kind, "the design misses its branch")
        # (what the third mutant is judged by) some running sum after the accumulation meets an infinity
        assert any(v["q_inf"] for s, v in ev.items() if s != "accumulate"), d.name


@pytest.mark.parametrize("curve", CURVES)
def test_every_stage_is_targeted(emus, tmp_path, curve):
    hit = set()
    for cfg in md.CONFIGS:
        for d, _, ev in _replays(emus, tmp_path, curve, cfg):
            hit |= {(s, k) for s, k in d.targets if ev.get(s, {}).get(k, 0) >= 1}
    missing = [t for t in md.required() if t not in hit]
    assert not missing, missing


@pytest.mark.parametrize("mutant", list(MUTANTS))
@pytest.mark.parametrize("curve", CURVES)
def test_mutant_breaks_every_design_that_targets_it(emus, tmp_path, curve, mutant):
    """each design at the first width that has it"""
    kind, pts, seen, judged = MUTANTS[mutant][2], _points(curve), set(), 0
    for cfg in md.CONFIGS:
        geo = md.Geometry(*cfg)
        for d in md.designs(geo):
            if d.name in seen or not (kind is None or any(k == kind for _, k in d.targets)):
                continue
            seen.add(d.name)
            _, res, _ = _run(emus[mutant], tmp_path, pts, d, geo, events=False)
            assert res != pts.expected(d, geo.c), (d.name, cfg, "agrees with the oracle under the mutant: "
                                                   "the design depends on nothing")
            judged += 1
    assert judged >= 20
