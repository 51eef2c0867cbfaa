"""`powersoftau new | contribute | beacon` through the Node host layer, in the argument shapes of the reference
circuit/scripts/generate_keys_phase1.sh:6,8,10,18: `cli.js powersoftau new bn128 3` -> `contribute` -> `beacon`
-> `verify` exits 0, another curve name exits 1 with snarkjs' error line, and the addon's ptauBeacon output
equals the Python binding's byte for byte."""
import os
import shutil
import subprocess
import sys

import pytest

import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                 reason="node or addon not available")]
BEACON_HEX = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f"  # the script's, 31 bytes


def _cli(*args):
    return subprocess.run([NODE, os.path.join(JS, "cli.js")] + list(args), capture_output=True, text=True, timeout=600)


def test_node_cli_phase1_from_new_to_verify(tmp_path):
    p = {n: str(tmp_path / n) for n in ("pot_0000.ptau", "pot_0001.ptau", "pot_0002.ptau", "pot_beacon.ptau", "x.ptau")}
    r = _cli("powersoftau", "new", "bn128", "3", p["pot_0000.ptau"], "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(p["pot_0000.ptau"], "rb").read() == pm.new(3)
    r = _cli("powersoftau", "contribute", p["pot_0000.ptau"], p["pot_0001.ptau"], "--name=First contribution", "-v",
             "-e=some random text")
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("powersoftau", "contribute", p["pot_0001.ptau"], p["pot_0002.ptau"], "-n=Second contribution")
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("powersoftau", "beacon", p["pot_0002.ptau"], p["pot_beacon.ptau"], BEACON_HEX, "10", "-n=Final Beacon")
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("powersoftau", "verify", p["pot_beacon.ptau"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["[INFO]  snarkJS: Powers Of tau file OK!"]
    cons = pm.Ptau.read(open(p["pot_beacon.ptau"], "rb").read()).contributions
    assert [c.get("name") for c in cons] == ["First contribution", "Second contribution", "Final Beacon"]
    assert [c["type"] for c in cons] == [0, 0, 1] and cons[2]["beaconHash"] == bytes.fromhex(BEACON_HEX)
    # the beacon is deterministic: the Python binding gives the same file
    before = open(p["pot_0002.ptau"], "rb").read()
    assert open(p["pot_beacon.ptau"], "rb").read() == zkp_amd.ptau_beacon(before, bytes.fromhex(BEACON_HEX), 10, name="Final Beacon")
    # another curve: snarkjs' error line, exit 1, no file
    r = _cli("powersoftau", "new", "bls12381", "3", p["x.ptau"])
    assert r.returncode == 1 and "[ERROR] snarkJS" in r.stdout and not os.path.exists(p["x.ptau"])
    # a wrong argument count prints the usage
    r = _cli("powersoftau", "beacon", p["pot_0002.ptau"])
    assert r.returncode == 1 and "powersoftau beacon <in.ptau> <out.ptau> <beaconHashHex> <numIterationsExp>" in r.stderr


def test_addon_beacon_equals_the_python_binding(tmp_path):
    src = tmp_path / "in.ptau"
    src.write_bytes(zkp_amd.ptau_contribute(zkp_amd.ptau_new(2), "e", rand64=bytes(range(64)), name="a"))
    out = tmp_path / "out.ptau"
    script = ("const { powersOfTau } = require(%r);"
              "powersOfTau.beacon(%r, %r, 'b', %r, 10).then(() => process.exit(0), (e) => { console.error(e); process.exit(1); });"
              % (os.path.join(JS, "groth16.js"), str(src), str(out), BEACON_HEX))
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == zkp_amd.ptau_beacon(src.read_bytes(), bytes.fromhex(BEACON_HEX), 10, name="b")
