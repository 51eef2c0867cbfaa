"""`powersoftau export challenge | challenge contribute | import response` through the Node host layer: the
commands of the reference circuit/scripts/generate_keys_phase1.sh:6-20 in its own argument shapes through cli.js
at power 3 (new, two contributions, the third by challenge and response, verify, beacon, prepare phase2, verify),
every one exiting 0 with the contribution names in order; the addon's importResponse against the Python
binding's; the usage on a wrong argument count; snarkjs' error line for another curve."""
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
OK_LINES = ["[INFO]  snarkJS: Powers Of tau file OK!"]


def _cli(*args):
    return subprocess.run([NODE, os.path.join(JS, "cli.js")] + list(args), capture_output=True, text=True, timeout=600)


def test_node_cli_runs_the_reference_phase1_script(tmp_path):
    p = {n: str(tmp_path / n) for n in ("pot_0000.ptau", "pot_0001.ptau", "pot_0002.ptau", "challenge_0003", "response_0003",
                                        "pot_0003.ptau", "pot_beacon.ptau", "pot_final.ptau", "x")}
    steps = [
        ("powersoftau", "new", "bn128", "3", p["pot_0000.ptau"], "-v"),
        ("powersoftau", "contribute", p["pot_0000.ptau"], p["pot_0001.ptau"], "--name=First contribution", "-v",
         "-e=some random text"),
        ("powersoftau", "contribute", p["pot_0001.ptau"], p["pot_0002.ptau"], "--name=Second contribution", "-v",
         "-e=some random text 2"),
        ("powersoftau", "export", "challenge", p["pot_0002.ptau"], p["challenge_0003"]),
        ("powersoftau", "challenge", "contribute", "bn128", p["challenge_0003"], p["response_0003"], "-e=some random text 3"),
        ("powersoftau", "import", "response", p["pot_0002.ptau"], p["response_0003"], p["pot_0003.ptau"],
         "-n=Third contribution name"),
        ("powersoftau", "verify", p["pot_0003.ptau"]),
        ("powersoftau", "beacon", p["pot_0003.ptau"], p["pot_beacon.ptau"], BEACON_HEX, "10", "-n=Final Beacon"),
        ("powersoftau", "prepare", "phase2", p["pot_beacon.ptau"], p["pot_final.ptau"], "-v"),
        ("powersoftau", "verify", p["pot_final.ptau"]),
    ]
    for args in steps:
        r = _cli(*args)
        assert r.returncode == 0, (args, r.stdout + r.stderr)
        if args[1] == "verify":
            assert r.stdout.splitlines() == OK_LINES
    assert os.path.getsize(p["challenge_0003"]) == 384 * 8 + 128 and os.path.getsize(p["response_0003"]) == 192 * 8 + 864
    cons = pm.Ptau.read(open(p["pot_final.ptau"], "rb").read()).contributions
    assert [c.get("name") for c in cons] == ["First contribution", "Second contribution", "Third contribution name",
                                             "Final Beacon"]
    assert [c["type"] for c in cons] == [0, 0, 0, 1]
    # the import is deterministic: the Python binding gives the same file from the same response
    old, response = (open(p[n], "rb").read() for n in ("pot_0002.ptau", "response_0003"))
    assert open(p["pot_0003.ptau"], "rb").read() == zkp_amd.ptau_import_response(old, response, name="Third contribution name")
    assert open(p["challenge_0003"], "rb").read() == zkp_amd.ptau_export_challenge(old)
    # a wrong argument count prints the usage
    for args, line in ((("powersoftau", "export", "challenge", p["pot_0002.ptau"]),
                        "powersoftau export challenge <in.ptau> <challenge>"),
                       (("powersoftau", "challenge", "contribute", "bn128", p["challenge_0003"]),
                        "powersoftau challenge contribute bn128 <challenge> <response>"),
                       (("powersoftau", "import", "response", p["pot_0002.ptau"], p["response_0003"]),
                        "powersoftau import response <old.ptau> <response> <new.ptau>")):
        r = _cli(*args)
        assert r.returncode == 1 and line in r.stderr
    # another curve: snarkjs' error line, exit 1, no file
    r = _cli("powersoftau", "challenge", "contribute", "bls12381", p["challenge_0003"], p["x"])
    assert r.returncode == 1 and r.stdout.splitlines() == ["[ERROR] snarkJS: Error: Curve not supported: bls12381"]
    assert not os.path.exists(p["x"])


def test_addon_import_response_equals_the_python_binding(tmp_path):
    old = zkp_amd.ptau_contribute(zkp_amd.ptau_new(2), "e", rand64=bytes(range(64)), name="a")
    response = zkp_amd.ptau_challenge_contribute(zkp_amd.ptau_export_challenge(old), "f", rand64=bytes(range(1, 65)))
    src, rsp, out, ch = (tmp_path / n for n in ("in.ptau", "response", "out.ptau", "challenge"))
    src.write_bytes(old), rsp.write_bytes(response)
    script = ("const { powersOfTau } = require(%r);"
              "powersOfTau.exportChallenge(%r, %r).then(() => powersOfTau.importResponse(%r, %r, %r, 'b'))"
              ".then(() => process.exit(0), (e) => { console.error(e); process.exit(1); });"
              % (os.path.join(JS, "groth16.js"), str(src), str(ch), str(src), str(rsp), str(out)))
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == zkp_amd.ptau_import_response(old, response, name="b")
    assert ch.read_bytes() == zkp_amd.ptau_export_challenge(old)
    assert zkp_amd.ptau_verify(out.read_bytes(), seed=bytes(32)) == (True, "OK")
