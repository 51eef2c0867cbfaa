"""`zkey export bellman | zkey bellman contribute | zkey import bellman` through the Node host layer: the three
cli.js lines in snarkjs' argument shapes on the tiny circuit's first contributed key, the new key against the
Python binding's, `zkey verify` on it, the contribution hash that -v prints, the usage on a wrong argument count
and snarkjs' error line for another curve."""
import hashlib
import os
import shutil
import subprocess

import pytest

from oracle import binfile
from test_gpu_zkey_verify import _chain
import zkp_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                 reason="node or addon not available")]


def _cli(*args):
    return subprocess.run([NODE, os.path.join(JS, "cli.js")] + list(args), capture_output=True, text=True, timeout=600)


def test_node_cli_runs_the_three_commands(tmp_path):
    r1cs, ptau, _, k1, _ = _chain("tiny")
    p = {n: str(tmp_path / n) for n in ("circuit.r1cs", "pot.ptau", "circuit_0001.zkey", "circuit.mpcparams",
                                        "circuit_response.mpcparams", "circuit_0002.zkey", "x")}
    for n, b in (("circuit.r1cs", r1cs), ("pot.ptau", ptau), ("circuit_0001.zkey", k1)):
        open(p[n], "wb").write(bytes(b))
    r = _cli("zkey", "export", "bellman", p["circuit_0001.zkey"], p["circuit.mpcparams"])
    assert r.returncode == 0, r.stdout + r.stderr
    challenge = open(p["circuit.mpcparams"], "rb").read()
    assert challenge == zkp_amd.zkey_export_bellman(k1)
    r = _cli("zkey", "bellman", "contribute", "bn128", p["circuit.mpcparams"], p["circuit_response.mpcparams"],
             "-e=some random text", "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    response = open(p["circuit_response.mpcparams"], "rb").read()
    assert len(response) == len(challenge) + 384 and zkp_amd.mpcparams_info(response)["n_contributions"] == 2
    h = hashlib.blake2b(response[-384:], digest_size=64).hexdigest()
    rows = ["\t\t" + " ".join(h[32 * i + 8 * j:32 * i + 8 * j + 8] for j in range(4)) for i in range(4)]
    assert r.stdout.splitlines() == ["[INFO]  snarkJS: Contribution Hash: "] + rows
    r = _cli("zkey", "import", "bellman", p["circuit_0001.zkey"], p["circuit_response.mpcparams"], p["circuit_0002.zkey"],
             "--name=Outside contributor", "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    new = open(p["circuit_0002.zkey"], "rb").read()
    assert new == zkp_amd.zkey_import_bellman(k1, response, name="Outside contributor")
    cons = binfile.read_zkey(new).extra["mpc"]["contributions"]
    assert [c.get("name") for c in cons] == ["first contribution", "Outside contributor"]
    r = _cli("zkey", "verify", p["circuit.r1cs"], p["pot.ptau"], p["circuit_0002.zkey"])
    assert r.returncode == 0 and r.stdout.splitlines() == ["[INFO]  snarkJS: ZKey Ok!"], r.stdout + r.stderr
    # a wrong argument count prints the usage
    for args, line in ((("zkey", "export", "bellman", p["circuit_0001.zkey"]),
                        "zkey export bellman <circuit_xxxx.zkey> <circuit.mpcparams>"),
                       (("zkey", "bellman", "contribute", "bn128", p["circuit.mpcparams"]),
                        "zkey bellman contribute bn128 <circuit.mpcparams> <circuit_response.mpcparams>"),
                       (("zkey", "import", "bellman", p["circuit_0001.zkey"], p["circuit_response.mpcparams"]),
                        "zkey import bellman <circuit_old.zkey> <circuit_response.mpcparams> <circuit_new.zkey>")):
        r = _cli(*args)
        assert r.returncode == 1 and line in r.stderr
    # another curve: snarkjs' error line, exit 1, no file
    r = _cli("zkey", "bellman", "contribute", "bls12381", p["circuit.mpcparams"], p["x"])
    assert r.returncode == 1 and r.stdout.splitlines() == ["[ERROR] snarkJS: Error: Curve not supported: bls12381"]
    assert not os.path.exists(p["x"])
