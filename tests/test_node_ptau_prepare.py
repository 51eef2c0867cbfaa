"""`powersoftau prepare phase2` through the Node host layer: `cli.js powersoftau prepare phase2 <in.ptau>
<out.ptau> [-v]` (reference circuit/scripts/generate_keys_phase1.sh:20) writes the oracle's prepared file,
that file feeds `cli.js zkey new`, and a truncated input fails with the message on stderr."""
import os
import shutil
import subprocess

import pytest

from oracle import binfile, circuit, groth16, mpc, setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                 reason="node or addon not available")]
TAU, ALPHA, BETA = 0x1234567890ABCDEF1122334455667788 % groth16.R, 987654321987654321, 555555555555


def _cli(*args):
    return subprocess.run([NODE, os.path.join(JS, "cli.js")] + list(args), capture_output=True, text=True, timeout=600)


def test_node_cli_prepare_phase2(tmp_path):
    r1cs, _ = circuit.gen_circuit(12, 10, 2, 11)
    k = circuit.domain_size_for(r1cs.n_constraints, r1cs.n_public).bit_length() - 1
    assert k + 1 == 5
    want = setup.ptau_known_tau(5, TAU, ALPHA, BETA)
    _, secs = binfile.read_binfile(want, b"ptau", 1)
    stripped = binfile.write_binfile(b"ptau", 1, [(sid, want[secs[sid][0][0]:secs[sid][0][0] + secs[sid][0][1]])
                                                  for sid in range(1, 8)])
    p = {n: str(tmp_path / n) for n in ("in.ptau", "out.ptau", "short.ptau", "none.ptau", "c.r1cs", "k0.zkey")}
    open(p["in.ptau"], "wb").write(stripped)
    r = _cli("powersoftau", "prepare", "phase2", p["in.ptau"], p["out.ptau"], "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(p["out.ptau"], "rb").read() == want
    # the prepared file feeds `zkey new`
    open(p["c.r1cs"], "wb").write(binfile.write_r1cs(r1cs))
    r = _cli("zkey", "new", p["c.r1cs"], p["out.ptau"], p["k0.zkey"])
    assert r.returncode == 0, r.stdout + r.stderr
    z = setup.zkey_new(r1cs, TAU, ALPHA, BETA)
    z.extra["mpc"] = {"cs_hash": mpc.cs_hash(z, TAU), "contributions": []}
    assert open(p["k0.zkey"], "rb").read() == binfile.write_zkey(z)
    # a truncated input: non-zero exit, the message on stderr, no output file
    open(p["short.ptau"], "wb").write(stripped[:len(stripped) // 2])
    r = _cli("powersoftau", "prepare", "phase2", p["short.ptau"], p["none.ptau"])
    assert r.returncode != 0 and "ptau: truncated section" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(p["none.ptau"])
    # a wrong argument count prints the usage
    r = _cli("powersoftau", "prepare", "phase2", p["in.ptau"])
    assert r.returncode == 1 and "powersoftau prepare phase2 <in.ptau> <out.ptau> [-v]" in r.stderr
