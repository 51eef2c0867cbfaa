"""`zkey export verificationkey` and `groth16 verify` through the Node host layer: the CLI with snarkjs' argv
shape, and groth16.verify / groth16.verifyBatch / zKey.exportVerificationKey through the module."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
GOLD = os.path.join(ROOT, "tests", "golden")
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                reason="node or addon not available")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def cli(*args, cwd=None):
    return subprocess.run([NODE, os.path.join(JS, "cli.js"), *[str(a) for a in args]], capture_output=True, text=True,
                          timeout=600, cwd=cwd)


def test_cli_export_verificationkey_equals_the_golden_key(tmp_path):
    r = cli("zkey", "export", "verificationkey", os.path.join(GOLD, "circuit_small.zkey"), tmp_path / "vk.json")
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "vk.json").read() == open(os.path.join(GOLD, "vkey_small.json")).read()
    # snarkjs' default output name
    r = cli("zkey", "export", "verificationkey", os.path.join(GOLD, "circuit_tiny.zkey"), cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert json.load(open(tmp_path / "verification_key.json")) == json.load(open(os.path.join(GOLD, "vkey_tiny.json")))


def test_usage_names_both_commands():
    r = cli("nonsense")
    assert r.returncode == 1
    assert "groth16 verify <verification_key.json> <public.json> <proof.json>" in r.stderr
    assert "zkey export verificationkey <circuit.zkey> [verification_key.json]" in r.stderr


@pytest.mark.gpu
def test_cli_export_then_verify_a_golden_proof_and_a_tampered_public(tmp_path):
    r = cli("zkey", "export", "verificationkey", os.path.join(GOLD, "circuit_tiny.zkey"), tmp_path / "vk.json")
    assert r.returncode == 0, r.stderr
    r = cli("groth16", "verify", tmp_path / "vk.json", os.path.join(GOLD, "public_tiny.json"),
            os.path.join(GOLD, "proof_tiny.json"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK!" in r.stdout
    pub = json.load(open(os.path.join(GOLD, "public_tiny.json")))
    pub[0] = str((int(pub[0]) + 1) % R)
    (tmp_path / "bad_public.json").write_text(json.dumps(pub))
    r = cli("groth16", "verify", tmp_path / "vk.json", tmp_path / "bad_public.json", os.path.join(GOLD, "proof_tiny.json"))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Invalid proof" in r.stdout and "OK!" not in r.stdout


@pytest.mark.gpu
def test_module_verify_and_verify_batch():
    code = """
const fs = require('fs');
const z = require('./zk-p2p-onramp_amd/js/groth16.js');
const G = %r;
(async () => {
  const vk = await z.zKey.exportVerificationKey(G + '/circuit_small.zkey');
  const gold = JSON.parse(fs.readFileSync(G + '/vkey_small.json', 'utf-8'));
  const proof = JSON.parse(fs.readFileSync(G + '/proof_small.json', 'utf-8'));
  const pub = JSON.parse(fs.readFileSync(G + '/public_small.json', 'utf-8'));
  const bad = pub.slice(); bad[0] = (BigInt(bad[0]) + 1n).toString();
  const log = [];
  const logger = { info: (m) => log.push('i:' + m), error: (m) => log.push('e:' + m) };
  const out = {
    same: JSON.stringify(vk) === JSON.stringify(gold),
    ok: await z.groth16.verify(vk, pub, proof, logger),
    no: await z.groth16.verify(vk, bad, proof, logger),
    batch: await z.groth16.verifyBatch(vk, [{publicSignals: pub, proof}, {publicSignals: bad, proof},
                                           {publicSignals: pub, proof}]),
    log,
  };
  try { await z.groth16.verifyBatch(vk, [{publicSignals: pub.slice(1), proof}]); out.count = 'accepted'; }
  catch (e) { out.count = e.message; }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
""" % GOLD
    r = subprocess.run([NODE, "-e", code], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["same"] is True
    assert out["ok"] is True and out["no"] is False
    assert out["batch"] == [True, False, True]
    assert out["log"] == ["i:OK!", "e:Invalid proof"]
    assert out["count"] == "Invalid number of public signals"
