"""`zkey verify` through the Node host layer: `cli.js zkey verify <r1cs> <ptau> <zkey>` (the gate of
the reference's ceremony, circuit/scripts/generate_keys_phase2_groth16.sh:26) on a ceremony the CLI
itself wrote, and zKey.verifyFromInit / verifyFromR1cs resolving to a boolean as snarkjs' do."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                reason="node or addon not available")
BEACON = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20"


def node(code):
    return subprocess.run([NODE, "-e", code], capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_addon_zkey_verify_checks_arguments():
    r = node("const a=require('./zk-p2p-onramp_amd/js/build/zkp_napi.node');"
             "const z=require('./zk-p2p-onramp_amd/js/groth16.js');"
             "let out=[typeof a.zkeyVerify, typeof a.zkeyVerifyFromR1cs, typeof z.zKey.verifyFromR1cs,"
             " typeof z.zKey.verifyFromInit];"
             "try{a.zkeyVerify('x')}catch(e){out.push(e.message)}"
             "try{a.zkeyVerify(Buffer.from('not a zkey file....'), Buffer.alloc(40))}catch(e){out.push(e.code)}"
             "console.log(JSON.stringify(out))")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out[:4] == ["function"] * 4 and "zkeyVerify(initBuffer, zkeyBuffer" in out[4] and out[5] == "3"


def _ceremony(tmp_path):
    """The tiny ceremony of tests/test_node.py through the CLI -> paths of r1cs, ptau, k0, k2."""
    from oracle import binfile, circuit, groth16, setup
    TAU, ALPHA, BETA = 0x1234567890ABCDEF1122334455667788 % groth16.R, 987654321987654321, 555555555555
    r1cs, _ = circuit.gen_circuit(12, 10, 2, 11)
    k = circuit.domain_size_for(r1cs.n_constraints, r1cs.n_public).bit_length() - 1
    p = {n: str(tmp_path / n) for n in ("c.r1cs", "p.ptau", "k0.zkey", "k1.zkey", "k2.zkey")}
    open(p["c.r1cs"], "wb").write(binfile.write_r1cs(r1cs))
    open(p["p.ptau"], "wb").write(setup.ptau_known_tau(k + 1, TAU, ALPHA, BETA))
    cli = [NODE, os.path.join(JS, "cli.js")]
    for st in (["groth16", "setup", p["c.r1cs"], p["p.ptau"], p["k0.zkey"], "-e=x"],
               ["zkey", "contribute", p["k0.zkey"], p["k1.zkey"], "-e=random text", "-n=1st"],
               ["zkey", "beacon", p["k1.zkey"], p["k2.zkey"], BEACON, "10", "-n=Final Beacon phase2"]):
        r = subprocess.run(cli + st, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    return p


def _swap_two_l_points(path_in, path_out):
    from oracle import binfile
    buf = bytearray(open(path_in, "rb").read())
    _, secs = binfile.read_binfile(bytes(buf), b"zkey", 1)
    off, ln = secs[8][0]
    assert ln >= 128 and buf[off:off + 64] != buf[off + 64:off + 128]
    buf[off:off + 64], buf[off + 64:off + 128] = buf[off + 64:off + 128], buf[off:off + 64]
    open(path_out, "wb").write(bytes(buf))


@pytest.mark.gpu
def test_node_cli_zkey_verify_and_verify_from_init(tmp_path):
    p = _ceremony(tmp_path)
    bad = str(tmp_path / "bad.zkey")
    _swap_two_l_points(p["k2.zkey"], bad)
    cli = [NODE, os.path.join(JS, "cli.js"), "zkey", "verify", p["c.r1cs"], p["p.ptau"]]
    r = subprocess.run(cli + [p["k2.zkey"]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "[INFO]  snarkJS: ZKey Ok!"
    r = subprocess.run(cli + [bad], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.splitlines()[-2:] == ["[ERROR] snarkJS: INVALID: L section is not the initial one times delta^-1",
                                          "[ERROR] snarkJS: Invalid zkey"]
    r = node("const z=require('./zk-p2p-onramp_amd/js/groth16.js');"
             "(async()=>{const log=[]; const L={error:(m)=>log.push(m)};"
             " const a=await z.zKey.verifyFromInit(%r, %r);"
             " const b=await z.zKey.verifyFromInit(%r, {type:'mem', data: require('fs').readFileSync(%r)}, L);"
             " const c=await z.zKey.verifyFromR1cs(%r, %r, %r);"
             " console.log(JSON.stringify([a, b, c, log]))})()"
             ".catch(e=>{console.log(JSON.stringify({err:e.message}));process.exit(1)})"
             % (p["k0.zkey"], p["k2.zkey"], p["k0.zkey"], bad, p["c.r1cs"], p["p.ptau"], p["k1.zkey"]))
    assert r.returncode == 0, r.stdout + r.stderr
    a, b, c, log = json.loads(r.stdout.strip().splitlines()[-1])
    assert a is True and b is False and c is True
    assert log == ["INVALID: L section is not the initial one times delta^-1", "Invalid zkey"]
