"""`wtns check` through the Node host layer: `cli.js wtns check <circuit.r1cs> <witness.wtns>` exits 0 on a
witness that satisfies its circuit and 1 on one that does not, with the log lines of later snarkjs (recalled,
unpinned) and the verdict between them; wtns.check resolves to a boolean as snarkjs' does, from file names
and from {type: "mem"} inputs; malformed input goes through the CLI's error path."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from oracle import binfile, bn254, circuit

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wtns_check_model as model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "zk-p2p-onramp_amd", "js")
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(JS, "build", "zkp_napi.node")),
                                reason="node or addon not available")


def node(code):
    return subprocess.run([NODE, "-e", code], capture_output=True, text=True, cwd=ROOT, timeout=600)


def _pair(tmp_path):
    """the small circuit, its witness and one with a signal changed -> paths and the model's verdict"""
    r1cs, w = circuit.gen_circuit(200, 230, 26, 21)
    m = list(w)
    m[150] = (m[150] + 1) % bn254.R
    p = {n: str(tmp_path / n) for n in ("c.r1cs", "good.wtns", "bad.wtns")}
    open(p["c.r1cs"], "wb").write(binfile.write_r1cs(r1cs))
    open(p["good.wtns"], "wb").write(binfile.write_wtns(w))
    open(p["bad.wtns"], "wb").write(binfile.write_wtns(m))
    return p, model.verdict(r1cs, m)


def test_addon_wtns_check_checks_arguments(tmp_path):
    """host side only: the functions exist, a non-buffer is a TypeError, a malformed r1cs throws ZKP_ERR_FORMAT
    (code 3) before any device work, and the CLI turns that into its error exit"""
    r = node("const a=require('./zk-p2p-onramp_amd/js/build/zkp_napi.node');"
             "const z=require('./zk-p2p-onramp_amd/js/groth16.js');"
             "let out=[typeof a.wtnsCheck, typeof z.wtns.check, typeof z.wtns.checkDetails];"
             "try{a.wtnsCheck('x')}catch(e){out.push(e.message)}"
             "try{a.wtnsCheck(Buffer.from('not an r1cs file....'), Buffer.alloc(40), 1048576)}catch(e){out.push(e.code)}"
             "console.log(JSON.stringify(out))")
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out[:3] == ["function"] * 3 and "wtnsCheck(r1csBuffer, wtnsBuffer" in out[3] and out[4] == "3"
    junk = tmp_path / "junk.r1cs"
    junk.write_bytes(b"r1cs" + bytes(20))
    r = subprocess.run([NODE, os.path.join(JS, "cli.js"), "wtns", "check", str(junk), str(junk)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 1 and "r1cs" in r.stderr and r.stdout == ""  # the CLI's error path, no verdict line
    r = subprocess.run([NODE, os.path.join(JS, "cli.js"), "wtns", "check", str(junk)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "usage:" in r.stderr


@pytest.mark.gpu
def test_node_cli_wtns_check_and_module_function(tmp_path):
    p, want = _pair(tmp_path)
    assert not want[0] and want[1].startswith("INVALID: constraint ")
    cli = [NODE, os.path.join(JS, "cli.js"), "wtns", "check", p["c.r1cs"]]
    r = subprocess.run(cli + [p["good.wtns"], "-v"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "[INFO]  snarkJS: WITNESS IS CORRECT"
    r = subprocess.run(cli + [p["bad.wtns"]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.splitlines()[-2:] == ["[ERROR] snarkJS: " + want[1], "[ERROR] snarkJS: WITNESS IS NOT CORRECT"]
    r = node("const z=require('./zk-p2p-onramp_amd/js/groth16.js'); const fs=require('fs');"
             "(async()=>{const log=[]; const L={info:(m)=>log.push(m), error:(m)=>log.push(m)};"
             " const a=await z.wtns.check(%r, %r, L);"
             " const b=await z.wtns.check({type:'mem', data: fs.readFileSync(%r)}, {type:'mem', data: fs.readFileSync(%r)}, L);"
             " const d=await z.wtns.checkDetails(%r, %r);"
             " console.log(JSON.stringify([a, b, log, d]))})()"
             ".catch(e=>{console.log(JSON.stringify({err:e.message}));process.exit(1)})"
             % (p["c.r1cs"], p["good.wtns"], p["c.r1cs"], p["bad.wtns"], p["c.r1cs"], p["bad.wtns"]))
    assert r.returncode == 0, r.stdout + r.stderr
    a, b, log, d = json.loads(r.stdout.strip().splitlines()[-1])
    assert a is True and b is False
    assert log == ["WITNESS IS CORRECT", want[1], "WITNESS IS NOT CORRECT"]
    assert (d["valid"], d["message"], d["nBad"], d["firstBad"], d["bad"], d["nConstraints"]) == \
           (False, want[1], want[2], want[3], want[4], 230)
