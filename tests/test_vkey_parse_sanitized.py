"""The verification-key JSON reader (csrc/vkey.cpp) in a stand-alone program (tools/hosttest/vkey_fuzz.cpp) under
AddressSanitizer + UBSan: the three golden keys, every truncation of one of them and a few hundred seeded byte
mutations.  No sanitizer report, and nothing loads whose parsed points fail the load checks.  CPU only; the
program has its own main and is never loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("vf") / "vkey_fuzz")
    srcs = [os.path.join(HT, "vkey_fuzz.cpp")] + [os.path.join(CSRC, f) for f in
                                                  ("vkey.cpp", "host_pairing.cpp", "host_ec.cpp", "zkey_parse.cpp",
                                                   "zkey_io.cpp")]
    # host code only: no device pass, every sanitizer flag behind -Xarch_host
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "--offload-host-only", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", *srcs, "-o", out,
                    "-lz", "-lpthread"], check=True, timeout=900)
    return out


def test_vkey_reader_under_sanitizers(fuzz_bin, golden_dir):
    keys = [os.path.join(golden_dir, "vkey_%s.json" % n) for n in ("tiny", "small", "venmo_mini")]
    r = subprocess.run([fuzz_bin, "20240612", "400", *keys], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    m = re.search(r"vkey_fuzz: (\d+) loaded, (\d+) rejected with ZkpError, (\d+) loaded but unsound", r.stdout)
    assert m, r.stdout
    loaded, rejected, unsound = (int(x) for x in m.groups())
    assert loaded >= 3 and unsound == 0
    assert rejected > 400  # every truncation, and nearly every mutation
