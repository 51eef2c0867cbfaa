"""`wtns check`'s per-lane bodies (csrc/wtns_check_kernels.hpp) and its r1cs reader (csrc/r1cs_parse.cpp)
replayed on the host by tools/hosttest/wtns_check_emu: the short kernel lane by lane, the long kernel's 64
lanes with the device's exchange pattern, the fail bitmap and its scan, on the hard-shape circuit and every
mutation of its witness, against the Python model.  Every constraint goes through BOTH paths in the replay
(the program fails if they disagree), and the threshold between them is tried at several values.  A second
build with AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone executable, host code only) runs
the same inputs, then every prefix and a few hundred one-byte mutations of the tiny r1cs.  CPU-only: this is
the coverage of the kernels' arithmetic and indexing on a machine without a GPU."""
import os
import shutil
import subprocess
import sys

import pytest

from oracle import binfile, bn254, circuit

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wtns_check_model as model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=87")


def _build(tmp_path_factory, name, flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp(name) / "wtns_check_emu")
    subprocess.run([hipcc, "-std=c++17", *flags, os.path.join(HT, "wtns_check_emu.cpp"), "-o", out], check=True, timeout=600)
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build(tmp_path_factory, "emu", ["-O1"])


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    # host code only: every sanitizer flag behind -Xarch_host (no device code is built or run)
    return _build(tmp_path_factory, "emu_san", ["-O1", "-g", "-fno-omit-frame-pointer", "-Xarch_host",
                                                "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the hard circuit, its bad variant and every witness as files; the model's verdict for each"""
    d = tmp_path_factory.mktemp("hard")
    h = model.hard_circuit()
    files = {}
    for name, r1cs in (("good", h.r1cs), ("bad", h.bad_r1cs)):
        files[name] = str(d / (name + ".r1cs"))
        open(files[name], "wb").write(binfile.write_r1cs(r1cs))
    wits = dict(model.mutations(h), good=h.w)
    wits["w0_is_2"] = [2] + h.w[1:]
    unreduced = list(h.w)
    unreduced[len(h.w) // 2] = bn254.R
    wits["unreduced"] = unreduced
    names = sorted(wits)
    paths = []
    for n in names:
        paths.append(str(d / (n + ".bin")))
        open(paths[-1], "wb").write(b"".join(v.to_bytes(32, "little") for v in wits[n]))
    return h, files, names, paths, wits


def _line(v):
    ok, msg, n_bad, first, bad = v
    if ok:
        return "OK"
    if "signal 0" in msg:
        return "W0"
    if "not reduced" in msg:
        return "UNREDUCED %s" % msg.split()[2]
    return "BAD %d %d %s" % (n_bad, first, ",".join(map(str, bad)))


def _run(binary, args, env=None):
    r = subprocess.run([binary, *args], capture_output=True, text=True, timeout=600, env=env and dict(os.environ, **env))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout.strip().split("\n")


# 0: every constraint short; 1: every one long (a wavefront for an empty constraint too); 24: the
# library's switch; 65 and 200: switches inside the hard circuit's run of lengths
@pytest.mark.parametrize("long_terms", [0, 1, 24, 65, 200])
def test_replay_matches_the_model_on_the_hard_circuit(emu, cases, long_terms):
    h, files, names, paths, wits = cases
    got = _run(emu, [files["good"], str(long_terms), *paths])
    assert got == [_line(model.verdict(h.r1cs, wits[n])) for n in names]
    assert got[names.index("good")] == "OK" and got[names.index("all_zero")].startswith("BAD")


def test_replay_matches_the_model_on_the_bad_circuit(emu, cases):
    h, files, names, paths, wits = cases
    i = names.index("good")
    n = h.r1cs.n_constraints
    assert _run(emu, [files["bad"], "24", paths[i]]) == ["BAD 1 %d %d" % (n, n)]


def test_replay_on_generated_circuits(emu, tmp_path):
    for shape in ((12, 10, 2, 11), (200, 230, 26, 21)):
        r1cs, w = circuit.gen_circuit(*shape)
        m = list(w)
        m[len(w) - 1] = (m[-1] + 1) % bn254.R
        f = tmp_path / "c.r1cs"
        f.write_bytes(binfile.write_r1cs(r1cs))
        ws = []
        for k, x in enumerate((w, m)):
            ws.append(str(tmp_path / ("w%d.bin" % k)))
            open(ws[-1], "wb").write(b"".join(v.to_bytes(32, "little") for v in x))
        assert _run(emu, [str(f), "4", *ws]) == [_line(model.verdict(r1cs, w)), _line(model.verdict(r1cs, m))]


def test_replay_under_sanitizers(emu_san, cases):
    h, files, names, paths, wits = cases
    got = _run(emu_san, [files["good"], "24", *paths], SAN_ENV)
    assert got == [_line(model.verdict(h.r1cs, wits[n])) for n in names]


def test_reader_under_sanitizers_on_truncated_and_mutated_files(emu_san, tmp_path):
    r1cs, _ = circuit.gen_circuit(12, 10, 2, 11)
    f = tmp_path / "tiny.r1cs"
    data = binfile.write_r1cs(r1cs)
    f.write_bytes(data)
    (line,) = _run(emu_san, ["--fuzz", str(f), "7", "400"], SAN_ENV)
    inputs, parsed = int(line.split()[1]), int(line.split()[3])
    assert inputs == len(data) + 1 + 400
    assert 1 <= parsed < inputs  # the whole file parses, no proper prefix does, most mutations do


def test_reader_refuses_what_the_issue_lists(emu, tmp_path):
    import struct
    r1cs, _ = circuit.gen_circuit(12, 10, 2, 11)
    data = bytearray(binfile.write_r1cs(r1cs))
    _, secs = binfile.read_binfile(bytes(data), b"r1cs", 1)
    (h_off, _), = secs[1]
    (c_off, c_len), = secs[2]
    w = tmp_path / "w.bin"
    wit = [1] + [3 * i + 1 for i in range(1, 12)]
    w.write_bytes(b"".join(v.to_bytes(32, "little") for v in wit))

    def status(buf):
        f = tmp_path / "m.r1cs"
        f.write_bytes(bytes(buf))
        (line,) = _run(emu, [str(f), "0", str(w)])
        return line.split()[0:2]

    FORMAT, CURVE = "3", "5"
    m = bytearray(data)
    struct.pack_into("<I", m, c_off + 4, 12)                      # the first term's wire = nWires
    assert status(m) == ["ERROR", FORMAT]
    assert status(data[:c_off + c_len - 1]) == ["ERROR", FORMAT]  # a truncated section
    m = bytearray(data)
    struct.pack_into("<I", m, h_off, 31)                          # n8
    assert status(m) == ["ERROR", CURVE]
    m = bytearray(data)
    m[h_off + 4] ^= 2                                             # another prime
    assert status(m) == ["ERROR", CURVE]
    m = bytearray(data)
    struct.pack_into("<I", m, c_off, 0xFFFFFFFF)                  # a term count past the section
    assert status(m) == ["ERROR", FORMAT]
    # legal: an empty combination, a zero coefficient, a repeated wire
    r1cs.constraints[0] = ([], [(1, 0), (2, 5), (2, 7)], [])
    f = tmp_path / "legal.r1cs"
    f.write_bytes(binfile.write_r1cs(r1cs))
    assert model.failing(r1cs, wit)[0] > 0  # the rewritten constraint 0 holds: 0 * (12 w2) = 0
    assert _run(emu, [str(f), "0", str(w)]) == [_line(model.verdict(r1cs, wit))]
