"""`wtns check` on the GPU (zkp_wtns_check / zkp_checker_*) against the Python model
(tests/helpers/wtns_check_model.py): good witnesses are accepted, every mutation is rejected with the
model's count, first index, list and message -- on the generated circuits, on the hard-shape circuit
(every row length around the switch between the two kernels, rows longer than a wavefront's pass, sums that
cancel and sums that wrap) and on a synth circuit of 2^16 signals (many workgroups) -- a checker keeps
nothing from one call to the next, and a staged witness is checked in place without changing it."""
import json
import os
import sys

import pytest

from oracle import binfile, bn254, circuit, groth16
import zkp_amd
from zkp_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wtns_check_model as model  # noqa: E402

pytestmark = pytest.mark.gpu

R = bn254.R
INVALID_ARG = 1
SIZES = {"tiny": (12, 10, 2, 11), "small": (200, 230, 26, 21)}
_cache = {}


def _hard():
    """the hard circuit's files and one resident checker, shared by the tests that only read them"""
    if "hard" not in _cache:
        h = model.hard_circuit()
        _cache["hard"] = (h, binfile.write_r1cs(h.r1cs), zkp_amd.WitnessChecker(binfile.write_r1cs(h.r1cs)))
    return _cache["hard"]


def _same(res, want):
    ok, msg, n_bad, first, bad = want
    assert (res.valid, res.message, res.n_bad, res.first_bad, res.bad) == (ok, msg, n_bad, first, bad)
    assert bool(res) == ok


@pytest.mark.parametrize("name", sorted(SIZES))
def test_accepts_generated_circuits_and_rejects_a_changed_signal(name):
    r1cs, w = circuit.gen_circuit(*SIZES[name])
    rb = binfile.write_r1cs(r1cs)
    res = zkp_amd.wtns_check(rb, binfile.write_wtns(w))
    _same(res, (True, "OK", 0, None, []))
    assert res.n_constraints == r1cs.n_constraints
    for wire in (1, len(w) // 2, len(w) - 1):
        m = list(w)
        m[wire] = (m[wire] + 1) % R
        _same(zkp_amd.wtns_check(rb, binfile.write_wtns(m)), model.verdict(r1cs, m))


def test_accepts_the_hard_circuit():
    h, rb, chk = _hard()
    info = chk.info()
    assert info["n_vars"] == len(h.w) and info["n_constraints"] == h.r1cs.n_constraints
    assert info["n_terms"] == sum(len(a) + len(b) + len(c) for a, b, c in h.r1cs.constraints)
    # both kernels have work: rows on either side of the switch
    assert 0 < info["n_long"] < info["n_constraints"] and info["long_terms"] > 0
    _same(chk.check(binfile.write_wtns(h.w)), (True, "OK", 0, None, []))
    _same(zkp_amd.wtns_check(rb, binfile.write_wtns(h.w)), (True, "OK", 0, None, []))


@pytest.mark.parametrize("name", sorted(model.mutations()))
def test_rejects_every_mutation_as_the_model_does(name):
    h, rb, chk = _hard()
    m = model.mutations(h)[name]
    want = model.verdict(h.r1cs, m)
    assert not want[0] and want[2] >= 1
    if name == "all_zero":
        assert want[2] > 16 and len(want[4]) == 16
    _same(chk.check(binfile.write_wtns(m)), want)


def test_rejects_the_bad_circuit():
    h, _, _ = _hard()
    n = h.r1cs.n_constraints
    want = model.verdict(h.bad_r1cs, h.w)
    assert want[1] == "INVALID: constraint %d is not satisfied (1 of %d fail)" % (n, n + 1)
    _same(zkp_amd.wtns_check(binfile.write_r1cs(h.bad_r1cs), binfile.write_wtns(h.w)), want)


def _raw_wtns(values):
    """a .wtns with the values as given (binfile.write_wtns reduces them)"""
    good = binfile.write_wtns([0] * len(values))
    body = b"".join(v.to_bytes(32, "little") for v in values)
    return good[:len(good) - len(body)] + body


def test_signal_zero_and_unreduced_values_are_verdicts():
    h, _, chk = _hard()
    res = chk.check(_raw_wtns([2] + h.w[1:]))
    _same(res, (False, "INVALID: signal 0 is not 1", 0, None, []))
    mid = len(h.w) // 2
    for value in (R, R + 5, (1 << 256) - 1):
        m = list(h.w)
        m[mid] = value
        m[mid + 7] = R  # a later one too: the lowest index is reported
        _same(chk.check(_raw_wtns(m)), (False, "INVALID: signal %d is not reduced" % mid, 0, None, []))
    m = list(h.w)
    m[mid] = R - 1  # the largest reduced value is a constraint's business, not this check's
    assert "signal" not in chk.check(_raw_wtns(m)).message


def test_one_checker_keeps_nothing_between_calls():
    h, rb, chk = _hard()
    muts = model.mutations(h)
    order = [h.w, muts["all_zero"], h.w, muts["c255_plus_1"], [2] + h.w[1:], muts["last_minus_1"], h.w]
    for w in order:
        one = zkp_amd.wtns_check(rb, _raw_wtns(w))
        got = chk.check(_raw_wtns(w))
        _same(got, model.verdict(h.r1cs, w))
        assert (got.valid, got.message, got.n_bad, got.first_bad, got.bad) == \
               (one.valid, one.message, one.n_bad, one.first_bad, one.bad)


def test_synth_circuit_of_2_to_16_signals():
    shape = (1 << 16, 70000, 26, 0x5A4B5099)
    c = synth.Circuit(*shape)
    r1cs, w = circuit.gen_circuit(*shape)
    rb = c.r1cs().bytes()
    wt = c.witness(shape[3])
    # the model speaks of the same circuit and witness as the library's generator
    assert rb == binfile.write_r1cs(r1cs) and wt == binfile.write_wtns(w)
    chk = zkp_amd.WitnessChecker(rb)
    assert chk.info()["n_constraints"] == 70000
    _same(chk.check(wt), (True, "OK", 0, None, []))
    # an input bit feeds many constraints (its booleanity check among them)
    wire = 1 + 26 + 5
    m = list(w)
    m[wire] = (m[wire] + 2) % R
    want = model.verdict(r1cs, m)
    assert want[2] >= 2
    _same(chk.check(binfile.write_wtns(m)), want)
    chk.close()


def test_staged_witness_is_checked_in_place(golden_dir):
    zk = open(os.path.join(golden_dir, "circuit_small.zkey"), "rb").read()
    wt = open(os.path.join(golden_dir, "circuit_small.wtns"), "rb").read()
    man = json.load(open(os.path.join(golden_dir, "manifest.json")))["circuits"]["small"]
    want_proof = open(os.path.join(golden_dir, "proof_small.json")).read()
    r1cs, w = circuit.gen_circuit(*SIZES["small"])
    assert binfile.write_wtns(w) == wt
    m = list(w)
    m[150] = (m[150] + 1) % R
    p = zkp_amd.Prover(zk, devices=[0])
    chk = zkp_amd.WitnessChecker(binfile.write_r1cs(r1cs))
    p.stage(wt, slot=0)
    p.stage(binfile.write_wtns(m), slot=1)
    _same(chk.check_staged(p, 0), (True, "OK", 0, None, []))
    _same(chk.check_staged(p, 1), model.verdict(r1cs, m))
    _same(chk.check_staged(p, 0), (True, "OK", 0, None, []))
    # the check only read the slot: the staged proof is still the golden one
    proof, _ = p.prove_staged_raw(0, int(man["r"]), int(man["s"]))
    assert groth16.js_stringify(zkp_amd.proof_object(*proof)) == want_proof
    # another circuit's checker, an empty slot, a device index the prover does not have
    tiny = zkp_amd.WitnessChecker(binfile.write_r1cs(circuit.gen_circuit(*SIZES["tiny"])[0]))
    for checker, slot, dev_index in ((tiny, 0, 0), (chk, 7, 0), (chk, 0, 3)):
        with pytest.raises(zkp_amd.ZkpError) as e:
            checker.check_staged(p, slot, dev_index)
        assert e.value.status == INVALID_ARG
    tiny.close()
    chk.close()
    p.close()


def test_timings_are_the_stages_of_the_last_call():
    h, rb, _ = _hard()
    assert zkp_amd.wtns_check(rb, binfile.write_wtns(h.w)).valid
    t = zkp_amd.wtns_check_timings()
    assert sorted(t) == sorted(["parse_csr", "upload_convert", "witness_copy", "kernels", "total"])
    assert all(v >= 0 for v in t.values()) and t["kernels"] > 0 and t["parse_csr"] > 0
    stages = t["parse_csr"] + t["upload_convert"] + t["witness_copy"] + t["kernels"]
    # the stages are disjoint parts of the call: never more than its wall time, and what they leave out
    # (the wtns header, the result's unpacking, the frees) is a small part of a call of tens of ms
    assert stages <= t["total"] * 1.02 and stages >= 0.5 * t["total"]
