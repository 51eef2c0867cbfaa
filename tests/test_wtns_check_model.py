"""The Python model of `wtns check` (tests/helpers/wtns_check_model.py) against the oracle's own
check_witness, on the tiny, small and hard circuits, on good witnesses and on every mutation the host
and GPU tests use -- so that those tests compare the kernels with a model that is itself checked."""
import os
import sys

import pytest

from oracle import circuit
from oracle.bn254 import R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wtns_check_model as model  # noqa: E402

CIRCUITS = {"tiny": (12, 10, 2, 11), "small": (200, 230, 26, 21)}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_model_agrees_with_the_oracle_on_generated_circuits(name):
    r1cs, w = circuit.gen_circuit(*CIRCUITS[name])
    assert circuit.check_witness(r1cs, w) and model.failing(r1cs, w) == []
    assert model.verdict(r1cs, w) == (True, "OK", 0, None, [])
    for wire in (1, len(w) // 2, len(w) - 1):
        m = list(w)
        m[wire] = (m[wire] + 1) % R
        bad = model.failing(r1cs, m)
        assert circuit.check_witness(r1cs, m) == (bad == [])
        assert bad == sorted(bad)


def test_hard_circuit_has_the_shapes_it_promises():
    h = model.hard_circuit()
    cons = h.r1cs.constraints
    assert h.r1cs.n_constraints == len(cons) and len(cons) % 64 and len(cons) % 256
    for side in range(3):
        lengths = {len(c[side]) for c in cons}
        assert lengths >= set(range(301)) and max(lengths) > 4096  # every side has a row past one pass of 4096 lanes
    assert any(len(a) == 4097 for a, _, _ in cons) and any(len(b) == 70001 for _, b, _ in cons)
    assert {len(a) for a, b, c in cons if len(a) == len(b) == len(c)} >= set(range(101))
    assert any(v == 0 for a, _, _ in cons for _, v in a)                    # an explicit zero coefficient
    assert any(len({s for s, _ in a}) < len(a) for a, _, _ in cons)         # a repeated wire
    terms = sum(len(a) + len(b) + len(c) for a, b, c in cons)
    assert 200_000 < terms < 500_000
    # a probe wire occurs once in the whole matrix, at the end of its row it is named for
    for (length, end), wire in h.probes.items():
        at = [(i, k, len(a)) for i, (a, b, c) in enumerate(cons) for lc in (a, b, c) for k, (s, _) in enumerate(lc) if s == wire]
        assert len(at) == 1 and at[0][2] == length and at[0][1] == (0 if end == "first" else length - 1)


def test_model_agrees_with_the_oracle_on_the_hard_circuit_and_its_mutations():
    h = model.hard_circuit()
    assert circuit.check_witness(h.r1cs, h.w) and model.failing(h.r1cs, h.w) == []
    n = h.r1cs.n_constraints
    # the designed failure of the bad variant: the added constraint and nothing else
    assert not circuit.check_witness(h.bad_r1cs, h.w) and model.failing(h.bad_r1cs, h.w) == [n]
    muts = model.mutations(h)
    want_single = {"first_plus_1": 0, "last_minus_1": n - 1, "c255_plus_1": 255, "c256_minus_1": 256}
    for name, m in muts.items():
        bad = model.failing(h.r1cs, m)
        assert bad and not circuit.check_witness(h.r1cs, m), name
        if name in want_single:
            assert bad == [want_single[name]], name
        if name.startswith("probe_"):
            assert len(bad) == 1 and len(h.r1cs.constraints[bad[0]][0]) == int(name.split("_")[1]), name
    assert len(model.failing(h.r1cs, muts["all_zero"])) > 16  # the list's cap is exercised
    v = model.verdict(h.r1cs, muts["all_zero"])
    assert not v[0] and len(v[4]) == 16 and v[3] == v[4][0] and v[2] > 16


def test_verdict_precedence():
    r1cs, w = circuit.gen_circuit(*CIRCUITS["tiny"])
    assert model.verdict(r1cs, [2] + w[1:])[1] == "INVALID: signal 0 is not 1"
    m = list(w)
    m[5] = R
    assert model.verdict(r1cs, m)[1] == "INVALID: signal 5 is not reduced"
