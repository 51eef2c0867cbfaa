"""`groth16 verify` from a verification key on the GPU (zkp_verifier_*, csrc/groth16_verify.hip): per-proof
gates, the randomised batch equation with the Miller loops on the device, and the tree search of a failing
batch.  The contract under test: verdict i equals zkp_proof_verify of proof i under the same key."""
import json
import os
import random
import sys
import threading

import pytest

from oracle import bn254
import zkp_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import g2_twist  # noqa: E402

pytestmark = pytest.mark.gpu

R, P = bn254.R, bn254.P
NAMES = ["tiny", "small", "venmo_mini"]
N = 130  # three waves, the last one partial


def _case(golden_dir, name):
    zk = open(os.path.join(golden_dir, "circuit_%s.zkey" % name), "rb").read()
    vk = open(os.path.join(golden_dir, "vkey_%s.json" % name)).read()
    proof = json.load(open(os.path.join(golden_dir, "proof_%s.json" % name)))
    pub = [int(x) for x in json.load(open(os.path.join(golden_dir, "public_%s.json" % name)))]
    return zk, vk, proof, pub


def _tup(proof):
    a, b, c = proof["pi_a"], proof["pi_b"], proof["pi_c"]
    return ((int(a[0]), int(a[1])), ((int(b[0][0]), int(b[0][1])), (int(b[1][0]), int(b[1][1]))), (int(c[0]), int(c[1])))


@pytest.mark.parametrize("name", NAMES)
def test_golden_proofs_verify_from_a_vkey_and_from_a_zkey(golden_dir, name):
    zk, vk, proof, pub = _case(golden_dir, name)
    for key in (vk, json.loads(vk), zk):
        v = zkp_amd.Verifier(key)
        assert v.n_public == len(pub)
        assert v.verify(proof, pub) is True
        assert v.verify(_tup(proof), pub) is True
        t = v.timings()
        assert t["node_checks"] == 1 and t["search_ms"] == 0 and t["total_ms"] > 0
        v.close()


@pytest.mark.parametrize("name", NAMES)
def test_every_tampering_is_rejected(golden_dir, name):
    zk, vk, proof, pub = _case(golden_dir, name)
    a, b, c = _tup(proof)
    v = zkp_amd.Verifier(vk)
    bad = []
    if pub:
        bad.append(((a, b, c), [(pub[0] + 1) % R] + pub[1:]))
        bad.append(((a, b, c), [pub[0] + R] + pub[1:]))  # the same residue, but >= r
    bad.append(((c, b, a), pub))
    bad.append(((a, b, bn254.g1_add(c, bn254.G1_GEN)), pub))
    bad.append(((a, (b[0], bn254.f2_neg(b[1])), c), pub))
    bad.append((((a[0], (a[1] + 1) % P), b, c), pub))            # A off the curve
    bad.append(((a, g2_twist.q_point(), c), pub))                # B on the twist, outside the subgroup
    bad.append(((a, g2_twist.t_point(), c), pub))                # ... of the small order 10069
    bad.append((((a[0] + P, a[1]), b, c), pub))                  # a coordinate >= p (the same residue)
    bad.append(((a, ((b[0][0], b[0][1] + P), b[1]), c), pub))
    for proof_t, signals in bad:
        assert v.verify(proof_t, signals) is False
    # one call: the good proof between the bad ones keeps its verdict
    items = [bad[0], ((a, b, c), pub)] + bad[1:]
    assert v.verify_batch(items, seed=bytes(range(32))) == [False, True] + [False] * (len(bad) - 1)
    v.close()


# ---------------------------------------------------------------- batches of circuit_tiny
@pytest.fixture(scope="module")
def batch(golden_dir):
    zk, vk, _, _ = _case(golden_dir, "tiny")
    wt = open(os.path.join(golden_dir, "circuit_tiny.wtns"), "rb").read()
    rng = random.Random(130)
    prover = zkp_amd.Prover(zk, devices=[0])
    items = prover.prove_batch_raw([wt] * N, [rng.randrange(1, R) for _ in range(N)], [rng.randrange(1, R) for _ in range(N)])
    prover.close()
    assert len({it[0] for it in items}) == N  # distinct r, s: distinct proofs
    return {"zk": zk, "vk": vk, "items": [(p, list(pub)) for p, pub in items], "ref": {}}


def _ref(batch, items):
    """per-proof zkp_proof_verify under the same key, each distinct proof once"""
    out = []
    for proof, pub in items:
        key = (proof, tuple(pub))
        if key not in batch["ref"]:
            try:
                batch["ref"][key] = zkp_amd.proof_verify(batch["zk"], proof, pub)
            except zkp_amd.ZkpError:  # the host verifier refuses a coordinate >= p with a status
                batch["ref"][key] = False
        out.append(batch["ref"][key])
    return out


def _c_plus(item, k=1):
    (a, b, c), pub = item
    g = bn254.G1_GEN if k > 0 else bn254.g1_neg(bn254.G1_GEN)
    return ((a, b, bn254.g1_add(c, g)), pub)


def _a_off_curve(item):
    (a, b, c), pub = item
    return (((a[0], (a[1] + 1) % P), b, c), pub)


def _with_bad(items, at):
    out = list(items)
    for i in at:
        out[i] = _c_plus(out[i])
    return out


CASES = {
    "none": lambda it: list(it),
    "one_at_0": lambda it: _with_bad(it, [0]),
    "one_at_63": lambda it: _with_bad(it, [63]),
    "one_at_64": lambda it: _with_bad(it, [64]),
    "one_at_129": lambda it: _with_bad(it, [129]),
    "two_adjacent": lambda it: _with_bad(it, [63, 64]),
    "every": lambda it: _with_bad(it, range(len(it))),
    "gated_beside_pairing_bad": lambda it: [_a_off_curve(x) if i == 40 else _c_plus(x) if i == 41 else x
                                            for i, x in enumerate(it)],
}


@pytest.fixture(scope="module")
def verifier(batch):
    v = zkp_amd.Verifier(batch["vk"])
    yield v
    v.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_batch_verdicts_equal_per_proof_verification(batch, verifier, case, seed):
    items = CASES[case](batch["items"])
    want = _ref(batch, items)
    assert want.count(False) == {"none": 0, "two_adjacent": 2, "every": N, "gated_beside_pairing_bad": 2}.get(case, 1)
    got = verifier.verify_batch(items, seed=seed.to_bytes(32, "little"))
    assert got == want
    t = verifier.timings()
    if case == "none":
        assert t["node_checks"] == 1
    else:
        assert 1 < t["node_checks"] <= 2 * N - 1  # the worst case: every node of the tree


def test_a_cancelling_pair_is_caught(batch, verifier):
    # C + G in one proof and C - G in another leave the plain sum of the C's unchanged: only the random
    # coefficients tell them apart
    items = list(batch["items"])
    items[10] = _c_plus(items[10], +1)
    items[100] = _c_plus(items[100], -1)
    want = [i not in (10, 100) for i in range(N)]
    assert _ref(batch, items) == want
    for seed in (1, 2, 3):
        assert verifier.verify_batch(items, seed=seed.to_bytes(32, "little")) == want
    assert verifier.verify_batch(items) == want  # the production call: OS seed


def test_a_batch_larger_than_the_chunk(batch, monkeypatch):
    items = _with_bad(batch["items"], [5, 64, 129])
    monkeypatch.setenv("ZKP_VERIFY_CHUNK", "64")
    v = zkp_amd.Verifier(batch["vk"])
    assert v.verify_batch(items, seed=bytes(32)) == _ref(batch, items)
    monkeypatch.setenv("ZKP_VERIFY_CHUNK", "63")  # below the range: refused, not clamped
    with pytest.raises(zkp_amd.ZkpError) as e:
        v.verify_batch(items[:2], seed=bytes(32))
    assert e.value.status == 1  # ZKP_ERR_INVALID_ARG
    v.close()


def test_empty_batch_and_wrong_public_count(batch, verifier):
    assert verifier.verify_batch([]) == []
    proof, pub = batch["items"][0]
    with pytest.raises(zkp_amd.ZkpError) as e:
        verifier.verify_batch([(proof, pub), (proof, pub + [1])])
    assert e.value.status == 1  # ZKP_ERR_INVALID_ARG
    with pytest.raises(zkp_amd.ZkpError) as e:
        verifier.verify(proof, pub[:-1])
    assert e.value.status == 1  # ZKP_ERR_INVALID_ARG


def test_two_threads_on_one_handle_agree(batch, verifier):
    items = _with_bad(batch["items"], [7, 77])
    want = _ref(batch, items)
    got = [None, None]

    def run(k):
        got[k] = verifier.verify_batch(items, seed=bytes([k + 1]) * 32)

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == want and got[1] == want
