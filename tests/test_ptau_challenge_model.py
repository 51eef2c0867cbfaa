"""The pure-Python model of `powersoftau export challenge | challenge contribute | import response`
(tests/helpers/ptau_challenge_model.py) against ptau_model: the three commands in a row equal one
ptau_model.contribute with the same rng byte for byte, the result verifies, the files have their stated sizes and
the exported challenge hashes to the chain's last challenge."""
import functools
import os
import sys

import pytest

from oracle import mpc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ptau_challenge_model as cm  # noqa: E402
import ptau_model as pm  # noqa: E402

RAND = [bytes((37 * i + 11 + 50 * k) & 0xFF for i in range(64)) for k in range(3)]
BEACON = bytes(range(1, 32))


@functools.lru_cache(maxsize=None)
def _file(power, prior):
    f = pm.new(power)
    if prior:
        f = pm.contribute(f, mpc.entropy_rng(RAND[0], "first"), "alice")
        f = pm.beacon(f, BEACON, 4, None)
    return f


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("prior", [0, 2])
def test_three_commands_equal_one_contribution(power, prior):
    f, n = _file(power, prior), 1 << power
    challenge = cm.export_challenge(f)
    assert len(challenge) == 384 * n + 128
    assert pm.blake2b(challenge) == pm._last_challenge(pm.Ptau.read(f))
    response = cm.challenge_contribute(challenge, mpc.entropy_rng(RAND[2], "third"))
    assert len(response) == 192 * n + 864 and response[:64] == pm.blake2b(challenge)
    got = cm.import_response(f, response, "Third contribution name")
    assert got == pm.contribute(f, mpc.entropy_rng(RAND[2], "third"), "Third contribution name")
    assert pm.verify(got) == (True, "OK")
    assert len(pm.Ptau.read(got).contributions) == prior + 1


def test_refusals():
    f = _file(1, 0)
    response = cm.challenge_contribute(cm.export_challenge(f), mpc.entropy_rng(RAND[1], "x"))
    with pytest.raises(ValueError, match="size of the contribution"):
        cm.import_response(f, response[:-1])
    with pytest.raises(ValueError, match="not based on the previous hash"):
        cm.import_response(f, bytes([response[0] ^ 1]) + response[1:])
    with pytest.raises(ValueError):
        cm.challenge_power(384 * 3 + 128)
    assert cm.challenge_power(384 * 8 + 128) == 3
