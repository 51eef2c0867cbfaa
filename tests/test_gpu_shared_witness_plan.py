"""One shared build for the witness plans B, A and C (MsmPlan::build_shared, ZKP_MSM share=): the digits
are computed and sorted once over the signals finite in any table, every entry tagged with the plans
it belongs to, and the sort's last pass writes each plan's words.

Every test is prover-level: the proof at fixed r, s equals oracle/cpu's and the proof under share=0
(one build per plan), from host memory and staged, and each launch accumulates the same number of
digits under both.  The masks are shaped by doctoring a synthetic key's sections 5-8 (A, B1, B2, C) in
Python: a base zeroed is the point at infinity for oracle/cpu and for the GPU alike, a base overwritten
with another finite base of its table is finite for both (such a key proves nothing, but both sides
compute the same five sums over it).
"""
import functools
import os

import pytest

from oracle import binfile, bn254, cpu_oracle
import zkp_amd
from zkp_amd import synth

pytestmark = pytest.mark.gpu
R_FIX, S_FIX = 0x1234567, 0x7654321
N_VARS, N_CONS, N_PUB = 3001, 3500, 5  # 3-part slices start at 1000 and 2000: inside a bitset word
TABLES = (("A", 5, 64), ("B1", 6, 64), ("B2", 7, 128), ("C", 8, 64))
HS_TILE = 8192  # hsort_kernels.hpp
EDGES = (31, 32, 33, 63, 64, 65, N_VARS - 1)


def _first(name, n_pub):
    return n_pub + 1 if name == "C" else 0  # section 8 starts at the first private signal


def _finite(zk, n_vars, n_pub):
    """per table: is the base of signal i finite"""
    _, secs = binfile.read_binfile(zk, b"zkey", 1)
    out = {}
    for name, sid, pw in TABLES:
        first = _first(name, n_pub)
        pos, ln = secs[sid][0]
        assert ln == (n_vars - first) * pw
        out[name] = [False] * first + [any(zk[pos + pw * i:pos + pw * i + pw]) for i in range(n_vars - first)]
    return out


def _doctor(zk, n_vars, n_pub, want):
    """the key with table `name` finite exactly where want[name](i) says (tables not named stay):
    bases zeroed, or overwritten with the table's first finite base"""
    _, secs = binfile.read_binfile(zk, b"zkey", 1)
    buf = bytearray(zk)
    have = _finite(zk, n_vars, n_pub)
    for name, sid, pw in TABLES:
        if name not in want:
            continue
        first = _first(name, n_pub)
        pos = secs[sid][0][0]
        donor_i = have[name].index(True)
        donor = bytes(zk[pos + pw * (donor_i - first):pos + pw * (donor_i - first) + pw])
        for i in range(first, n_vars):
            at = pos + pw * (i - first)
            if want[name](i) and not have[name][i]:
                buf[at:at + pw] = donor
            elif not want[name](i) and have[name][i]:
                buf[at:at + pw] = bytes(pw)
    return bytes(buf)


@functools.lru_cache(maxsize=None)
def _plain(bool_pct, n_vars=N_VARS, n_cons=N_CONS):
    circ = synth.Circuit(n_vars, n_cons, N_PUB, 0x5A4B5032, bool_pct=bool_pct)
    return circ.zkey(0x5A4B5033).bytes(), circ.witness(11)


def _shapes():
    """name -> {table: i -> finite} over the 3001-signal key (bool_pct 70)"""
    edge = set(EDGES)
    return {
        # an empty plan beside two full ones
        "a_empty": {"A": lambda i: False},
        # every base of A finite (no mask: the unmasked plan) beside the masked B and C
        "a_all_finite": {"A": lambda i: True},
        # B1 and B2 differ: plan B takes their union
        "b_union": {"B1": lambda i: i % 3 == 0, "B2": lambda i: i % 5 == 0},
        # signals in exactly one table, in two, in all three and in none: bit 0 of i % 8 is A, bit 1 B, bit 2 C
        "membership": {"A": lambda i: bool(i % 8 & 1), "B1": lambda i: bool(i % 8 & 2), "B2": lambda i: bool(i % 8 & 2),
                       "C": lambda i: bool(i % 8 & 4)},
        # mask edges at the bitset-word and wave boundaries and the last signal: A only there, B and C only elsewhere
        "edges": {"A": lambda i: i in edge, "B1": lambda i: i not in edge, "B2": lambda i: i not in edge,
                  "C": lambda i: i not in edge},
        # nothing finite anywhere but C
        "only_c": {"A": lambda i: False, "B1": lambda i: False, "B2": lambda i: False},
    }


@functools.lru_cache(maxsize=None)
def _shaped(name):
    """(doctored key, witness, oracle/cpu's proof) of one mask shape, made once"""
    zk, wt = _plain(70)
    key = _doctor(zk, N_VARS, N_PUB, _shapes()[name])
    want, _ = cpu_oracle.prove(key, wt, R_FIX, S_FIX, threads=8)
    return key, wt, want


@functools.lru_cache(maxsize=None)
def _plain_case(bool_pct):
    zk, wt = _plain(bool_pct)
    want, _ = cpu_oracle.prove(zk, wt, R_FIX, S_FIX, threads=8)
    return zk, wt, want


def _run(zk, wt, spec, monkeypatch):
    """(proof from host memory, staged proof, {launch kind: adds}) of a fresh prover under ZKP_MSM=spec"""
    if spec is None:
        monkeypatch.delenv("ZKP_MSM", raising=False)
    else:
        monkeypatch.setenv("ZKP_MSM", spec)
    p = zkp_amd.Prover(zk, devices=[0])
    try:
        p.instrument(True)
        got, _ = p.prove_raw(wt, R_FIX, S_FIX)
        rec = p.launch_stats()
        p.instrument(False)
        p.stage(wt, slot=0)
        staged, _ = p.prove_staged_raw(0, R_FIX, S_FIX)
    finally:
        p.close()
    adds = {}
    for r in rec:
        assert r["msm"] not in adds  # one proof: one launch per kind
        adds[r["msm"]] = r["adds"]
    kinds = ("A", "B1", "B2", "C", "H")
    assert set(adds) <= set(kinds)
    for k in kinds:  # an empty plan launches nothing
        adds.setdefault(k, 0)
    return got, staged, adds


def _check(zk, wt, want, wsel, monkeypatch, unset=False):
    assert want and len(want) > 0
    got1, st1, adds1 = _run(zk, wt, "share=1,wsel=" + wsel, monkeypatch)
    got0, st0, adds0 = _run(zk, wt, "share=0,wsel=" + wsel, monkeypatch)
    print("adds share=1:", adds1, "share=0:", adds0)
    assert got0 == want and st0 == want  # the yardstick itself
    assert got1 == want and st1 == want
    assert adds1 == adds0
    if unset:  # the default is the shared build; which configuration a proof takes is then automatic
        gotd, std, _ = _run(zk, wt, None, monkeypatch)
        assert gotd == want and std == want
    return adds1


# ------------------------------------------------------------------ the oracle first

def test_oracle_proves_every_doctored_key():
    """on the CPU: oracle/cpu proves each doctored key, and the doctoring did what it says"""
    for name, shape in _shapes().items():
        key, _, want = _shaped(name)
        assert want, name
        f = _finite(key, N_VARS, N_PUB)
        for t, fn in shape.items():
            first = _first(t, N_PUB)
            assert f[t] == [False] * first + [bool(fn(i)) for i in range(first, N_VARS)], (name, t)
    f = _finite(_shaped("membership")[0], N_VARS, N_PUB)
    combos = {(f["A"][i], f["B1"][i] or f["B2"][i], f["C"][i]) for i in range(N_PUB + 1, N_VARS)}
    assert len(combos) == 8  # every membership from none to all three
    f = _finite(_shaped("b_union")[0], N_VARS, N_PUB)
    assert f["B1"] != f["B2"]
    f = _finite(_shaped("a_all_finite")[0], N_VARS, N_PUB)
    assert all(f["A"])


# ------------------------------------------------------------------ the plain key

@pytest.mark.parametrize("wsel", ["first", "second"])
@pytest.mark.parametrize("bool_pct", [0, 70, 100])
def test_plain_key(monkeypatch, bool_pct, wsel):
    zk, wt, want = _plain_case(bool_pct)
    adds = _check(zk, wt, want, wsel, monkeypatch, unset=wsel == "first")
    assert adds["B1"] == adds["B2"]


# ------------------------------------------------------------------ mask shapes

@pytest.mark.parametrize("wsel", ["first", "second"])
@pytest.mark.parametrize("name", sorted(_shapes()))
def test_mask_shapes(monkeypatch, name, wsel):
    key, wt, want = _shaped(name)
    adds = _check(key, wt, want, wsel, monkeypatch)
    if name == "a_empty":
        assert adds["A"] == 0 and adds["C"] > 0 and adds["B1"] > 0
    if name == "only_c":
        assert adds["A"] == adds["B1"] == adds["B2"] == 0 and adds["C"] > 0
    if name == "b_union":  # one plan for both: the union's digits
        assert adds["B1"] == adds["B2"] > 0


# ------------------------------------------------------------------ the tile boundary of pass C

TILE_VARS, TILE_CONS = 32000, 35000  # bool_pct=100: ~9100 signals of value 1, more than one tile


@functools.lru_cache(maxsize=None)
def _tile_case(a_ones):
    """C finite on every private signal of value 1 (more than HS_TILE of them: bucket 0 of plan C spans
    two tiles), B on HS_TILE - 1000 of them, A on exactly a_ones of them; no other value-1 signal has a
    finite A or B base, so bucket 0 of each plan holds exactly that many entries (+ signal 0 in A)"""
    zk, wt = _plain(100, TILE_VARS, TILE_CONS)
    _, w = binfile.read_wtns(wt)
    ones = [i for i in range(N_PUB + 1, TILE_VARS) if w[i] == 1]
    assert len(ones) > HS_TILE + 1
    have = _finite(zk, TILE_VARS, N_PUB)
    is_one = set(ones)
    a_set, b_set = set(ones[-a_ones:]), set(ones[:HS_TILE - 1000])
    # signal 0 (the constant 1) keeps a zero A base here, so A's bucket of value 1 is exactly a_set
    shape = {
        "A": lambda i: i in a_set if (i in is_one or i == 0) else have["A"][i],
        "B1": lambda i: i in b_set if (i in is_one or i == 0) else have["B1"][i],
        "B2": lambda i: i in b_set if (i in is_one or i == 0) else have["B2"][i],
        "C": lambda i: True if i in is_one else have["C"][i],
    }
    key = _doctor(zk, TILE_VARS, N_PUB, shape)
    want, _ = cpu_oracle.prove(key, wt, R_FIX, S_FIX, threads=8)
    f = _finite(key, TILE_VARS, N_PUB)
    ones_all = [i for i in range(TILE_VARS) if w[i] == 1]
    count = {t: sum(1 for i in ones_all if f[t][i]) for t in ("A", "B1", "B2", "C")}
    return key, wt, want, count


@pytest.mark.parametrize("a_ones", [HS_TILE, HS_TILE + 1])
def test_pass_c_tile_boundary(monkeypatch, a_ones):
    key, wt, want, count = _tile_case(a_ones)
    print("entries of the bucket of value 1:", count)
    assert count["C"] > HS_TILE and count["B1"] == count["B2"] == HS_TILE - 1000 and count["A"] == a_ones
    _check(key, wt, want, "first", monkeypatch)


# ------------------------------------------------------------------ split provers

@pytest.mark.parametrize("name", [None, "membership"])
def test_three_part_split(monkeypatch, name):
    zk, wt, want = _plain_case(70) if name is None else _shaped(name)
    out = {}
    for share in (1, 0):
        monkeypatch.setenv("ZKP_MSM", "share=%d" % share)
        parts = []
        for k in range(3):
            p = zkp_amd.Prover(zk, devices=[0], part=k, nparts=3)
            try:
                parts.append(p.prove_partial(wt))
            finally:
                p.close()
        out[share], _ = zkp_amd.proof_combine_raw(zk, parts, wt, R_FIX, S_FIX)
    assert out[0] == want and out[1] == want


def test_serial_streams(monkeypatch):
    """ZKP_SERIAL=1 chains the streams: the shared build feeds the same accumulations"""
    key, wt, want = _shaped("membership")
    monkeypatch.setenv("ZKP_SERIAL", "1")
    got, staged, _ = _run(key, wt, "share=1", monkeypatch)
    assert got == want and staged == want


@pytest.mark.parametrize("spec", ["share=1,cgate=1", "share=0,cgate=1", "share=1,cgate=0"])
def test_c_gate(monkeypatch, spec):
    """cgate=1 only moves accumulation C behind the quotient: the same proof"""
    key, wt, want = _shaped("membership")
    got, staged, _ = _run(key, wt, spec, monkeypatch)
    assert got == want and staged == want


# ------------------------------------------------------------------ knob validation

@pytest.mark.parametrize("spec", ["share=2", "share=", "share=yes", "share=-1", "share=01", "cgate=2", "cgate=",
                                  "cgate=on", "cgate=-1", "cgate=10"])
def test_bad_knob_value_is_rejected(golden_dir, monkeypatch, spec):
    pts = synth.points(synth.scalars(0x51, 0, 1))
    monkeypatch.setenv("ZKP_MSM", spec)
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.msm_g1(pts, bn254.int_to_le(1))
    assert e.value.status == 1 and "ZKP_MSM" in e.value.message
    zk = open(os.path.join(golden_dir, "circuit_small.zkey"), "rb").read()
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.Prover(zk, devices=[0])
    assert e.value.status == 1 and "ZKP_MSM" in e.value.message


@pytest.mark.parametrize("val", ["4", "-1", "x", "1x"])
def test_bad_g2first_value_is_rejected(golden_dir, monkeypatch, val):
    monkeypatch.setenv("ZKP_G2FIRST", val)
    zk = open(os.path.join(golden_dir, "circuit_small.zkey"), "rb").read()
    with pytest.raises(zkp_amd.ZkpError) as e:
        zkp_amd.Prover(zk, devices=[0])
    assert e.value.status == 1 and "ZKP_G2FIRST" in e.value.message
