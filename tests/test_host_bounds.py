"""The lazy-reduction bounds of csrc/field.hpp, curve.hpp and ntt_unit.hpp, PROVEN for every input:
tools/hosttest/bounds.cpp evaluates the project's own templates on interval limbs with an exact value
interval (tools/hosttest/bounds.hpp) and fails on any limb expression outside [0, 2^32), any column
accumulator at 2^64, any truncation other than the two intended ones, any borrow-form top limb the
value does not bring back above zero, and any chain output outside the invariant it started from.

a. the tree is proven, and every documented bound is implied by the proven one (exact integers);
b. the prover rejects known-bad code: five one-line mutations of a copy of csrc/, each of which must
   fail at the op named for it (the first is the round-5 sub_raw8 top-limb wrap);
c. the abstraction is sound: the same chains on real uint32_t limbs (random, extreme and corner
   inputs) never leave the interval proven for the same step.

CPU-only.  The chains are independent, so the proving run is spread over a few processes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT = os.path.join(ROOT, "tools", "hosttest")
CSRC = os.path.join(ROOT, "zk-p2p-onramp_amd", "csrc")

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return hipcc


def _build(tmp, csrc=None):
    """bounds.cpp compiled for the host; csrc: a (mutated) copy of the device headers to build against"""
    src = os.path.join(HT, "bounds.cpp")
    if csrc is not None:  # the tool includes ../../zk-p2p-onramp_amd/csrc/: mirror that layout around the copy
        ht = os.path.join(tmp, "tools", "hosttest")
        os.makedirs(ht)
        for f in ("bounds.cpp", "bounds.hpp"):
            shutil.copy(os.path.join(HT, f), ht)
        src = os.path.join(ht, "bounds.cpp")
    out = os.path.join(tmp, "bounds")
    subprocess.run([_hipcc(), "--offload-host-only", "-O1", "-std=c++17", src, "-o", out], check=True, timeout=900)
    return out


# the proving run, spread over processes: each group is one --chains argument
GROUPS = ["NTT[Fr]", "G1[FqAcc]", "G1[Fq]",
          "G2[Fq2] forms,G2[Fq2] xyzz_add,G2[Fq2] xyzz_dbl,G2[Fq2] store_xyzz",
          "G2[Fq2] xyzz_from_aff_pair np=0 nq=0", "G2[Fq2] xyzz_from_aff_pair np=1 nq=0",
          "G2[Fq2] xyzz_from_aff_pair np=0 nq=1", "G2[Fq2] xyzz_from_aff_pair np=1 nq=1"]


@pytest.fixture(scope="module")
def proof(tmp_path_factory):
    exe = _build(str(tmp_path_factory.mktemp("bounds")))
    procs = [subprocess.Popen([exe, "--quiet", "--chains", g], stdout=subprocess.PIPE, text=True) for g in GROUPS]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    names = subprocess.run([exe, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {"codes": [p.returncode for p in procs], "out": "\n".join(outs), "chains": [n for n in names if n and not n.startswith("CONST ")]}


def test_tree_is_proven(proof):
    out = proof["out"]
    assert proof["codes"] == [0] * len(GROUPS), out[-4000:]
    assert "FAIL" not in out and "UNSOUND" not in out
    # no chain left unproven: every chain of the tool was visited by exactly one process
    proven = re.findall(r"^CHAIN (.*) paths=\d+$", out, re.M)
    assert sorted(proven) == sorted(proof["chains"]) and len(set(proven)) == len(proven)
    for want in ("xyzz_from_aff_pair", "xyzz_add_aff", "xyzz_add", "xyzz_dbl_aff", "xyzz_dbl", "store_xyzz", "primitives"):
        for grp in ("G1[FqAcc]", "G1[Fq]", "G2[Fq2]"):
            if want == "primitives" and grp == "G2[Fq2]":
                continue
            assert any(c.startswith(grp + " " + want) for c in proven), (grp, want)
    for want in ("r4 unit (Hh > 1)", "r4 last pair raw", "r4 last pair stored", "r2 first stage pair", "r2 first stage one",
                 "r2 only stage raw", "r2 only stage stored", "primitives"):
        assert "NTT[Fr] " + want in proven


def _bounds(out):
    """(chain, name) -> (proven inclusive value bound, low-limb maximum, top-limb maximum)"""
    b = {}
    for ln in out.split("\n"):
        if ln.startswith("BOUND "):
            f = [x.strip() for x in ln[6:].split("|")]
            b[(f[0], f[1])] = (int(f[3], 16), int(f[5].split("<=")[1]), int(f[6].split("<=")[1]))
    return b


def test_documented_bounds_are_implied(proof):
    """Exact: proven (inclusive) bound < documented (exclusive) bound, as integers."""
    b = _bounds(proof["out"])
    L29, L30 = (1 << 29) - 1, (1 << 30) - 1

    def implied(chain, name, num, den, m, limbs=L29):
        assert (chain, name) in b, (chain, name)
        v, lo, _ = b[(chain, name)]
        assert v * den < num * m, (chain, name, hex(v))
        assert lo <= limbs, (chain, name, lo)

    for g1 in ("G1[FqAcc]", "G1[Fq]"):
        # mul, mul2 and sqr outputs < 2m, at the primitives' documented operand limits
        for name in ("mont_sop N=1, both limbs < 2^30, < 8m", "mont_sop N=1, raw limbs < 2.5 * 2^30 x normalised",
                     "mont_sop N=1, 11m x 11m", "mont_sop N=2, 162 m^2", "mont_sop N=4, 144 m^2", "mont_sqr, 11m"):
            implied(g1 + " primitives", name, 2, 1, P)
        implied(g1 + " primitives", "mont_shoup, raw limbs < 2.5 * 2^30, < 2^261", 3, 1, P)
        implied(g1 + " primitives", "qreduce, limbs < 2^32 - 2^10", 6, 5, P)
        implied(g1 + " forms", "sub_2x8", 8, 1, P)      # G1 x < 8m
        implied(g1 + " forms", "lsub8", 10, 1, P)
        implied(g1 + " forms", "lsub", 4, 1, P)
        implied(g1 + " forms", "rsub", 6, 1, P, limbs=(1 << 31) - 1)
        implied(g1 + " forms", "sub_2x", 2, 1, P)
        implied(g1 + " forms", "canon8", 2, 1, P)
        implied(g1 + " forms", "mul2(r, t, y, d)", 2, 1, P)
        for ch in ("xyzz_from_aff_pair np=0 nq=0", "xyzz_from_aff_pair np=1 nq=1", "xyzz_add_aff neg=0", "xyzz_add_aff neg=1",
                   "xyzz_add", "xyzz_dbl_aff", "xyzz_dbl"):  # the induction closes
            implied(g1 + " " + ch, "x", 8, 1, P)
            for c in ("y", "zz", "zzz"):
                implied(g1 + " " + ch, c, 2, 1, P)
        implied(g1 + " store_xyzz", "x stored", 2, 1, P)
    for s in (".c0", ".c1"):  # G2 components as commented
        implied("G2[Fq2] forms", "sub_2x4" + s, 4, 1, P)
        implied("G2[Fq2] forms", "lsub4_lazy" + s, 6, 1, P)
        implied("G2[Fq2] forms", "lsub2_lazy" + s, 4, 1, P)
        implied("G2[Fq2] forms", "sqr_lazy" + s, 2, 1, P)
        implied("G2[Fq2] forms", "acc_y3" + s, 2, 1, P)
        implied("G2[Fq2] forms", "mul" + s, 2, 1, P)
        implied("G2[Fq2] forms", "canon4" + s, 2, 1, P)
        for ch in ("xyzz_from_aff_pair np=0 nq=1", "xyzz_add_aff neg=0", "xyzz_add_aff neg=1", "xyzz_add", "xyzz_dbl_aff", "xyzz_dbl"):
            implied("G2[Fq2] " + ch, "x" + s, 4, 1, P)
            for c in ("y", "zz", "zzz"):
                implied("G2[Fq2] " + ch, c + s, 2, 1, P)
    v, _, _ = b[("G2[Fq2] forms", "neg4 (<= 4m)")]
    assert v <= 4 * P
    # NTT: tile values back < 3m, Shoup < 3m, qreduce < 1.2m = 6m/5, the raw last-pair forms
    for ch, n in (("r4 unit (Hh > 1)", 4), ("r4 last pair stored", 4), ("r2 first stage pair", 4), ("r2 first stage one", 2),
                  ("r2 only stage stored", 2)):
        for k in range(n):
            implied("NTT[Fr] " + ch, "p%d" % k, 3, 1, R)
    for name, num, limbs in (("p0 raw", 12, (1 << 31) - 1), ("p1 raw (sub_raw8)", 14, 5 * (1 << 29) - 1), ("p2 raw", 6, L30),
                             ("p3 raw", 7, 3 * (1 << 29) - 1)):
        implied("NTT[Fr] r4 last pair raw", name, num, 1, R, limbs=limbs)
    for k in range(4):
        implied("NTT[Fr] r4 last pair raw", "p%d x table" % k, 2, 1, R)
        implied("NTT[Fr] r4 last pair raw", "p%d x root" % k, 3, 1, R)
    for k in range(2):
        implied("NTT[Fr] r2 only stage raw", "p%d x table" % k, 2, 1, R)
    implied("NTT[Fr] forms", "sub_raw8", 14, 1, R, limbs=5 * (1 << 29) - 1)  # limbs < 2.5 * 2^30, value < 14m
    for name in ("add", "sub", "sub4", "add (tile values < 3m)", "add_raw_reduce", "qreduce(sub_raw8)", "sub_2x"):
        implied("NTT[Fr] forms", name, 6, 5, R)
    implied("NTT[Fr] primitives", "mont_shoup, raw limbs < 2.5 * 2^30, < 2^261", 3, 1, R)
    implied("NTT[Fr] primitives", "qreduce, limbs < 2^32 - 2^10", 6, 5, R)


def test_abstraction_is_sound(proof):
    """Every limb and value of the real arithmetic lies inside the interval proven for the same step."""
    out = proof["out"]
    sound = re.findall(r"^SOUND (.*) checked=(\d+) escapes=(\d+)$", out, re.M)
    assert sorted(s[0] for s in sound) == sorted(proof["chains"])
    assert all(int(s[1]) > 400 for s in sound), [s for s in sound if int(s[1]) <= 400]
    assert all(int(s[2]) == 0 for s in sound), [s for s in sound if int(s[2])]
    assert "ESCAPE" not in out


def _mod8_b30_as_6m(m):
    """6m in the 2^30-raised borrow form (the round-5 table): low limbs + 2^30, each borrowing 2 from the next"""
    v, limbs = 6 * m, []
    for i in range(9):
        limbs.append((v >> (29 * i)) & ((1 << 29) - 1) if i < 8 else v >> (29 * 8))
    for i in range(8):
        limbs[i] += 1 << 30
        limbs[i + 1] -= 2
    assert sum(x << (29 * i) for i, x in enumerate(limbs)) == 6 * m and all(x >= 0 for x in limbs)
    return "{" + ", ".join("0x%08xu" % x for x in limbs) + "}"


def _line_of(path, key, field):
    """the `static constexpr uint32_t <key>[9] = {...};` line of struct <field> in consts.hpp"""
    txt = open(path).read()
    a = txt.index("struct %s {" % field)
    i = txt.index("  static constexpr uint32_t %s[9] = " % key, a)
    return txt[i:txt.index("\n", i)]


MUTATIONS = [
    # (id, file, old text (None: computed), new text, chains to run, op the failure must name, words it must hold)
    ("mod8_b30_is_6m", "consts.hpp", None, None, "NTT[Fr]", "sub_raw8", "top limb"),
    ("lsub8_on_6m", "field.hpp", "normalized(borrow_sub(a, ZTAB(MOD8_BORROW), b))", "normalized(borrow_sub(a, ZTAB(MOD6_BORROW), b))",
     "G1[FqAcc]", "lsub8", "negative"),
    ("g2_y3_in_g1_order", "curve.hpp", "{ return mul2(t, r, d, y); }", "{ return mul2(r, t, y, d); }", "G2[Fq2]", "neg4", "negative"),
    ("fq2_rsub_raw", "field.hpp",
     "ZDEV Fq2T<C> rsub(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{lsub(a.c0, b.c0), lsub(a.c1, b.c1)}; }",
     "ZDEV Fq2T<C> rsub(const Fq2T<C>& a, const Fq2T<C>& b) { return Fq2T<C>{rsub(a.c0, b.c0), rsub(a.c1, b.c1)}; }",
     "G2[Fq2] xyzz_add_aff", "mul", "not normalised"),
    ("g1_x_into_lsub", "curve.hpp", "F P = acc_xsub(U2, acc.x);", "F P = acc_sub(U2, acc.x);", "G1[FqAcc] xyzz_add_aff", "lsub",
     "negative"),
]


@pytest.mark.parametrize("mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_prover_rejects_mutation(mut, tmp_path):
    name, fname, old, new, chains, op, words = mut
    csrc = tmp_path / "zk-p2p-onramp_amd" / "csrc"
    os.makedirs(csrc)
    for f in os.listdir(CSRC):
        if f.endswith(".hpp"):
            shutil.copy(os.path.join(CSRC, f), csrc)
    path = str(csrc / fname)
    if old is None:  # the historical bug: MOD8_B30 holds 6m with its low limbs raised by 2^30
        old = _line_of(path, "MOD8_B30", "FrCfg")
        new = "  static constexpr uint32_t MOD8_B30[9] = %s;" % _mod8_b30_as_6m(R)
    txt = open(path).read()
    assert txt.count(old) == 1, "the mutation must match exactly once"
    open(path, "w").write(txt.replace(old, new))
    exe = _build(str(tmp_path), csrc=str(csrc))
    r = subprocess.run([exe, "--quiet", "--chains", chains], stdout=subprocess.PIPE, text=True, timeout=900)
    fails = [ln for ln in r.stdout.split("\n") if ln.startswith("FAIL ")]
    assert r.returncode != 0 and len(fails) == 1, r.stdout[-2000:]
    assert re.search(r"\bop=%s:" % re.escape(op), fails[0]) or (" %s " % op) in fails[0], fails[0]
    assert op in fails[0] and words in fails[0], fails[0]
    if name == "mod8_b30_is_6m":
        assert "top limb of a sub_raw8 result" in fails[0] and "NTT[Fr] r4" in fails[0], fails[0]
