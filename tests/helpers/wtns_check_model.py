"""Python model of `wtns check` and the shared hard-shape circuit of its tests.

failing(r1cs, w): the ascending list of constraints with ev(A) ev(B) != ev(C), in Python integers mod r.
verdict(r1cs, w): what zkp_wtns_check must answer (valid, message, n_bad, first_bad, bad).
hard_circuit(): the smallest set of row shapes at which the constraint kernels can go wrong -- every row
length 0..300 in A, in B and in C, all three rows alike for 0..100, rows of 4097 and 70 001 terms (longer
than one pass of a wavefront or a workgroup), exact cancellation, sums that wrap r many times, a zero
coefficient, repeated wires, empty sides -- with a witness that satisfies it, a variant with one designed
failure, and the named mutations of the witness.  Built once per process and never modified.
"""
from __future__ import annotations

from oracle.bn254 import R
from oracle.circuit import R1CS, SplitMix64

NPOOL = 64          # input wires 1..NPOOL; wire 0 is the constant 1
PROBE_LENGTHS = (64, 65, 129, 4097)
_cache = {}


def ev(lc, w):
    return sum(c * w[s] for s, c in lc) % R


def failing(r1cs, w):
    return [i for i, (a, b, c) in enumerate(r1cs.constraints) if ev(a, w) * ev(b, w) % R != ev(c, w)]


def verdict(r1cs, w):
    """(valid, message, n_bad, first_bad, bad) as the library must report them; w holds the values as the
    .wtns file does (unreduced values allowed here: they are a verdict of their own)."""
    n = len(r1cs.constraints)
    if w[0] != 1:
        return False, "INVALID: signal 0 is not 1", 0, None, []
    for i, v in enumerate(w):
        if v >= R:
            return False, "INVALID: signal %d is not reduced" % i, 0, None, []
    bad = failing(r1cs, w)
    if bad:
        return (False, "INVALID: constraint %d is not satisfied (%d of %d fail)" % (bad[0], len(bad), n), len(bad), bad[0],
                bad[:16])
    return True, "OK", 0, None, []


class Hard:
    """r1cs, its satisfying witness w, bad_r1cs (one more constraint, a designed failure: A empty, C = w0),
    defining[c] (the wire constraint c defines, or None) and probes {(L, "first" | "last"): wire}: a wire
    that occurs only as term 0 / term L - 1 of one row of L terms."""


def _build() -> Hard:
    rng = SplitMix64(0x77746E73, 7)
    w = [1]
    for k in range(NPOOL):  # input values from {0, 1, r - 1, random}
        w.append((0, 1, R - 1, None)[k % 4] if k % 4 != 3 else rng.fr())
    cons, defining = [], []

    def coef():
        x = rng.below(4)
        if x == 0:
            return 1
        if x == 1:
            return R - 1
        if x == 2:
            return 1 << rng.below(254)
        return rng.fr() or 1

    def wire():
        # wire 0, the first and the last input and any other; repeats inside a row happen by themselves
        x = rng.below(8)
        return 0 if x == 0 else 1 if x == 1 else NPOOL if x == 2 else 1 + rng.below(NPOOL)

    def row(n):
        return [(wire(), coef()) for _ in range(n)]

    def new_wire(value):
        w.append(value % R)
        return len(w) - 1

    def define(lc, where):
        """(lc)(w0) = d with the long row in A or B, or (d)(w0) = lc with it in C; d = ev(lc)"""
        d = new_wire(ev(lc, w))
        one, dd = [(0, 1)], [(d, 1)]
        cons.append({"A": (lc, one, dd), "B": (one, lc, dd), "C": (dd, one, lc)}[where])
        defining.append(d)

    for where in "ABC":
        for n in range(301):
            define(row(n), where)
    for n in range(101):  # all three rows n terms; C's last term is the defining wire
        a, b = row(n), row(n)
        if n == 0:
            cons.append(([], [], []))  # A, B and C all empty: satisfied
            defining.append(None)
            continue
        c = row(n - 1)
        d = new_wire(ev(a, w) * ev(b, w) - ev(c, w))
        cons.append((a, b, c + [(d, 1)]))
        defining.append(d)
    define(row(4097), "A")
    define(row(70001), "B")
    define(row(4097), "C")
    define([(1 + rng.below(NPOOL), rng.fr() or 1), (5, 0), (2, 3)], "A")  # an explicit zero coefficient
    # exact cancellation: every term nonzero (wire 2 is 1, wire 3 is r - 1), the row's sum 0 mod r
    for n in (2, 64, 130, 300):
        lc = []
        for _ in range(n // 2):
            c = rng.fr() or 1
            s = (2, 3)[rng.below(2)]
            lc += [(s, c), (s, R - c)]
        assert ev(lc, w) == 0 and all(c * w[s] % R for s, c in lc)
        define(lc, "ABC"[n % 3])
    # many (r - 1)(r - 1) terms: the sum of the unreduced products wraps r hundreds of times
    for n, where in ((40, "A"), (300, "B"), (5000, "C")):
        define([(3, R - 1)] * n, where)
    # probes: a wire of its own as term 0, another as term L - 1, of a row of L terms
    probes = {}
    for n in PROBE_LENGTHS:
        first, last = new_wire(rng.fr()), new_wire(rng.fr())
        probes[(n, "first")], probes[(n, "last")] = first, last
        define([(first, rng.fr() or 1)] + row(n - 2) + [(last, rng.fr() or 1)], "A")
    if len(cons) % 64 == 0:
        define(row(3), "A")
    assert len(cons) % 64 and len(cons) % 256
    h = Hard()
    h.w = w
    h.r1cs = R1CS(len(w), 2, len(cons), cons)
    h.bad_r1cs = R1CS(len(w), 2, len(cons) + 1, cons + [([], [(0, 1)], [(0, 1)])])  # 0 * 1 = 1
    h.defining = defining
    h.probes = probes
    return h


def hard_circuit() -> Hard:
    if "h" not in _cache:
        _cache["h"] = _build()
    return _cache["h"]


def mutations(h: Hard = None):
    """name -> witness: the mutations of the hard circuit's witness that the tests reject"""
    h = h or hard_circuit()
    n = h.r1cs.n_constraints

    def bump(wire, by):
        m = list(h.w)
        m[wire] = (m[wire] + by) % R
        return m

    out = {
        "first_plus_1": bump(h.defining[0], 1),
        "last_minus_1": bump(h.defining[n - 1], -1),
        "c255_plus_1": bump(h.defining[255], 1),
        "c256_minus_1": bump(h.defining[256], -1),
        "all_zero": [1] + [0] * (len(h.w) - 1),
    }
    for (length, end), wire in sorted(h.probes.items()):
        out["probe_%d_%s" % (length, end)] = bump(wire, 1)
    return out
