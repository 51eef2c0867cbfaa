"""Designed MSM inputs that force the general XYZZ addition (csrc/curve.hpp xyzz_add) into its doubling
and cancellation branches in every stage of the pipeline after the buckets are filled: the heavy-bucket
merges, the row / column chains, the shuffle butterfly, the segment sums and the subset-sum trees.

A design is a list of entries (point name, window, bucket index k).  An entry is one base with the scalar
(k + 1) << (c * window): a single nonzero digit k + 1 <= 2^(c-1), which the signed-digit recoding leaves
alone, so the base lands in bucket k of that window and nowhere else.  Negatives are explicit bases -P.
Every point is a small multiple of one generator multiple P or Q, so the oracle's MSM over the design is a
handful of scalar multiplications (the entries of one point are summed first).

The geometry (rows U, columns V, chain lengths, partials per sum, segment size, subset-sum values, task
sizes, and whether the subset sums start with trees or a chain level) is computed here from the window bits
the way MsmParams / rowcol_make / run_finish do; tests assert it against what tools/hosttest/msm_emu
prints, so that a change of the engine's constants fails loudly instead of quietly moving the collisions.

Plain module (no tests): tests/test_host_xyzz_events.py certifies on the CPU that every design reaches
the (stage, kind) it declares; tests/test_gpu_xyzz_events.py runs the same catalogue on the GPU."""
import collections

from oracle import bn254, groth16

R = bn254.R
TASK = 48          # accumulate task size of the kernel-level entry points (apply_task_options)
S2 = 4             # fan-in of a heavy-bucket merge level
CHAIN, SPAN = 8, 128     # msmk::ROWCOL_CHAIN / ROWCOL_SPAN
TREE_TPB, TREE_CHAIN_FAN, TREE_FIRST_MAX = 256, 4, 512

# multiples of the two independent-looking generator multiples the designs use
_A, _B = 0x1F3D5B79A2C4E6F80123456789ABCDEF, 0x0FEDCBA987654321F6E8D4C2B0A39175
MULT = {"P": _A, "-P": -_A, "2P": 2 * _A, "-2P": -2 * _A, "Q": _B}

# (c, table depth (0: every row), segment override (0: the default M = 4))
CONFIGS = [(8, 1, 0), (8, 0, 0), (9, 1, 0), (9, 0, 0), (13, 1, 0), (13, 0, 0), (16, 1, 0), (16, 0, 0),
           (20, 0, 0), (20, 0, 1), (20, 1, 1)]


class Geometry:
    def __init__(self, c, depth=0, seg=0):
        self.c, self.seg = c, seg
        self.windows = (255 + c - 1) // c
        self.depth = min(depth, self.windows) if depth > 0 else self.windows
        self.groups = (self.windows + self.depth - 1) // self.depth
        self.V = 1 << (c // 2)
        self.U = 1 << (c - 1 - c // 2)
        self.M = min(4, self.V)
        if 0 < seg <= self.V:
            self.M = seg
        self.Lr = min(self.V, max(CHAIN, self.V // SPAN))
        self.Lc = min(self.U, max(CHAIN, self.U // SPAN))
        self.nr, self.nc = self.V // self.Lr, self.U // self.Lc
        self.P = self.V // self.M
        self.lgP = self.P.bit_length() - 1
        self.K = self.lgP + 1
        self.S, self.S2 = TASK, S2
        ch = 2 * TREE_TPB
        self.chunks = (self.P + ch - 1) // ch
        self.first = "tree" if 2 * self.groups * self.K * self.chunks <= TREE_FIRST_MAX else "chain"
        if self.first == "chain":
            self.chunks = (self.P + 2 * TREE_CHAIN_FAN - 1) // (2 * TREE_CHAIN_FAN)

    def merge_levels(self, n):
        m, levels = (max(n, 1) * self.depth + self.S - 1) // self.S, 0
        while m > 2 * self.S2:
            m, levels = (m + self.S2 - 1) // self.S2, levels + 1
        return levels

    def line(self, n):
        """what `msm_emu --events` prints for this geometry and n bases"""
        return ("geometry c=%d windows=%d depth=%d groups=%d U=%d V=%d Lr=%d Lc=%d nr=%d nc=%d M=%d P=%d S=%d S2=%d "
                "levels=%d first=%s chunks=%d" % (self.c, self.windows, self.depth, self.groups, self.U, self.V,
                                                  self.Lr, self.Lc, self.nr, self.nc, self.M, self.P, self.S, self.S2,
                                                  self.merge_levels(n), self.first, self.chunks))

    def emu_args(self):
        return [str(self.c), str(self.depth), "--task", str(self.S)] + (["--seg", str(self.seg)] if self.seg else [])

    def zkp_msm(self, plan):
        """the ZKP_MSM setting that gives the GPU entry points this geometry"""
        return "plan=" + plan + (",seg=%d" % self.seg if self.seg else "")


Design = collections.namedtuple("Design", "name entries targets")   # targets: [(stage, kind)], kind dbl | cancel | ...


def _pow2_below(n):
    m = 1
    while m < n:
        yield m
        m *= 2


def designs(geo):
    """the catalogue for one geometry.  Every design sits in one window: window 1 (group 1) for a table of
    depth 1, window 0 otherwise."""
    w = 1 if geo.depth == 1 else 0
    V, Lr, Lc, M, P = geo.V, geo.Lr, geo.Lc, geo.M, geo.P
    out = []

    def b(u, v):
        assert 0 <= u < geo.U and 0 <= v < V
        return u * V + v

    def add(name, cells, targets):
        out.append(Design(name, [(pt, w, k) for pt, k in cells], targets))

    def pair(name, k0, k1, stage, behind=None, chain=False):
        """P in bucket k0 and +-P in bucket k1 (with Q in the bucket `behind` the resulting infinity, which
        a chain then adds to it in the same stage)"""
        add(name + "_dbl", [("P", k0), ("P", k1)], [(stage, "dbl")])
        cells = [("P", k0), ("-P", k1)] + ([("Q", behind)] if behind is not None else [])
        add(name + "_cancel", cells, [(stage, "cancel")] + ([(stage, "acc_inf")] if chain else []))

    wide = geo.c == 20      # c = 20 runs for the whole-wave butterfly and the tree levels only
    if not wide:
        # a chain of Lr neighbouring buckets of row 1 / of Lc buckets V apart of column 3
        pair("row_chain", b(1, 0), b(1, 1), "rowcol_chain.row", behind=b(1, 2), chain=True)
        pair("col_chain", b(1, 3), b(2, 3), "rowcol_chain.col", behind=b(3, 3), chain=True)
        # row 0 has weight 0 and no slot: its lanes of the butterfly hold infinity, its buckets meet the
        # column chains only.  P twice in row 0 (no row sum may see them) and once more below the first.
        add("row0_dbl", [("P", b(0, 5)), ("P", b(0, 6)), ("P", b(1, 5))], [("rowcol_chain.col", "dbl")])
        add("row0_cancel", [("P", b(0, 5)), ("-P", b(0, 6)), ("-P", b(1, 5)), ("Q", b(2, 5))],
            [("rowcol_chain.col", "cancel"), ("rowcol_chain.col", "acc_inf")])
        # the two partials of one lane
        if geo.nr >= 2:
            pair("row_pair", b(1, 0), b(1, Lr), "rowcol_tree.row.pair", behind=b(1, 2 * Lr) if geo.nr >= 4 else None)
        if geo.nc >= 2:
            pair("col_pair", b(1, 0), b(1 + Lc, 0), "rowcol_tree.col.pair",
                 behind=b(1 + 2 * Lc, 0) if geo.nc >= 4 else None)
    if geo.seg == 0:
        # lanes l and l ^ m of a sum: partials 2l and 2(l ^ m)
        for m in _pow2_below(geo.nr // 2):
            pair("row_bfly%d" % m, b(1, 0), b(1, 2 * m * Lr), "rowcol_tree.row.bfly.%d" % m)
        for m in _pow2_below(geo.nc // 2):
            pair("col_bfly%d" % m, b(1, 0), b(1 + 2 * m * Lc, 0), "rowcol_tree.col.bfly.%d" % m)
    if not wide and M >= 2:
        # running sums of a segment of the column sub-group (X_v = column sum v), from its last point down:
        # R = X_(M-1) + X_(M-2) = P - P;  T = X_(M-1) + R = P + (P - 2P)
        add("segment_R_cancel", [("P", b(1, M - 1)), ("-P", b(2, M - 2)), ("Q", b(3, 0))],
            [("reduce_segments.R", "cancel")])
        add("segment_T_cancel", [("P", b(1, M - 1)), ("-2P", b(2, M - 2)), ("Q", b(3, 0))],
            [("reduce_segments.T", "cancel")])

    # subset sums: columns j + p M and j + p' M hold +-P (in rows 1 and 2), so that segments p and p' of the
    # column sub-group have equal (opposite) S and T; value p of the sum of all T sits in thread p % 256 of
    # chunk p / 512, load p / 256 % 2
    def subset(name, p0, p1, stage):
        pair(name, b(1, p0 * M + M - 1), b(2, p1 * M + M - 1), stage)

    if geo.first == "tree":
        if not (wide and geo.seg):
            for sh in _pow2_below(min(P, TREE_TPB)):        # threads 1 and 1 + sh meet at LDS level sh
                if (wide and sh < 64) or 1 + sh >= P:
                    continue
                subset("subset_lds%d" % sh, 1, 1 + sh, "subset_tree.lds.%d" % sh)
        if P >= 2 * TREE_TPB:
            subset("subset_own_loads", 1, 1 + TREE_TPB, "subset_tree.load1")
        if geo.chunks == 2:                                 # chunk sums 0 and 1: threads 0 and 1 of the next level
            subset("subset_chunks", 1, 1 + 2 * TREE_TPB, "subset_next.lds.1")
    else:
        subset("subset_chain", 1, 2, "subset_first")        # one thread's 2 * TREE_CHAIN_FAN values
        sh = geo.chunks // 2                                # chain outputs 0 and sh: threads 0 and sh
        subset("subset_chain_lds%d" % sh, 1, 1 + 2 * TREE_CHAIN_FAN * sh, "subset_next.lds.%d" % sh)

    if not wide:
        # heavy buckets.  The device's order inside a bucket is unspecified, so what a GPU run is known to
        # reach are the designs whose task partials do not depend on it: all entries equal (the *_dbl
        # designs), and S entries P with S entries -P (final_cancel: the two partials are opposite or both
        # infinity in any order).  The heavy*_cancel designs reach their branch in the replay's stable order
        # only; on the GPU they still have to give the oracle's sum, in whatever order.
        S, k = geo.S, b(1, 1)
        add("final_dbl", [("P", k)] * (2 * S), [("merge_final", "dbl")])
        add("final_cancel", [("P", k)] * S + [("-P", k)] * S + [("Q", b(1, 2))], [("merge_final", "cancel")])
        levels = [0, 1] if geo.c == 8 else [0]
        for lv in levels:
            tasks = 2 * S2 * S2 ** lv + 1                   # more than 2 * S2 partials enter level lv
            add("heavy%d_dbl" % lv, [("P", k)] * (tasks * S), [("merge_heavy.%d" % lv, "dbl")])
            # blocks of S2^lv * S entries P, then as many -P, ...: in the replay's order the partials that
            # enter level lv alternate
            cells = []
            for t in range(tasks):
                cells += [("-P" if (t // S2 ** lv) & 1 else "P", k)] * S
            add("heavy%d_cancel" % lv, cells + [("Q", b(1, 2))], [("merge_heavy.%d" % lv, "cancel")])
    return out


# every (stage, level) x {dbl, cancel} the catalogue must reach over CONFIGS (reduce_segments: cancel only)
def required():
    req = []
    stages = ["rowcol_chain.row", "rowcol_chain.col", "rowcol_tree.row.pair", "rowcol_tree.col.pair"]
    stages += ["rowcol_tree.row.bfly.%d" % m for m in (1, 2, 4, 8, 16, 32)]      # nr = 128 at c = 20: a whole wave
    stages += ["rowcol_tree.col.bfly.%d" % m for m in (1, 2, 4, 8, 16)]
    stages += ["subset_tree.load1"] + ["subset_tree.lds.%d" % sh for sh in (1, 2, 4, 8, 16, 32, 64, 128)]
    stages += ["subset_first", "subset_next.lds.1", "subset_next.lds.64"]
    stages += ["merge_final", "merge_heavy.0", "merge_heavy.1"]
    for s in stages:
        req += [(s, "dbl"), (s, "cancel")]
    return req + [("reduce_segments.R", "cancel"), ("reduce_segments.T", "cancel")]


class Points:
    """the designs' points on one curve"""

    def __init__(self, curve):
        self.curve = curve
        g2 = curve == "g2"
        fb = bn254.FixedBase(bn254.G2_GEN if g2 else bn254.G1_GEN, g2)
        self.pt = {name: fb.mul(m % R) for name, m in MULT.items()}
        self.enc = bn254.g2_to_lem if g2 else bn254.g1_to_lem
        self.lem = {name: self.enc(p) for name, p in self.pt.items()}
        self._want = {}

    def encode(self, design, c):
        """(points in zkey layout, scalars as 32-byte LE, n)"""
        pts = b"".join(self.lem[pt] for pt, _, _ in design.entries)
        sc = b"".join(bn254.int_to_le((k + 1) << (c * w)) for _, w, k in design.entries)
        return pts, sc, len(design.entries)

    def expected(self, design, c):
        """the oracle's MSM of the design, the scalars of one point summed first"""
        tot = collections.OrderedDict()
        for pt, w, k in design.entries:
            tot[pt] = tot.get(pt, 0) + ((k + 1) << (c * w))
        key = (c, tuple(tot.items()))
        if key not in self._want:
            msm = groth16.msm_g2 if self.curve == "g2" else groth16.msm_g1
            self._want[key] = msm([self.pt[p] for p in tot], [s % R for s in tot.values()])
        return self._want[key]


def parse_emu(stdout):
    """`msm_emu --events` output -> (geometry line, result, {stage: {kind: count}})"""
    geo, res, ev = None, None, {}
    for ln in stdout.strip().split("\n"):
        if ln.startswith("geometry "):
            geo = ln
        elif ln.startswith("event "):
            f = ln.split()
            ev[f[1]] = dict(zip(("dbl", "cancel", "acc_inf", "q_inf"), map(int, f[2:6])))
        elif ln == "inf":
            res = None
        else:
            v = [int(t) for t in ln.split()]
            res = tuple(v) if len(v) == 2 else ((v[0], v[1]), (v[2], v[3]))
    return geo, res, ev
