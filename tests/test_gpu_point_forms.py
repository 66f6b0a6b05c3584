"""Every point-addition form of the MSMs at the bounds its comments argue, one form and one coordinate at a time.

The bucket accumulation and its reduction tail run on hand-built additions in the lazy radix-2^29 representation (csrc/lazy29.cuh,
quad29.cuh, fold_park.cuh and the two generated bodies of madd_asm.inc).  Whole MSMs only ever feed them curve points, whose limbs look
uniformly random; here tests/cpp/point_forms_check.hip calls the product's own functions on raw limb vectors, so every coordinate of
every form sits at every corner of its contract, and Python integers evaluate the published formulas (madd-2008-s, add-2008-s,
dbl-2008-s-1, dbl-2009-l, add-2007-bl / madd-2007-bl) mod p.  The formulas are polynomial identities: operands need not lie on the curve.

Three layers share one generator of operands:
  * unmarked (no GPU): the generator's self-check, the host compilation of the one-lane C++ forms, the CPU simulation of the two asm
    bodies (tools/gen_madd_asm.simulate), the share of jobs that fall into the same-x branch;
  * gpu: ONE run of the harness per module (all jobs, the asm bodies as waves, the chains), then tests that read its result file.

Operand contracts (per component; p = the base field's modulus, "normal form" = limbs 0..7 in [0, 2^29), top limb signed):
  M   a Montgomery output: normal form in (-p/4, 1.3 p)                                  (lazy29.cuh header)
  X   X3 = norm(RR - PPP - 2Q) of three Montgomery outputs: (-4.15 p, 2.05 p)
  Y1  G1 accumulator Y = mont_diff(..): |value| < 3 p                                    (mont_diff's comment)
  YR  the Y register of the asm bodies (Y3 after the odd body, -Y3 after the even): (-p/4, 3 p)  (the generator's range assertion)
  Y2  G2 accumulator Y = norm(R D - Y PPP), two Fq2 products: (-1.55 p, 1.55 p)
  T   a table coordinate: canonical, [0, p);  TS  the same or its limb-wise negation (limbs <= 0);  TY  TS normalised: (-p, p)
  JX, JY, JZ  a Jacobian accumulator of the tail: a canonical load or the output of one dbl_lazy / add_lazy on such:
      D = 2 (t - A - C) in (-5.7 p, 3.6 p), X3 = E^2 - 2 D in (-7.45 p, 12.7 p), Y3 = E (D - X3) - 8 C in (-10.65 p, 3.3 p),
      Z3 = 2 Y Z in (-p/2, 2.6 p); every Jacobian output must stay a normal form with |value| < 16 p (store_exact's range).
Every XYZZ form must return X in X, Y in Y1 / Y2, ZZ and ZZZ in M: the contracts are closed, which the chains check under iteration.
"""
import functools
import hashlib
import os
import random
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("tools", "oracle"):
    if os.path.join(ROOT, _d) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, _d))
import gen_madd_asm as GM          # noqa: E402
from gen_mont_asm import FQ, model, value   # noqa: E402
import pyref                        # noqa: E402

P = pyref.Q
assert value(FQ["P29"]) == P
M29 = (1 << 29) - 1
R261 = 1 << 261
RINV = pow(R261, -1, P)
K = {1: pyref._Fq1Ops, 2: pyref._Fq2Ops}
CSRC = os.path.join(ROOT, "zksnark_rs_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpp", "point_forms_check.hip")
MAGIC, JOB_IN, JOB_OUT, ASM_IN, ASM_OUT, NOT_RUN = 0x50464331, 148, 76, 74, 80, -99
FORM_CODE = dict(madd_xyzz=0, madd_xyzz_nz=1, madd_xyzz_second=2, add_xyzz=3, dbl_xyzz=4, add_xyzz_from=5, add_xyzz_from_parked=6, dbl_lazy=7,
                 add_lazy=8, madd_lazy=9, mul_small_lazy=10, quad_add_xyzz=11, quad_dbl_xyzz=12, quad_mul_small_xyzz=13)
HOST_FORMS = {"madd_xyzz", "madd_xyzz_nz", "madd_xyzz_second", "add_xyzz", "dbl_xyzz", "dbl_lazy", "add_lazy", "madd_lazy", "mul_small_lazy"}
QUAD_FORMS = {"quad_add_xyzz", "quad_dbl_xyzz", "quad_mul_small_xyzz"}
SAME_X_CAP = 0.10
NCORNER = 17                        # a prime: the orthogonal design below covers every pair of corners of every two coordinates


def normal_form(v):
    out = []
    for _ in range(8):
        out.append(v & M29)
        v >>= 29
    out.append(v)
    return out


def neg(l):
    return [-x for x in l]


# ---- operand domains ------------------------------------------------------------------------------------------------------
class Dom:
    """normal forms with lo < value < hi; signed: also the limb-wise negations of such"""

    def __init__(self, name, lo, hi, signed=False):
        self.name, self.lo, self.hi, self.signed = name, lo, hi, signed

    def contains(self, l):
        if self.signed and all(x <= 0 for x in l) and any(x < 0 for x in l):
            l = neg(l)
        return len(l) == 9 and all(0 <= x <= M29 for x in l[:8]) and self.lo < value(l) < self.hi and abs(l[8]) < (1 << 31)

    @functools.lru_cache(maxsize=None)
    def extremes(self):
        """low limbs all 2^29 - 1 / all 0 / alternating both ways, each with the top limb at both ends of the range and at 0"""
        out = []
        for low in ([M29] * 8, [0] * 8, [M29 if i % 2 else 0 for i in range(8)], [0 if i % 2 else M29 for i in range(8)]):
            lv = value(low + [0])
            tmax = (self.hi - 1 - lv) >> 232
            tmin = -((lv - self.lo - 1) >> 232)
            assert tmin <= tmax
            out += [low + [tmax], low + [tmin], low + [0 if tmin <= 0 <= tmax else tmin]]
        return out

    @functools.lru_cache(maxsize=None)
    def near_multiples(self):
        """k p + d, d in {-1, 0, 1}, for every k in the range"""
        out = []
        for k in range(self.lo // P - 1, self.hi // P + 2):
            for d in (-1, 0, 1):
                if self.lo < k * P + d < self.hi:
                    out.append(normal_form(k * P + d))
        return out

    def random(self, rng):
        l = normal_form(rng.randrange(self.lo + 1, self.hi))
        return neg(l) if self.signed and rng.random() < 0.5 else l

    @functools.lru_cache(maxsize=None)
    def corners(self):
        """NCORNER vectors: the twelve extremes, the two ends of the value range, two values next to a multiple of p, one random fill;
        a signed domain takes every second one negated"""
        rng = random.Random("corners " + self.name)
        nm = [l for l in self.near_multiples() if value(l) % P]
        c = self.extremes() + [normal_form(self.lo + 1), normal_form(self.hi - 1), nm[0], nm[-1], self.random(rng)]
        assert len(c) == NCORNER
        if self.signed:
            c = [neg(l) if i % 2 and any(l) else l for i, l in enumerate(c)]
        return c

    @functools.lru_cache(maxsize=None)
    def everything(self):
        rng = random.Random("all " + self.name)
        out = self.corners() + self.near_multiples() + [self.random(rng) for _ in range(8)]
        if self.signed:
            out += [neg(l) for l in self.extremes() + self.near_multiples() if any(l)]
        return out


DOM = {d.name: d for d in (
    Dom("M", -P // 4, 13 * P // 10), Dom("X", -415 * P // 100, 205 * P // 100), Dom("Y1", -3 * P, 3 * P), Dom("YR", -P // 4, 3 * P),
    Dom("Y2", -155 * P // 100, 155 * P // 100), Dom("T", -1, P), Dom("TS", -1, P, signed=True), Dom("TY", -P, P),
    Dom("JX", -745 * P // 100, 127 * P // 10), Dom("JY", -1065 * P // 100, 33 * P // 10), Dom("JZ", -P // 2, 26 * P // 10), Dom("J16", -16 * P, 16 * P))}


def ydom(field):
    return "Y1" if field == 1 else "Y2"


# operand slots: 0..3 = A.X, A.Y, A.ZZ (Jacobian: Z), A.ZZZ; 4..7 = B.X (affine: qx), B.Y (qy), B.ZZ, B.ZZZ
SLOT = ("A.X", "A.Y", "A.ZZ", "A.ZZZ", "B.X", "B.Y", "B.ZZ", "B.ZZZ")


def form_inputs(form, field):
    """the contract of every operand coordinate of a form, derived from its producers (see the module docstring)"""
    y = ydom(field)
    acc = [(0, "X"), (1, y), (2, "M"), (3, "M")]                 # an accumulator image: what the XYZZ forms themselves return
    pt = [(4, "T"), (5, "TS")]                                   # a table point, y negated by the digit's sign
    jac = [(0, "JX"), (1, "JY"), (2, "JZ")]
    return {
        "madd_xyzz": acc + pt, "madd_xyzz_nz": acc + pt,
        "madd_xyzz_second": [(0, "T"), (1, "TY")] + pt,          # the accumulator still is the run's first point: (qx, qy.norm()), ZZ = ZZZ = 1
        "add_xyzz": acc + [(4, "X"), (5, y), (6, "M"), (7, "M")],
        "dbl_xyzz": acc, "dbl_lazy": jac,
        "add_lazy": jac + [(4, "JX"), (5, "JY"), (6, "JZ")],
        "madd_lazy": [(0, "X"), (1, "Y2"), (2, "M")] + pt,       # madd_lazy's own outputs: X3 as above, Y3 = norm of two products, Z3 = Z H
    }[form]


SHARES_OPERANDS = {"add_xyzz_from": "add_xyzz", "add_xyzz_from_parked": "add_xyzz", "quad_add_xyzz": "add_xyzz", "quad_dbl_xyzz": "dbl_xyzz"}
PATTERN_FORMS = {1: ["madd_xyzz", "madd_xyzz_nz", "madd_xyzz_second", "add_xyzz", "dbl_xyzz", "add_xyzz_from", "dbl_lazy", "add_lazy", "madd_lazy",
                     "quad_add_xyzz", "quad_dbl_xyzz"]}
PATTERN_FORMS[2] = PATTERN_FORMS[1] + ["add_xyzz_from_parked"]
ASM_INPUTS = [("X", "X"), ("Y", "YR"), ("ZZ", "M"), ("ZZZ", "M"), ("qx", "T"), ("qy", "TS")]


def design(coords, seed, extra=111):
    """coords: domain names, one per coordinate (at most NCORNER).  Rows (a, b) of an orthogonal array over the NCORNER corners --
    coordinate c takes corner (a + c b) mod NCORNER, so every two coordinates meet in every pair of corners exactly once -- then
    `extra` rows drawn from everything the domains list (all k p + d, negations, random fill)."""
    assert len(coords) <= NCORNER
    rows = [[DOM[d].corners()[(a + c * b) % NCORNER] for c, d in enumerate(coords)] for a in range(NCORNER) for b in range(NCORNER)]
    rng = random.Random(seed)
    rows += [[rng.choice(DOM[d].everything()) for d in coords] for _ in range(extra)]
    return rows


@functools.lru_cache(maxsize=None)
def pattern_jobs(form, field):
    src = SHARES_OPERANDS.get(form, form)
    ins = form_inputs(src, field)
    coords = [(slot, comp, d) for slot, d in ins for comp in range(field)]
    jobs = []
    for row in design([d for _, _, d in coords], "%s %d" % (src, field)):
        ops = {}
        for (slot, comp, _), l in zip(coords, row):
            ops.setdefault(slot, [None] * field)[comp] = l
        jobs.append(dict(form=form, field=field, ops=ops, flags=0, k=0))
    return jobs


@functools.lru_cache(maxsize=None)
def asm_pattern_lanes():
    """the operands of the pattern lanes of both bodies; the Y register holds Y (even) or -Y (odd)"""
    return [dict(zip([n for n, _ in ASM_INPUTS], row)) for row in design([d for _, d in ASM_INPUTS], "asm")]


# ---- the reference: published formulas on residues -------------------------------------------------------------------------
def elem(field, comps):
    """the field element a coordinate stands for (operands are Montgomery images: value 2^-261 mod p)"""
    e = tuple(value(c) * RINV % P for c in comps)
    return e[0] if field == 1 else e


def job_elems(job):
    return {s: elem(job["field"], c) for s, c in job["ops"].items()}


def ref_madd(F, X1, Y1, ZZ1, ZZZ1, x2, y2):
    """madd-2008-s; returns (branch, X3, Y3, ZZ3, ZZZ3): branch 'same' / 'opp' when P^2 == 0 (then R^2 == 0 decides)"""
    Pd, Rd = F.sub(F.mul(x2, ZZ1), X1), F.sub(F.mul(y2, ZZZ1), Y1)
    PP = F.mul(Pd, Pd)
    if PP == F.zero:
        return ("same" if F.mul(Rd, Rd) == F.zero else "opp",)
    PPP, Q = F.mul(Pd, PP), F.mul(X1, PP)
    X3 = F.sub(F.sub(F.mul(Rd, Rd), PPP), F.add(Q, Q))
    return "sum", X3, F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(Y1, PPP)), F.mul(ZZ1, PP), F.mul(ZZZ1, PPP)


def ref_add(F, X1, Y1, ZZ1, ZZZ1, X2, Y2, ZZ2, ZZZ2):
    """add-2008-s"""
    U1, U2, S1, S2 = F.mul(X1, ZZ2), F.mul(X2, ZZ1), F.mul(Y1, ZZZ2), F.mul(Y2, ZZZ1)
    Pd, Rd = F.sub(U2, U1), F.sub(S2, S1)
    PP = F.mul(Pd, Pd)
    if PP == F.zero:
        return ("same" if F.mul(Rd, Rd) == F.zero else "opp",)
    PPP, Q = F.mul(Pd, PP), F.mul(U1, PP)
    X3 = F.sub(F.sub(F.mul(Rd, Rd), PPP), F.add(Q, Q))
    return "sum", X3, F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(S1, PPP)), F.mul(F.mul(ZZ1, ZZ2), PP), F.mul(F.mul(ZZZ1, ZZZ2), PPP)


def ref_dbl(F, X1, Y1, ZZ1, ZZZ1):
    """dbl-2008-s-1 with a = 0"""
    U = F.add(Y1, Y1)
    V = F.mul(U, U)
    W, S = F.mul(U, V), F.mul(X1, V)
    M = F.mul(F.small(3), F.mul(X1, X1))
    X3 = F.sub(F.mul(M, M), F.add(S, S))
    return "sum", X3, F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, Y1)), F.mul(V, ZZ1), F.mul(W, ZZZ1)


def ref_dbl_jac(F, X1, Y1, Z1):
    """dbl-2009-l"""
    A, B = F.mul(X1, X1), F.mul(Y1, Y1)
    C = F.mul(B, B)
    t = F.add(X1, B)
    D = F.mul(F.small(2), F.sub(F.sub(F.mul(t, t), A), C))
    E = F.mul(F.small(3), A)
    X3 = F.sub(F.mul(E, E), F.add(D, D))
    return "sum", X3, F.sub(F.mul(E, F.sub(D, X3)), F.mul(F.small(8), C)), F.mul(F.small(2), F.mul(Y1, Z1))


def ref_add_jac(F, X1, Y1, Z1, X2, Y2, Z2):
    """add-2007-bl.  The code drops the formula's constant factors: its (X, Y, Z) is this one's (X3 / 4, Y3 / 8, Z3 / 2) -- the same
    point (lambda = 2) -- so the outputs are compared as 4 X, 8 Y, 2 Z (JAC_SCALE)."""
    Z1Z1, Z2Z2 = F.mul(Z1, Z1), F.mul(Z2, Z2)
    U1, U2 = F.mul(X1, Z2Z2), F.mul(X2, Z1Z1)
    S1, S2 = F.mul(F.mul(Y1, Z2), Z2Z2), F.mul(F.mul(Y2, Z1), Z1Z1)
    H = F.sub(U2, U1)
    r = F.mul(F.small(2), F.sub(S2, S1))
    if F.mul(H, H) == F.zero:
        return ("same" if F.mul(r, r) == F.zero else "opp",)
    I = F.mul(F.small(4), F.mul(H, H))
    J, V = F.mul(H, I), F.mul(U1, I)
    X3 = F.sub(F.sub(F.mul(r, r), J), F.add(V, V))
    Y3 = F.sub(F.mul(r, F.sub(V, X3)), F.mul(F.small(2), F.mul(S1, J)))
    zs = F.add(Z1, Z2)
    return "sum", X3, Y3, F.mul(F.sub(F.sub(F.mul(zs, zs), Z1Z1), Z2Z2), H)


def ref_madd_jac(F, X1, Y1, Z1, x2, y2):
    """madd-2007-bl; scaled like add-2007-bl"""
    return ref_add_jac(F, X1, Y1, Z1, x2, y2, F.small(1))


JAC_SCALE = (4, 8, 2)


def reference(job):
    """(branch, outputs...) of a job by the published formula of its form"""
    F, e, form = K[job["field"]], job_elems(job), job["form"]
    a = [e.get(i) for i in range(8)]
    if form in ("madd_xyzz", "madd_xyzz_nz"):
        return ref_madd(F, a[0], a[1], a[2], a[3], a[4], a[5])
    if form == "madd_xyzz_second":
        return ref_madd(F, a[0], a[1], F.small(1), F.small(1), a[4], a[5])
    if form in ("add_xyzz", "add_xyzz_from", "add_xyzz_from_parked", "quad_add_xyzz"):
        return ref_add(F, *a)
    if form in ("dbl_xyzz", "quad_dbl_xyzz"):
        return ref_dbl(F, *a[:4])
    if form == "dbl_lazy":
        return ref_dbl_jac(F, *a[:3])
    if form == "add_lazy":
        return ref_add_jac(F, a[0], a[1], a[2], a[4], a[5], a[6])
    if form == "madd_lazy":
        return ref_madd_jac(F, a[0], a[1], a[2], a[4], a[5])
    raise KeyError(form)


def is_jac(form):
    return form in ("dbl_lazy", "add_lazy", "madd_lazy", "mul_small_lazy")


def output_contract(form, field):
    """names and domains of the coordinates a form returns"""
    if is_jac(form):
        return [("X", "J16"), ("Y", "J16"), ("Z", "J16")]
    return [("X", "X"), ("Y", ydom(field)), ("ZZ", "M"), ("ZZZ", "M")]


def expected_flags(form, branch, job=None):
    """(status, inf) a form reports for the branch the reference takes; None = not specified"""
    if form in ("madd_xyzz", "madd_lazy"):                 # returns false when the caller must double
        return {"sum": (1, 0), "same": (0, 0), "opp": (1, 1)}[branch]
    if form in ("madd_xyzz_nz", "madd_xyzz_second"):       # 0 sum, 1 caller doubles, 2 infinity (accumulator left as it was)
        return {"sum": (0, 0), "same": (1, 0), "opp": (2, 0)}[branch]
    if form == "add_xyzz" and branch == "same" and job is not None:
        # add_xyzz doubles through the Jacobian image (X ZZ^2, Y ZZZ^2, ZZZ), where Z = ZZZ == 0 IS infinity: off the curve only
        return 0, int(elem(job["field"], job["ops"][3]) == K[job["field"]].zero)
    return {"sum": (0, 0), "same": (0, 0), "opp": (0, 1)}[branch]    # the general additions double themselves


class Out:
    """one lane's record of a job result"""

    def __init__(self, rec, field):
        self.status, self.inf = int(rec[0]), int(rec[1])
        self.coords = [[[int(x) for x in rec[4 + 18 * c + 9 * k:13 + 18 * c + 9 * k]] for k in range(field)] for c in range(4)]


def check_job(job, res, where, lanes=(0,)):
    """(a) residues, (b) output contract, (c) branch flags of one pattern job; returns the reference's branch"""
    form, field = job["form"], job["field"]
    ref = reference(job)
    branch = ref[0]
    for lane in lanes:
        out = Out(res[lane], field)
        tag = "%s G%d %s lane %d" % (form, field, where, lane)
        assert out.status != NOT_RUN, tag + ": the harness did not run this form"
        assert (out.status, out.inf) == expected_flags(form, branch, job), "%s: status / inf %s for branch '%s'" % (tag, (out.status, out.inf), branch)
        if branch != "sum":
            continue                                        # same x: the flags are the contract, the coordinates are not specified
        for c, (name, dom) in enumerate(output_contract(form, field)):
            got = out.coords[c]
            scale = JAC_SCALE[c] if form in ("add_lazy", "madd_lazy") else 1
            want = ref[1 + c]
            e = elem(field, got)
            e = F_scale(field, e, scale)
            assert e == want, "%s: coordinate %s has the wrong residue" % (tag, name)
            for k, l in enumerate(got):
                assert DOM[dom].contains(l), "%s: coordinate %s component %d leaves its contract %s: %s" % (tag, name, k, dom, l)
    return branch


def F_scale(field, e, s):
    return e * s % P if field == 1 else tuple(x * s % P for x in e)


# ---- on-curve cases ------------------------------------------------------------------------------------------------------
def lazy_rep(v, dom, rng):
    """a normal form of the residue v (already a Montgomery image) inside dom"""
    d = DOM[dom]
    ks = [k for k in range(d.lo // P - 1, d.hi // P + 2) if d.lo < v + k * P < d.hi]
    return normal_form(v + rng.choice(ks) * P)


def mont_image(field, e, doms, rng):
    comps = (e,) if field == 1 else e
    return [lazy_rep(c * R261 % P, doms, rng) for c in comps]


def rand_elem(field, rng):
    return rng.randrange(1, P) if field == 1 else (rng.randrange(1, P), rng.randrange(P))


def xyzz_image(field, pt, rng, trivial=False):
    """XYZZ image of an affine point with a random ZZ = z^2, ZZZ = z^3 inside the accumulator's contract"""
    F = K[field]
    z = F.small(1) if trivial else rand_elem(field, rng)
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    if pt is None:
        pt = (rand_elem(field, rng), rand_elem(field, rng))     # infinity: the coordinates are to be ignored
    return {0: mont_image(field, F.mul(pt[0], zz), "X", rng), 1: mont_image(field, F.mul(pt[1], zzz), ydom(field), rng),
            2: mont_image(field, zz, "M", rng), 3: mont_image(field, zzz, "M", rng)}


def jac_image(field, pt, rng, doms=("JX", "JY", "JZ")):
    F = K[field]
    z = rand_elem(field, rng)
    zz = F.mul(z, z)
    if pt is None:
        pt = (rand_elem(field, rng), rand_elem(field, rng))
    return {0: mont_image(field, F.mul(pt[0], zz), doms[0], rng), 1: mont_image(field, F.mul(pt[1], F.mul(zz, z)), doms[1], rng), 2: mont_image(field, z, doms[2], rng)}


def table_point(field, pt, negate):
    """(qx, qy) as the accumulation loads them: canonical, qy negated limb-wise for a negative digit; stands for +-pt"""
    comps = lambda e: (e,) if field == 1 else e          # noqa: E731
    qx = [normal_form(c * R261 % P) for c in comps(pt[0])]
    qy = [normal_form(c * R261 % P) for c in comps(pt[1])]
    return {4: qx, 5: [neg(l) for l in qy] if negate else qy}


def shift(ops, by=4):
    return {s + by: v for s, v in ops.items()}


def to_affine(field, form, out):
    F = K[field]
    if out.inf:
        return None
    e = [elem(field, c) for c in out.coords]
    if is_jac(form):
        zi = F.inv(e[2])
        zi2 = F.mul(zi, zi)
        return F.mul(e[0], zi2), F.mul(e[1], F.mul(zi2, zi))
    return F.mul(e[0], F.inv(e[2])), F.mul(e[1], F.inv(e[3]))


SMALL_K = [0, 1, 2, 3, (1 << 15) - 1, 11, 1234, 20011]


@functools.lru_cache(maxsize=None)
def law_jobs(field):
    """group-law cases on the curve: jobs with the affine point (or None) or the status they must give"""
    rng = random.Random("law %d" % field)
    F = K[field]
    mul, add, ng, G = (pyref.g1_mul, pyref.g1_add, pyref.g1_neg, pyref.G1_GEN) if field == 1 else (pyref.g2_mul, pyref.g2_add, pyref.g2_neg, pyref.G2_GEN)
    pts = [mul(G, k) for k in (1, 2, 5, 77, 1 << 40 | 12345)]
    jobs = []

    def job(form, ops, want=None, flags=0, k=0, status=None, case=""):
        jobs.append(dict(form=form, field=field, ops=ops, flags=flags, k=k, want=want, want_status=status, case=case))

    pairs = [(pts[1], pts[3]), (pts[4], pts[0]), (pts[2], pts[4])]
    for form in ["add_xyzz", "add_xyzz_from", "quad_add_xyzz"] + (["add_xyzz_from_parked"] if field == 2 else []) + ["add_lazy"]:
        img = (lambda p: jac_image(field, p, rng)) if form == "add_lazy" else (lambda p: xyzz_image(field, p, rng))
        for a, b in pairs:
            cases = [("P + Q", a, b, 0), ("P + P", a, a, 0), ("P + (-P)", a, ng(a), 0), ("inf + Q", None, b, 1), ("P + inf", a, None, 2), ("inf + inf", None, None, 3)]
            for case, x, y, flags in cases:
                ops = dict(img(x))
                ops.update(shift(img(y)))
                job(form, ops, want=("pt", add(x, y)), flags=flags, case=case)
    for form in ("madd_xyzz", "madd_xyzz_nz", "madd_lazy", "madd_xyzz_second"):
        for a, b in pairs:
            for case, q, sign in (("P + Q", b, 0), ("P - Q", b, 1), ("P + P", a, 0), ("P + (-P)", a, 1)):
                if form == "madd_xyzz_second":
                    acc = table_point(field, a, False)
                    ops = {0: acc[4], 1: acc[5]}            # the run's first point, ZZ = ZZZ = 1 implied
                elif form == "madd_lazy":
                    ops = dict(jac_image(field, a, rng, ("X", "Y2", "M")))
                else:
                    ops = dict(xyzz_image(field, a, rng))
                ops.update(table_point(field, q, sign))
                sq = ng(q) if sign else q
                if case == "P + P":
                    want, status = None, (0 if form in ("madd_xyzz", "madd_lazy") else 1)        # the caller doubles
                elif case == "P + (-P)":
                    want, status = (("pt", None), 1) if form in ("madd_xyzz", "madd_lazy") else (None, 2)
                else:
                    want, status = ("pt", add(a, sq)), (1 if form in ("madd_xyzz", "madd_lazy") else 0)
                job(form, ops, want=want, status=status, case=case)
            if form in ("madd_xyzz", "madd_lazy"):
                ops = dict(xyzz_image(field, None, rng) if form == "madd_xyzz" else jac_image(field, None, rng, ("X", "Y2", "M")))
                ops.update(table_point(field, b, 1))
                job(form, ops, want=("pt", ng(b)), flags=1, status=1, case="inf + (-Q)")
    a = pts[3]
    ops = dict(xyzz_image(field, a, rng, trivial=True))
    ops.update(table_point(field, pts[1], 0))
    job("madd_xyzz_nz", ops, want=("pt", add(a, pts[1])), status=0, case="accumulator with ZZ = ZZZ = 1")
    for form in ("dbl_xyzz", "quad_dbl_xyzz", "dbl_lazy"):
        for a in pts[:3]:
            job(form, dict(jac_image(field, a, rng) if form == "dbl_lazy" else xyzz_image(field, a, rng)), want=("pt", add(a, a)), case="2 P")
        job(form, dict(jac_image(field, None, rng) if form == "dbl_lazy" else xyzz_image(field, None, rng)), want=("pt", None), flags=1, case="2 inf")
    for form in ("mul_small_lazy", "quad_mul_small_xyzz"):
        for i, k in enumerate(SMALL_K):
            a = pts[i % len(pts)]
            # mul_small_lazy weighs canonical loads (jacr_load(acc_store(..))): its chain of doublings starts inside (JX, JY, JZ)
            ops = dict(jac_image(field, a, rng, ("T", "T", "T")) if form == "mul_small_lazy" else xyzz_image(field, a, rng))
            job(form, ops, want=("pt", mul(a, k) if k else None), k=k, case="%d P" % k)
        job(form, dict(jac_image(field, None, rng) if form == "mul_small_lazy" else xyzz_image(field, None, rng)), want=("pt", None), flags=1, k=5, case="5 inf")
    return jobs


def check_law_job(job, res, where):
    form, field = job["form"], job["field"]
    lanes = range(4) if form in QUAD_FORMS else (0,)
    for lane in lanes:
        out = Out(res[lane], field)
        tag = "%s G%d %s (%s) lane %d" % (form, field, where, job["case"], lane)
        assert out.status != NOT_RUN, tag
        if job["want_status"] is not None:
            assert out.status == job["want_status"], tag + ": status %d" % out.status
        if job["want"] is not None:
            assert to_affine(field, form, out) == job["want"][1], tag + ": not the sum as an affine point"
            if not out.inf and not is_jac(form):
                for c, (name, dom) in enumerate(output_contract(form, field)):
                    assert all(DOM[dom].contains(l) for l in out.coords[c]), tag + ": coordinate %s leaves its contract" % name
            if not out.inf and is_jac(form):
                assert all(DOM["J16"].contains(l) for c in out.coords[:3] for l in c), tag + ": leaves |value| < 16 p"


# ---- the asm bodies ------------------------------------------------------------------------------------------------------
def asm_expect(odd, X, Y, ZZ, ZZZ, qx, qy):
    """what a body must leave, by the limb-exact model of madd_xyzz_nz (gen_madd_asm.ref_madd over gen_mont_asm.model) on the value the
    Y register stands for, and by the big-int formula"""
    Y = neg(Y) if odd else Y                       # the value the register stands for
    X3, Y3, ZZ3, ZZZ3, PP, RR = GM.ref_madd(X, Y, ZZ, ZZZ, qx, qy, FQ)
    same_x = value(PP) % P == 0
    e = [elem(1, [c]) for c in (X, Y, ZZ, ZZZ, qx, qy)]
    ref = ref_madd(K[1], *e)
    assert (ref[0] != "sum") == same_x
    if ref[0] == "sum":
        assert [elem(1, [c]) for c in (X3, Y3, ZZ3, ZZZ3)] == list(ref[1:]), "the limb model and the formula disagree"
    return dict(X=X3, Y3=value(Y3) % P, ZZ=ZZ3, ZZZ=ZZZ3, same_x=same_x, same_point=same_x and value(RR) % P == 0, PP=PP, RR=RR)


def check_asm_lane(odd, got, exp, tag):
    """got: X, Y, ZZ, ZZZ limb vectors after a body that formed a sum"""
    for n in ("X", "ZZ", "ZZZ"):
        assert got[n] == exp[n], "%s: %s differs from madd_xyzz_nz's limbs" % (tag, n)
    sign = 1 if odd else -1
    assert (sign * value(got["Y"]) - exp["Y3"]) % P == 0, "%s: the Y register is not %sY3" % (tag, "+" if odd else "-")
    assert DOM["YR"].contains(got["Y"]), "%s: the Y register leaves (-p/4, 3 p): %s" % (tag, got["Y"])
    assert DOM["X"].contains(got["X"]) and DOM["M"].contains(got["ZZ"]) and DOM["M"].contains(got["ZZZ"]), tag + ": an output leaves its contract"


def simulate_body(odd, lane):
    rng = random.Random(7)
    rin = {}
    for n, key in (("XA", "X"), ("Y", "Y"), ("ZZ", "ZZ"), ("ZZZ", "ZZZ"), ("QX", "qx"), ("QY", "qy")):
        for i in range(9):
            rin["%s%d" % (n, i)] = lane[key][i]
    for n in ("XB", "PP", "M"):
        for i in range(9):
            rin["%s%d" % (n, i)] = rng.getrandbits(32)
    out, masks = GM.simulate(BODIES[odd], rin, **FQ)          # asserts every 64-bit column
    return {k: [GM.s32(out["%s%d" % (n, i)]) for i in range(9)] for k, n in (("X", "XB"), ("Y", "Y"), ("ZZ", "ZZ"), ("ZZZ", "ZZZ"))}, masks


BODIES = {False: GM.gen_madd_g1(False), True: GM.gen_madd_g1(True)}


def solve_product(target, other):
    """a canonical a with mont(a, other) == target exactly (target: a normal form of a value in (p/128, p))"""
    a = normal_form(value(target) * R261 * pow(value(other), -1, P) % P)
    return a if model([(a, other)], **FQ) == target else None


@functools.lru_cache(maxsize=None)
def derived_lanes():
    """Corners of the INTERMEDIATES that meet an operand limb by limb: U2 = qx ZZ against X (P = U2 - X) and S2 = qy ZZZ against the Y
    register (R = S2 -+ Y; the odd body ADDS two normal forms).  qx / qy are solved so that the product lands on the corner."""
    rng = random.Random("derived")
    lanes = []
    tops = (0x100000, 0x300000)
    lows = ([M29] * 8, [0] * 8, [M29 if i % 2 else 0 for i in range(8)], [0 if i % 2 else M29 for i in range(8)])
    for low in lows:
        for top in tops:
            target = low + [top]
            for acc_corner in DOM["YR"].extremes()[:6] + DOM["YR"].extremes()[6::3]:
                zz, zzz = DOM["M"].random(rng), DOM["M"].random(rng)
                qx, qy = solve_product(target, zz), solve_product(target, zzz)
                if qx is None or qy is None or not value(zz) % P or not value(zzz) % P:
                    continue
                xc = DOM["X"].extremes()[len(lanes) % 12]
                lanes.append(dict(X=xc, Y=acc_corner, ZZ=zz, ZZZ=zzz, qx=qx, qy=qy))
    return lanes


def find_filter_lane(rng, which, same_x, odd):
    """operands whose PP (which = 'PP') or R^2 ('RR') has limb 0 equal to 0 or to p's limb 0 without being 0 mod p: the two-compare
    filter of the body passes, the exact comparison must not.  same_x: additionally P == 0 mod p (then R^2 decides same_point).
    The square's value w is chosen first; P (or R) is a root of w 2^261, and X (or the Y register) is what makes it so."""
    p0 = FQ["P29"][0]
    while True:
        w = (rng.randrange(P >> 30) << 29) + (p0 if rng.random() < 0.5 else 0)
        if not P // 64 < w < P:
            continue
        s2 = w * R261 % P
        if pow(s2, (P - 1) // 2, P) != 1:
            continue
        root = pow(s2, (P + 1) // 4, P) * rng.choice((1, -1)) + rng.choice((-1, 0, 1)) * P          # p = 3 mod 4
        ZZ, ZZZ, qx, qy = DOM["M"].random(rng), DOM["M"].random(rng), DOM["T"].random(rng), DOM["TS"].random(rng)
        U2, S2 = model([(qx, ZZ)], **FQ), model([(qy, ZZZ)], **FQ)
        if which == "PP":
            X, Y = normal_form(value(U2) - root), DOM["YR"].random(rng)
        else:
            X = normal_form(value(U2) - (P if same_x else rng.randrange(1, P)))
            Y = normal_form(root - value(S2) if odd else value(S2) - root)       # R = S2 + N (odd) or S2 - Y (even)
        if not (DOM["X"].contains(X) and DOM["YR"].contains(Y)):
            continue
        lane = dict(X=X, Y=Y, ZZ=ZZ, ZZZ=ZZZ, qx=qx, qy=qy)
        exp = asm_expect(odd, **lane)
        sq = exp[which]
        if sq[0] in (0, p0) and value(sq) % P and exp["same_x"] == same_x:
            return lane


def curve_lane(rng, kind, odd):
    """accumulator = an image of a curve point a (the Y register holds -Y for the odd body); the table point is another point
    ('ord'), a ('same') or -a ('opp')"""
    F = K[1]
    a, b = pyref.g1_mul(pyref.G1_GEN, rng.randrange(2, 1 << 60)), pyref.g1_mul(pyref.G1_GEN, rng.randrange(2, 1 << 60))
    z = rand_elem(1, rng)
    zz, zzz = F.mul(z, z), F.mul(F.mul(z, z), z)
    y = F.mul(a[1], zzz)
    pt = table_point(1, a if kind != "ord" else b, kind == "opp")
    return dict(X=mont_image(1, F.mul(a[0], zz), "X", rng)[0], Y=mont_image(1, F.neg(y) if odd else y, "YR", rng)[0], ZZ=mont_image(1, zz, "M", rng)[0],
                ZZZ=mont_image(1, zzz, "M", rng)[0], qx=pt[4][0], qy=pt[5][0])


@functools.lru_cache(maxsize=None)
def wave_cases():
    """64-lane launches with different work per lane: kinds 'ord', 'same', 'opp', 'PP' / 'RR' (limb-0 filter hits that are no zeros: RR
    lanes have the same x), 'off' (lanes that sit the body out).  mode 0 / 1 / 2 = even / odd / even then odd on the same registers."""
    rng = random.Random("waves")
    pats = asm_pattern_lanes()
    filt = {(kind, odd): [find_filter_lane(rng, kind[:2], kind == "RR", odd) for _ in range(n)]
            for kind, n in (("PP", 6), ("RR", 6), ("RRx", 2)) for odd in (False, True)}
    layouts = [
        {0: "PP", 5: "PP", 33: "PP", 63: "PP", 7: "off", 40: "off"},                      # filter hits only: the exact comparison must clear every bit
        {0: "same", 1: "opp", 31: "PP", 32: "RR", 62: "RRx", 63: "same", 2: "off", 3: "off", 47: "off"},
        {13: "opp", 14: "RR", 15: "RR", 16: "PP", 48: "same", 49: "RRx", 50: "off"},
        {**{i: "off" for i in range(0, 64, 2)}, 1: "same", 3: "RR", 5: "PP", 61: "opp"},   # every second lane off
        dict({i: "off" for i in range(64) if i != 17}),                                    # a single live lane
        {},                                                                                # ordinary additions only
    ]
    cases = []
    for mode in (0, 1, 2):
        for li, layout in enumerate(layouts):
            lanes = []
            for i in range(64):
                kind = layout.get(i, "ord")
                odd = mode == 1
                if kind in ("same", "opp"):
                    l = curve_lane(rng, kind, odd)
                elif kind in ("PP", "RR", "RRx"):
                    l = filt[(kind, odd)][(i + li) % len(filt[(kind, odd)])]
                elif i % 3 == 0:
                    l = curve_lane(rng, "ord", odd)
                else:
                    l = pats[rng.randrange(len(pats))]           # the Y register at a corner, whichever sign it stands for
                l = dict(l, kind=kind, active=kind != "off", mode=mode)
                second = pats[rng.randrange(len(pats))] if i % 2 else curve_lane(rng, "ord", False)
                l["qx2"], l["qy2"] = second["qx"], second["qy"]
                lanes.append(l)
            cases.append(lanes)
    return cases


@functools.lru_cache(maxsize=None)
def asm_lanes():
    """every lane of the asm section, in order: (set name, lanes); each set is padded with switched-off lanes to whole waves"""
    def pad(lanes):
        lanes = list(lanes)
        while len(lanes) % 64:
            lanes.append(dict(lanes[0], active=False, kind="off"))
        return lanes
    sets = []
    for odd in (False, True):
        sets.append(("patterns odd" if odd else "patterns even", pad(dict(l, active=True, mode=int(odd), kind="pat") for l in asm_pattern_lanes())))
        sets.append(("derived odd" if odd else "derived even", pad(dict(l, active=True, mode=int(odd), kind="pat") for l in derived_lanes())))
    sets.append(("waves", [l for case in wave_cases() for l in case]))
    return sets


def check_asm_section(results):
    """results: one record per lane: (masks of the first body (same_x, same_point), first outputs, masks of the second, second outputs);
    returns (pattern lanes, pattern lanes with the same x, filter lanes seen) for the cap and the coverage assertions"""
    at, npat, nsame, nfilter = 0, 0, 0, 0
    for name, lanes in asm_lanes():
        for w0 in range(0, len(lanes), 64):
            wave = lanes[w0:w0 + 64]
            exps = [asm_expect(l["mode"] == 1, l["X"], l["Y"], l["ZZ"], l["ZZZ"], l["qx"], l["qy"]) if l["active"] else None for l in wave]
            want_x = sum(1 << i for i, e in enumerate(exps) if e and e["same_x"])
            want_p = sum(1 << i for i, e in enumerate(exps) if e and e["same_point"])
            for i, (l, e) in enumerate(zip(wave, exps)):
                tag = "asm %s body, %s, wave %d lane %d (%s)" % ("odd" if l["mode"] == 1 else "even", name, w0 // 64, i, l["kind"])
                r = results[at + w0 + i]
                if not l["active"]:
                    assert r is None or r["touched"] is False, tag + ": a switched-off lane wrote a result"
                    continue
                assert (r["same_x"], r["same_point"]) == (want_x, want_p), "%s: masks %016x / %016x, want %016x / %016x" % (tag, r["same_x"], r["same_point"], want_x, want_p)
                if l["kind"] == "pat":
                    npat += 1
                    nsame += e["same_x"]
                if l["kind"] in ("PP", "RR", "RRx"):
                    which = "PP" if l["kind"] == "PP" else "RR"
                    assert e[which][0] in (0, FQ["P29"][0]) and value(e[which]) % P, tag + ": not a filter hit"
                    nfilter += 1
                if e["same_x"]:
                    continue                                # documented garbage
                check_asm_lane(l["mode"] == 1, r["out1"], e, tag)
                if l["mode"] == 2:
                    s = r["out1"]
                    e2 = asm_expect(True, s["X"], s["Y"], s["ZZ"], s["ZZZ"], l["qx2"], l["qy2"])
                    assert not e2["same_x"]
                    assert (r["same_x2"] >> i) & 1 == 0 and (r["same_point2"] >> i) & 1 == 0, tag + ": second body's masks"
                    check_asm_lane(True, r["out2"], e2, tag + " second body")
        at += len(lanes)
    return npat, nsame, nfilter


# ---- chains ------------------------------------------------------------------------------------------------------------------
CHAIN_LANES, CHAIN_STEPS, FOLD_STEPS, CHAIN_T = 8, 256, 64, 24          # 256 = RUN_MAX additions


def chain_index(lane, step, T):
    return (lane * 5 + step * (2 * lane + 1)) % T


@functools.lru_cache(maxsize=None)
def chain_inputs():
    rng = random.Random("chains")
    nz = {d: [l for l in DOM[d].everything() if value(l) % P] for d in DOM}      # a zero coordinate pins a chain to a degenerate orbit; the pattern jobs have them
    pick = lambda d, i: nz[d][(i * 7 + 3) % len(nz[d])] if i % 3 else DOM[d].random(rng)   # noqa: E731
    corner = lambda d, i: [l for l in DOM[d].corners() if value(l) % P][i]         # noqa: E731
    g1 = dict(table=[(pick("T", i), pick("TS", i + 1)) for i in range(CHAIN_T)],
              start=[(corner("X", i), corner("YR", i + 1), corner("M", i + 2), corner("M", i + 5)) for i in range(CHAIN_LANES)])
    g2 = dict(table=[([pick("T", 2 * i), pick("T", 2 * i + 1)], [pick("TS", i), pick("TS", i + 2)]) for i in range(CHAIN_T)],
              start=[([corner("X", i), corner("X", i + 3)], [corner("Y2", i + 1), corner("Y2", i + 4)],
                      [corner("M", i + 2), corner("M", i + 6)], [corner("M", i + 5), corner("M", i + 7)]) for i in range(CHAIN_LANES)])
    img = lambda i: tuple([pick(d, i + c), pick(d, 2 * i + c + 1)] for c, d in enumerate(("X", "Y2", "M", "M")))          # noqa: E731
    fold = dict(table=[(img(i), i == 5) for i in range(CHAIN_T)], start=[(img(40 + i), i == 6) for i in range(CHAIN_LANES)])
    return g1, g2, fold


# ---- request / result files -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def job_sets():
    """every job of the module, in order: (set name, jobs).  G1 first, then G2."""
    out = {1: [], 2: []}
    for field in (1, 2):
        for form in PATTERN_FORMS[field]:
            out[field].append(("pattern %s" % form, pattern_jobs(form, field)))
        out[field].append(("law", law_jobs(field)))
    # madd_xyzz_nz on the operands of the asm bodies' pattern lanes: the bodies promise its limbs in X3, ZZ3, ZZZ3
    for odd in (False, True):
        jobs = []
        for name, lanes in asm_lanes():
            if name in ("patterns odd" if odd else "patterns even", "derived odd" if odd else "derived even"):
                for l in lanes:
                    if l["active"]:
                        y = normal_form(-value(l["Y"])) if odd else l["Y"]       # the value the register stands for, as a normal form
                        jobs.append(dict(form="madd_xyzz_nz", field=1, flags=0, k=0, ops={0: [l["X"]], 1: [y], 2: [l["ZZ"]], 3: [l["ZZZ"]], 4: [l["qx"]], 5: [l["qy"]]}))
        out[1].append(("nz twin of the %s body" % ("odd" if odd else "even"), jobs))
    return out


def encode_jobs(jobs):
    a = np.zeros((len(jobs), JOB_IN), np.int64)
    for i, j in enumerate(jobs):
        a[i, 0:3] = (FORM_CODE[j["form"]], j["flags"], j["k"])
        for slot, comps in j["ops"].items():
            for k, l in enumerate(comps):
                a[i, 4 + 18 * slot + 9 * k:13 + 18 * slot + 9 * k] = l
    assert np.all(np.abs(a) < (1 << 31))
    return a.astype(np.int32).reshape(-1)


def flat(*vecs):
    out = []
    for v in vecs:
        out += v
    return out


def write_request(path, with_device_sections=True):
    sets = job_sets()
    j1 = [j for _, js in sets[1] for j in js]
    j2 = [j for _, js in sets[2] for j in js]
    parts = [encode_jobs(j1), encode_jobs(j2)]
    head = [MAGIC, len(j1), len(j2)] + [0] * 10
    if with_device_sections:
        lanes = [l for _, ls in asm_lanes() for l in ls]
        rows = [[int(l["active"]), l["mode"]] + flat(l["X"], l["Y"], l["ZZ"], l["ZZZ"], l["qx"], l["qy"], l.get("qx2", l["qx"]), l.get("qy2", l["qy"])) for l in lanes]
        parts.append(np.array(rows, np.int64).astype(np.int32).reshape(-1))
        g1, g2, fold = chain_inputs()
        words = lambda rows: np.array(flat(*rows), np.int64).astype(np.int32)          # noqa: E731
        parts.append(words([flat(*t) for t in g1["table"]] + [flat(*s) for s in g1["start"]]))
        parts.append(words([flat(*(c for co in t for c in co)) for t in g2["table"]] + [flat(*(c for co in s for c in co)) for s in g2["start"]]))
        frow = lambda e: flat(*(c for co in e[0] for c in co)) + [int(e[1])]          # noqa: E731
        parts.append(words([frow(e) for e in fold["table"]] + [frow(e) for e in fold["start"]]))
        head[3:] = [len(lanes), CHAIN_LANES, CHAIN_T, CHAIN_STEPS, CHAIN_LANES, CHAIN_T, CHAIN_STEPS, CHAIN_LANES, CHAIN_T, FOLD_STEPS]
    np.concatenate([np.array(head, np.int32)] + parts).astype("<i4").tofile(path)
    return len(j1), len(j2)


class Results:
    def __init__(self, path, device):
        raw = np.fromfile(path, "<i4")
        sets = job_sets()
        n1, n2 = (sum(len(js) for _, js in sets[f]) for f in (1, 2))
        at = (n1 + n2) * 4 * JOB_OUT
        self.jobs = {1: raw[:n1 * 4 * JOB_OUT].reshape(n1, 4, JOB_OUT), 2: raw[n1 * 4 * JOB_OUT:at].reshape(n2, 4, JOB_OUT)}
        if not device:
            assert len(raw) == at
            return
        nl = sum(len(ls) for _, ls in asm_lanes())
        self.asm = raw[at:at + nl * ASM_OUT].reshape(nl, ASM_OUT)
        at += nl * ASM_OUT
        n = CHAIN_LANES * CHAIN_STEPS
        self.chain_g1 = raw[at:at + n * 38].reshape(CHAIN_LANES, CHAIN_STEPS, 38)
        at += n * 38
        self.chain_g2 = raw[at:at + n * 73].reshape(CHAIN_LANES, CHAIN_STEPS, 73)
        at += n * 73
        self.fold = raw[at:at + CHAIN_LANES * FOLD_STEPS * 73].reshape(CHAIN_LANES, FOLD_STEPS, 73)
        at += CHAIN_LANES * FOLD_STEPS * 73
        assert at == len(raw), "result file has %d words, expected %d" % (len(raw), at)

    def of(self, field, set_name):
        """(jobs, result records) of one job set"""
        at = 0
        for name, js in job_sets()[field]:
            if name == set_name:
                return js, self.jobs[field][at:at + len(js)]
            at += len(js)
        raise KeyError(set_name)

    def asm_records(self):
        u64 = lambda lo, hi: (int(lo) & 0xffffffff) | (int(hi) & 0xffffffff) << 32      # noqa: E731
        vec = lambda r, o: {n: [int(x) for x in r[o + 9 * k:o + 9 * k + 9]] for k, n in enumerate(("X", "Y", "ZZ", "ZZZ"))}   # noqa: E731
        return [dict(touched=bool(np.any(r)), same_x=u64(r[0], r[1]), same_point=u64(r[2], r[3]), same_x2=u64(r[4], r[5]), same_point2=u64(r[6], r[7]),
                     out1=vec(r, 8), out2=vec(r, 44)) for r in self.asm]


def library_flags():
    """CXXFLAGS of csrc/Makefile, read (not copied) so that the harness is compiled exactly as the library is"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda n: re.search(r"^%s \?= (.*)$" % n, text, re.M).group(1).strip()       # noqa: E731
    return var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


@pytest.fixture(scope="module")
def harness():
    """point_forms_check, built once per state of its sources (kept under tests/cpp/_build, which git ignores)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build tests/cpp/point_forms_check.hip"
    flags = library_flags()
    h = hashlib.sha256(" ".join(flags).encode())
    for f in [HARNESS] + sorted(os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith((".cuh", ".hpp", ".inc"))):
        h.update(open(f, "rb").read())
    out_dir = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "point_forms_check_" + h.hexdigest()[:16])
    if not os.path.exists(exe):
        t0 = time.time()
        tmp = exe + ".tmp%d" % os.getpid()
        subprocess.run([hipcc] + flags + ["-I", CSRC, HARNESS, "-o", tmp], check=True, capture_output=True, text=True, timeout=1800)
        os.replace(tmp, exe)
        print("point_forms_check built in %.0f s" % (time.time() - t0))
    return exe


def run_harness(exe, args, seconds):
    """a fresh child process under a time limit; any failure is the fixture's failure and nothing is launched again"""
    res = subprocess.run(["timeout", "-k", "10", str(seconds), exe] + args, capture_output=True, text=True)
    assert res.returncode == 0, "point_forms_check exited with %d\n%s%s" % (res.returncode, res.stdout, res.stderr)


@pytest.fixture(scope="module")
def host_results(harness, tmp_path_factory):
    d = tmp_path_factory.mktemp("point_forms_host")
    write_request(str(d / "request.bin"), with_device_sections=False)
    run_harness(harness, ["--host", str(d / "request.bin"), str(d / "result.bin")], 300)
    return Results(str(d / "result.bin"), device=False)


@pytest.fixture(scope="module")
def device_results(harness, tmp_path_factory):
    """ALL jobs of the module in one run of the harness on the GPU"""
    d = tmp_path_factory.mktemp("point_forms_device")
    write_request(str(d / "request.bin"))
    t0 = time.time()
    run_harness(harness, [str(d / "request.bin"), str(d / "result.bin")], 120)
    print("point_forms_check ran in %.1f s" % (time.time() - t0))
    return Results(str(d / "result.bin"), device=True)


# ---- the CPU twin ----------------------------------------------------------------------------------------------------------
def test_every_pattern_is_inside_its_contract_and_every_corner_pair_is_covered():
    for d in DOM.values():
        assert len(d.corners()) == NCORNER and all(d.contains(l) for l in d.everything()), d.name
        if not d.signed:
            lows = {tuple(l[:8]) for l in d.extremes()}
            assert len(lows) == 4 and len(d.extremes()) == 12
            for low in lows:
                tops = [l[8] for l in d.extremes() if tuple(l[:8]) == low]
                lv = value(list(low) + [0])
                assert d.lo < lv + (min(tops) << 232) and lv + ((min(tops) - 1) << 232) <= d.lo        # the top limb sits AT both ends
                assert lv + (max(tops) << 232) < d.hi and lv + ((max(tops) + 1) << 232) >= d.hi
    assert any(all(x <= 0 for x in l) and any(l) for l in DOM["TS"].corners()) and any(all(x >= 0 for x in l) and any(l) for l in DOM["TS"].corners())
    designs = [("asm", [d for _, d in ASM_INPUTS], [[l[n] for n, _ in ASM_INPUTS] for l in asm_pattern_lanes()])]
    for field in (1, 2):
        for form in PATTERN_FORMS[field]:
            ins = form_inputs(SHARES_OPERANDS.get(form, form), field)
            coords = [(s, k, d) for s, d in ins for k in range(field)]
            jobs = pattern_jobs(form, field)
            assert len(jobs) >= 300
            designs.append(("%s G%d" % (form, field), [d for _, _, d in coords], [[j["ops"][s][k] for s, k, _ in coords] for j in jobs]))
    for name, doms, rows in designs:
        idx = []
        for c, d in enumerate(doms):
            corner = {tuple(l): i for i, l in reversed(list(enumerate(DOM[d].corners())))}
            assert all(DOM[d].contains(r[c]) for r in rows), "%s coordinate %d" % (name, c)
            idx.append([corner.get(tuple(r[c])) for r in rows[:NCORNER * NCORNER]])
            assert set(idx[-1]) >= set(corner.values()), "%s: coordinate %d misses a corner" % (name, c)
        for c1 in range(len(doms)):
            for c2 in range(c1 + 1, len(doms)):
                n1, n2 = len(set(idx[c1])), len(set(idx[c2]))
                assert len(set(zip(idx[c1], idx[c2]))) == n1 * n2, "%s: coordinates %d and %d do not meet in every pair of corners" % (name, c1, c2)
    assert len(derived_lanes()) >= 48
    for lanes in wave_cases():
        assert len(lanes) == 64
    for field in (1, 2):
        for j in law_jobs(field):
            for slot, d in (form_inputs(j["form"], field) if j["form"] in FORM_INPUT_FORMS else []):
                if slot in j["ops"] and not (j["flags"] & (1 if slot < 4 else 2)):
                    assert all(DOM[d].contains(l) for l in j["ops"][slot]), (j["form"], j["case"], slot)


FORM_INPUT_FORMS = {"madd_xyzz", "madd_xyzz_nz", "madd_xyzz_second", "add_xyzz", "dbl_xyzz", "dbl_lazy", "add_lazy", "madd_lazy"}


def test_same_x_share_of_the_pattern_jobs_stays_below_the_cap():
    """pattern jobs whose operands happen to have the same x are compared with the branch only; were they many, the formula comparison
    would be hollow"""
    for field in (1, 2):
        for form in PATTERN_FORMS[field]:
            if form in SHARES_OPERANDS:
                continue
            jobs = pattern_jobs(form, field)
            n = sum(reference(j)[0] != "sum" for j in jobs)
            print("%s G%d: %d of %d pattern jobs in the same-x branch" % (form, field, n, len(jobs)))
            assert n <= SAME_X_CAP * len(jobs), (form, field, n)


def test_asm_bodies_on_the_simulator_at_every_coordinate_corner():
    """gen_madd_asm.simulate (wrap-around semantics, every 64-bit column asserted) on the pattern, derived and wave lanes of both bodies,
    against the limb-exact model of madd_xyzz_nz and the big-int formula"""
    npat = nsame = nfilter = 0
    for name, lanes in asm_lanes():
        for i, l in enumerate(lanes):
            if not l["active"]:
                continue
            odd = l["mode"] == 1
            tag = "simulated %s body, %s, lane %d (%s)" % ("odd" if odd else "even", name, i, l["kind"])
            e = asm_expect(odd, l["X"], l["Y"], l["ZZ"], l["ZZZ"], l["qx"], l["qy"])
            try:
                got, masks = simulate_body(odd, l)
            except AssertionError as err:
                raise AssertionError("%s: %s" % (tag, err))
            assert (masks["z"], masks["z2"]) == (e["same_x"], e["same_point"]), tag + ": masks"
            if l["kind"] == "pat":
                npat += 1
                nsame += e["same_x"]
            nfilter += l["kind"] in ("PP", "RR", "RRx")
            if e["same_x"]:
                continue
            check_asm_lane(odd, got, e, tag)
            if l["mode"] == 2:
                l2 = dict(X=got["X"], Y=got["Y"], ZZ=got["ZZ"], ZZZ=got["ZZZ"], qx=l["qx2"], qy=l["qy2"])
                got2, masks2 = simulate_body(True, l2)
                assert not masks2["z"] and not masks2["z2"]
                check_asm_lane(True, got2, asm_expect(True, **l2), tag + " second body")
    print("asm bodies: %d pattern lanes, %d with the same x, %d filter lanes" % (npat, nsame, nfilter))
    assert npat >= 600 and nsame <= SAME_X_CAP * npat and nfilter >= 24


def _host_sets(field):
    return [(name, js) for name, js in job_sets()[field] if js and all(j["form"] in HOST_FORMS for j in js)]


@pytest.mark.parametrize("field", [1, 2])
def test_host_compiled_forms_match_the_published_formulas(host_results, field):
    """the one-lane forms are ZK_HD: the same C++ on the CPU.  A failure here is a formula or bound error; one that shows on the
    device only is code generation (asm multipliers, DPP, LDS)."""
    seen = 0
    for name, jobs in _host_sets(field):
        _, res = host_results.of(field, name)
        for i, (j, r) in enumerate(zip(jobs, res)):
            if name == "law":
                continue
            check_job(j, r, "%s job %d" % (name, i))
            seen += 1
    jobs, res = host_results.of(field, "law")
    for i, (j, r) in enumerate(zip(jobs, res)):
        if j["form"] in HOST_FORMS:
            check_law_job(j, r, "law job %d" % i)
    assert seen >= 7 * 300


# ---- on the device ------------------------------------------------------------------------------------------------------------
def _pattern_params():
    return [pytest.param(form, field, id="%s-G%d" % (form, field)) for field in (1, 2) for form in PATTERN_FORMS[field]]


@pytest.mark.gpu
@pytest.mark.parametrize("form,field", _pattern_params())
def test_gpu_form_at_the_limb_bounds(device_results, form, field):
    jobs, res = device_results.of(field, "pattern %s" % form)
    lanes = range(4) if form in QUAD_FORMS else (0,)
    same = 0
    for i, (j, r) in enumerate(zip(jobs, res)):
        same += check_job(j, r, "pattern job %d" % i, lanes) != "sum"
        if form in QUAD_FORMS:
            assert all(np.array_equal(r[0], r[k]) for k in range(1, 4)), "%s G%d job %d: the four lanes of the quad differ" % (form, field, i)
    assert same <= SAME_X_CAP * len(jobs)
    twin = SHARES_OPERANDS.get(form)
    if twin in ("add_xyzz",) and form != "quad_add_xyzz":
        # add_xyzz_from / add_xyzz_from_parked: "same formulas, same order, same bounds" -- the limbs of add_xyzz
        tj, tres = device_results.of(field, "pattern %s" % twin)
        for i, (j, r, t) in enumerate(zip(jobs, res, tres)):
            if reference(j)[0] == "sum":
                for c, name in enumerate(("X", "Y", "ZZ", "ZZZ")):
                    assert np.array_equal(r[0][4 + 18 * c:22 + 18 * c], t[0][4 + 18 * c:22 + 18 * c]), "%s G%d job %d: %s differs from add_xyzz's limbs" % (form, field, i, name)
                assert r[0][1] == t[0][1]


@pytest.mark.gpu
@pytest.mark.parametrize("field", [1, 2])
def test_gpu_group_law_on_the_curve(device_results, field):
    jobs, res = device_results.of(field, "law")
    assert len(jobs) >= 100
    for i, (j, r) in enumerate(zip(jobs, res)):
        check_law_job(j, r, "law job %d" % i)
        if j["form"] in QUAD_FORMS:
            assert all(np.array_equal(r[0], r[k]) for k in range(1, 4)), "%s (%s): the four lanes differ" % (j["form"], j["case"])


@pytest.mark.gpu
def test_gpu_asm_bodies_as_waves(device_results):
    """both bodies on the pattern and derived lanes, and the wave cases: masks bit by bit, limbs of every ordinary lane"""
    npat, nsame, nfilter = check_asm_section(device_results.asm_records())
    assert npat >= 600 and nsame <= SAME_X_CAP * npat and nfilter >= 24


@pytest.mark.gpu
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
def test_gpu_asm_bodies_have_the_limbs_of_madd_xyzz_nz(device_results, odd):
    """X3, ZZ3, ZZZ3 of a body against the C++ form run on the device with the same operands"""
    jobs, res = device_results.of(1, "nz twin of the %s body" % ("odd" if odd else "even"))
    recs = device_results.asm_records()
    at, k = 0, 0
    for name, lanes in asm_lanes():
        if name in ("patterns odd" if odd else "patterns even", "derived odd" if odd else "derived even"):
            for i, l in enumerate(lanes):
                if not l["active"]:
                    continue
                out, status = Out(res[k][0], 1), int(res[k][0][0])
                assert status == check_flag_of(jobs[k]), "madd_xyzz_nz twin %d: status" % k
                if status == 0:
                    for c, n in enumerate(("X", "ZZ", "ZZZ")):
                        assert recs[at + i]["out1"][n] == out.coords[(0, 2, 3)[c]][0], "%s lane %d: %s differs from madd_xyzz_nz on the device" % (name, i, n)
                k += 1
        at += len(lanes)
    assert k == len(jobs)
    for i, (j, r) in enumerate(zip(jobs, res)):
        check_job(j, r, "nz twin %d" % i)


def check_flag_of(job):
    return expected_flags(job["form"], reference(job)[0])[0]


@pytest.mark.gpu
def test_gpu_chain_of_256_additions_alternating_the_asm_bodies(device_results):
    g1, _, _ = chain_inputs()
    for lane in range(CHAIN_LANES):
        X, Y, ZZ, ZZZ = g1["start"][lane]
        for s in range(CHAIN_STEPS):
            qx, qy = g1["table"][chain_index(lane, s, CHAIN_T)]
            odd = bool(s & 1)
            tag = "G1 chain lane %d step %d (%s body)" % (lane, s, "odd" if odd else "even")
            e = asm_expect(odd, X, Y, ZZ, ZZZ, qx, qy)
            r = device_results.chain_g1[lane, s]
            got = {n: [int(x) for x in r[9 * k:9 * k + 9]] for k, n in enumerate(("X", "Y", "ZZ", "ZZZ"))}
            assert (int(r[36]), int(r[37])) == (int(e["same_x"]), int(e["same_point"])), tag + ": masks"
            assert not e["same_x"], tag + ": the chain ran into the same x"
            check_asm_lane(odd, got, e, tag)
            X, Y, ZZ, ZZZ = got["X"], got["Y"], got["ZZ"], got["ZZZ"]


def _g2_state(rec):
    return [[[int(x) for x in rec[18 * c + 9 * k:18 * c + 9 * k + 9]] for k in range(2)] for c in range(4)]


def _check_g2_step(ref, got, tag):
    assert ref[0] == "sum", tag + ": the chain ran into the same x"
    for c, (name, dom) in enumerate(output_contract("add_xyzz", 2)):
        assert elem(2, got[c]) == ref[1 + c], "%s: coordinate %s has the wrong residue" % (tag, name)
        assert all(DOM[dom].contains(l) for l in got[c]), "%s: coordinate %s leaves its contract %s" % (tag, name, dom)


@pytest.mark.gpu
def test_gpu_chain_of_256_additions_over_fq2(device_results):
    _, g2, _ = chain_inputs()
    F = K[2]
    for lane in range(CHAIN_LANES):
        st = [list(c) for c in g2["start"][lane]]
        for s in range(CHAIN_STEPS):
            qx, qy = g2["table"][chain_index(lane, s, CHAIN_T)]
            tag = "G2 chain (madd_xyzz_nz) lane %d step %d" % (lane, s)
            ref = ref_madd(F, *[elem(2, c) for c in st], elem(2, qx), elem(2, qy))
            rec = device_results.chain_g2[lane, s]
            assert int(rec[72]) == 0, tag + ": status %d" % int(rec[72])
            got = _g2_state(rec)
            _check_g2_step(ref, got, tag)
            st = got


@pytest.mark.gpu
def test_gpu_fold_of_64_parked_additions(device_results):
    _, _, fold = chain_inputs()
    F = K[2]
    for lane in range(CHAIN_LANES):
        st, inf = [list(c) for c in fold["start"][lane][0]], fold["start"][lane][1]
        for s in range(FOLD_STEPS):
            q, qinf = fold["table"][chain_index(lane, s, CHAIN_T)]
            tag = "fold (add_xyzz_from_parked) lane %d step %d" % (lane, s)
            rec = device_results.fold[lane, s]
            got = _g2_state(rec)
            if qinf:
                assert got == st and int(rec[72]) == int(inf), tag + ": adding infinity changed the sum"
            elif inf:
                assert got == [list(c) for c in q] and int(rec[72]) == 0, tag + ": infinity + q is not q"
                st, inf = got, False
            else:
                assert int(rec[72]) == 0, tag
                _check_g2_step(ref_add(F, *[elem(2, c) for c in st], *[elem(2, c) for c in q]), got, tag)
                st = got
