"""A Python model of zk_crs_check (include/zkgpu.h): the relations, restated with the oracle's group operations (oracle_lib:
msm_g1 / msm_g2 / g1_mul_batch), the host pairing zksnark_rs_amd.pairing, Gt products from oracle/pyref.py and Python integers for
every polynomial.  It shares no code with csrc/crs_check.hip: wire polynomials come from Lagrange sums (never an NTT or a tree), the
geometric sums S_d(z) are summed term by term (never the closed form), and every relation is two Gt values compared (never one
product against 1).  tests/test_crs_check_model.py ties it to the oracle's setup; tests/test_gpu_crs_check.py compares the device's
verdict bits with it for the same challenge."""
import os
import sys

import numpy as np

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib, ints_to_limbs, limbs_to_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402

R = zk.R_MODULUS
BIT = {name: 1 << k for k, name in enumerate(_lib.CRS_CHECK_BITS)}
T_ZERO, LAGRANGE_PRESENT = _lib.CRS_CHECK_T_ZERO, _lib.CRS_CHECK_LAGRANGE_PRESENT
INF1, INF2 = np.zeros(8, np.uint64), np.zeros(16, np.uint64)


# ---- the QAP as the model sees it ------------------------------------------------------------------------------------------------
def sparse_qap(roots, m, l, u, v, w):
    """rows by wire (ptr, gate, val limbs) over the integer list `roots` (gate j sits at roots[j])"""
    return dict(n=len(roots), m=m, l=l, roots=[int(r) % R for r in roots], rows=(u, v, w), t=poly_from_roots(roots))


def dense_qap(u, v, w, t, l):
    """(m, n, 4) coefficient limbs and t as (n + 1, 4) limbs"""
    to_ints = lambda a: [[limbs_to_int(c) for c in row] for row in np.asarray(a)]   # noqa: E731
    return dict(n=np.asarray(u).shape[1], m=np.asarray(u).shape[0], l=l, dense=(to_ints(u), to_ints(v), to_ints(w)),
                t=[limbs_to_int(c) for c in np.asarray(t).reshape(-1, 4)])


def poly_from_roots(roots):
    full = [1]
    for r in roots:
        nxt = [0] * (len(full) + 1)
        for i, c in enumerate(full):
            nxt[i + 1] = (nxt[i + 1] + c) % R
            nxt[i] = (nxt[i] - r * c) % R
        full = nxt
    return full


def interpolate(roots, values):
    """coefficients (len(roots) of them) of the polynomial through (roots[k], values[k]): plain Lagrange sums"""
    n = len(roots)
    out = [0] * n
    for k in range(n):
        if not values[k]:
            continue
        num, den = [1], 1
        for j in range(n):
            if j != k:
                num = [((num[i - 1] if i else 0) - roots[j] * (num[i] if i < len(num) else 0)) % R for i in range(len(num) + 1)]
                den = den * (roots[k] - roots[j]) % R
        f = values[k] * pow(den, -1, R) % R
        for i in range(n):
            out[i] = (out[i] + f * num[i]) % R
    return out


def wire_sums(q, rho, upto):
    """coefficients of sum_{i < upto} rho_i u_i, v_i, w_i"""
    n = q["n"]
    out = []
    for which in range(3):
        if "dense" in q:
            mat = q["dense"][which]
            out.append([sum(rho[i] * mat[i][k] for i in range(upto)) % R for k in range(n)])
        else:
            ptr, gate, val = q["rows"][which]
            vals = [0] * n
            for i in range(upto):
                for e in range(int(ptr[i]), int(ptr[i + 1])):
                    vals[int(gate[e])] = (vals[int(gate[e])] + rho[i] * limbs_to_int(val[e])) % R
            out.append(interpolate(q["roots"], vals))
    return out


# ---- group and pairing helpers ---------------------------------------------------------------------------------------------------
class Groups:
    def __init__(self, orc):
        self.orc = orc
        self._pairings = {}

    def msm1(self, pts, scalars):
        pts = np.asarray(pts, np.uint64).reshape(-1, 8)
        return self.orc.msm_g1(pts, ints_to_limbs(list(scalars))) if len(pts) else INF1.copy()

    def msm2(self, pts, scalars):
        pts = np.asarray(pts, np.uint64).reshape(-1, 16)
        return self.orc.msm_g2(pts, ints_to_limbs(list(scalars))) if len(pts) else INF2.copy()

    def mul1(self, p, k):
        return self.orc.g1_mul_batch(np.asarray(p).reshape(1, 8), ints_to_limbs([k % R]))[0]

    def mul2(self, p, k):
        return self.orc.g2_mul_batch(np.asarray(p).reshape(1, 16), ints_to_limbs([k % R]))[0]

    def add1(self, a, b):
        return self.orc.g1_add_batch(np.asarray(a).reshape(1, 8), np.asarray(b).reshape(1, 8))[0]

    def add2(self, a, b):
        return self.orc.g2_add_batch(np.asarray(a).reshape(1, 16), np.asarray(b).reshape(1, 16))[0]

    def e(self, p, q):
        """the pairing as an Fq12 tuple of pyref's; values are cached (a tampered CRS shares most of its pairings with the honest one)"""
        key = (np.asarray(p, np.uint64).tobytes(), np.asarray(q, np.uint64).tobytes())
        if key not in self._pairings:
            it = iter(zk.pairing(p, q))
            self._pairings[key] = tuple(tuple((next(it), next(it)) for _ in range(3)) for _ in range(2))
        return self._pairings[key]

    def prod(self, *pairs):
        f = pyref.FQ12_ONE
        for p, q in pairs:
            f = pyref.fq12_mul(f, self.e(p, q))
        return f


def is_inf(p):
    return not np.asarray(p).any()


# ---- the check -------------------------------------------------------------------------------------------------------------------
def check(grp, crs, q, s, lagrange=None):
    """(failed, flags) of zk_crs_check for the CRS arrays `crs` (Context.crs_arrays layout), the model QAP `q`, the challenge s and,
    when the CRS carries them, lagrange = dict(lag1=(n, 8), lagS_t1=(n - 1, 8), lag2=(n, 16))"""
    n, m, l = q["n"], q["m"], q["l"]
    assert crs["xi_g1"].shape[0] == n and crs["sum_gamma_g1"].shape[0] == l + 1 and crs["sum_delta_g1"].shape[0] == m - l - 1
    assert 1 <= s < R
    rho = [pow(s, k, R) for k in range(max(n, m))]
    xi1, xi2, xit = crs["xi_g1"], crs["xi_g2"], crs["xi_t_g1"]
    G, H = xi1[0], xi2[0]
    failed, flags = 0, (LAGRANGE_PRESENT if lagrange is not None else 0)
    if not (np.array_equal(G, grp.orc.enc_base_g1()) and np.array_equal(H, grp.orc.enc_base_g2())):
        failed |= BIT["GENERATORS"]
    if any(is_inf(crs[k]) for k in ("gamma_g2", "delta_g2", "delta_g1", "alpha_g1", "beta_g1", "beta_g2")):
        failed |= BIT["DEGENERATE"]
    if grp.e(crs["beta_g1"], H) != grp.e(G, crs["beta_g2"]) or grp.e(crs["delta_g1"], H) != grp.e(G, crs["delta_g2"]):
        failed |= BIT["TWINS"]
    all1, all2 = grp.msm1(xi1, rho[:n]), grp.msm2(xi2, rho[:n])
    if grp.e(all1, H) != grp.e(G, all2):
        failed |= BIT["POWERS_G2"]
    xt = grp.msm1(xit, rho[:n - 1])
    if n >= 2:
        if is_inf(xit[0]):
            flags |= T_ZERO
        P, Q = grp.msm1(xi1[:n - 1], rho[:n - 1]), grp.msm1(xi1[1:], rho[:n - 1])
        if grp.e(P, xi2[1]) != grp.e(Q, H):
            failed |= BIT["POWERS_G1"]
        t = q["t"]
        assert len(t) == n + 1
        t_prime = grp.msm2(xi2, t[1:])
        if grp.prod((xt, crs["delta_g2"])) != grp.prod((Q, t_prime), (grp.mul1(P, t[0]), H)):
            failed |= BIT["XI_T"]

    def wires(upto, sg, sd):
        uc, vc, wc = wire_sums(q, rho, upto)
        U, V, W = grp.msm1(xi1, uc), grp.msm2(xi2, vc), grp.msm1(xi1, wc)
        return grp.prod((sg, crs["gamma_g2"]), (sd, crs["delta_g2"])), (U, V, W)

    SG, SD = grp.msm1(crs["sum_gamma_g1"], rho[:l + 1]), grp.msm1(crs["sum_delta_g1"], rho[l + 1:m])
    rhs = lambda U, V, W: grp.prod((U, crs["beta_g2"]), (crs["alpha_g1"], V), (W, H))   # noqa: E731
    lhs, (U, V, W) = wires(m, SG, SD)
    if lhs != rhs(U, V, W):
        failed |= BIT["WIRES"]
        lhs_in, (Ui, Vi, Wi) = wires(l + 1, SG, INF1)
        if lhs_in != rhs(Ui, Vi, Wi):
            failed |= BIT["WIRES_GAMMA"]
        neg = R - 1
        Uo, Vo, Wo = grp.add1(U, grp.mul1(Ui, neg)), grp.add2(V, grp.mul2(Vi, neg)), grp.add1(W, grp.mul1(Wi, neg))
        if grp.prod((SD, crs["delta_g2"])) != rhs(Uo, Vo, Wo):
            failed |= BIT["WIRES_DELTA"]
    if lagrange is not None:
        S = lambda d, z: sum(pow(s * z % R, k, R) for k in range(d)) % R   # noqa: E731
        wn = [S(n, k + 1) for k in range(n)]
        ws = [S(n - 1, n + 1 + j) for j in range(n - 1)]
        if not (np.array_equal(grp.msm1(lagrange["lag1"], wn), all1) and np.array_equal(grp.msm2(lagrange["lag2"], wn), all2)
                and np.array_equal(grp.msm1(lagrange["lagS_t1"], ws), xt)):
            failed |= BIT["LAGRANGE"]
    return failed, flags


# ---- honest Lagrange-basis arrays from the trapdoor, and tampering -----------------------------------------------------------------
def lagrange_arrays(grp, n, trapdoor):
    """what zk_setup emits next to the powers for an integer-roots QAP: [L_k(x)]_1, [L_k(x)]_2 over 1..n and [L^S_j(x) t(x) / delta]_1
    over S = n+1..2n-1, from the trapdoor (alpha, beta, gamma, delta, x as ints)"""
    delta, x = trapdoor[3], trapdoor[4]
    def basis(nodes):
        out = []
        for k, rk in enumerate(nodes):
            num = den = 1
            for j, rj in enumerate(nodes):
                if j != k:
                    num, den = num * (x - rj) % R, den * (rk - rj) % R
            out.append(num * pow(den, -1, R) % R)
        return out
    tx = 1
    for k in range(1, n + 1):
        tx = tx * (x - k) % R
    L = basis(list(range(1, n + 1)))
    LS = [v * tx % R * pow(delta, -1, R) % R for v in basis(list(range(n + 1, 2 * n)))]
    g1, g2 = grp.orc.enc_base_g1(), grp.orc.enc_base_g2()
    mul1 = lambda ks: grp.orc.g1_mul_batch(np.tile(g1, (len(ks), 1)), ints_to_limbs(ks)) if ks else np.zeros((0, 8), np.uint64)   # noqa: E731
    return dict(lag1=mul1(L), lagS_t1=mul1(LS), lag2=grp.orc.g2_mul_batch(np.tile(g2, (n, 1)), ints_to_limbs(L)))


def other_point(grp, p):
    """another valid point in the place of p: 2 p (which stays in the G2 subgroup), or the base where p is infinity"""
    p = np.asarray(p)
    if p.size == 8:
        return grp.orc.enc_base_g1() if is_inf(p) else grp.add1(p, p)
    return grp.orc.enc_base_g2() if is_inf(p) else grp.add2(p, p)


def tampered(grp, arrs, key, pos=None):
    """a copy of the arrays with one point replaced (pos = None: `key` is a single point)"""
    out = {k: np.array(v, copy=True) for k, v in arrs.items()}
    if pos is None:
        out[key] = other_point(grp, out[key])
    else:
        out[key][pos] = other_point(grp, out[key][pos])
    return out


def positions(count):
    return sorted({0, count // 2, count - 1}) if count else []


SINGLE_POINTS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2")
WIRE_BITS = BIT["WIRES"] | BIT["WIRES_GAMMA"] | BIT["WIRES_DELTA"]


def expected_bits(key, pos, n, lagrange):
    """(required, allowed) bits of `failed` after one point of array `key` was replaced: the relation(s) the array has to itself are
    required; relations that merely READ the array (the wire relation forms U, V, W from the powers) may or may not notice"""
    lag = BIT["LAGRANGE"] if lagrange else 0
    if key == "xi_g1":
        if pos == 0:
            return BIT["GENERATORS"], BIT["GENERATORS"] | BIT["POWERS_G1"] | BIT["POWERS_G2"] | BIT["TWINS"] | BIT["XI_T"] | WIRE_BITS | lag
        return BIT["POWERS_G1"] | BIT["POWERS_G2"] | lag, BIT["POWERS_G1"] | BIT["POWERS_G2"] | BIT["XI_T"] | WIRE_BITS | lag
    if key == "xi_g2":
        if pos == 0:
            return BIT["GENERATORS"], BIT["GENERATORS"] | BIT["POWERS_G1"] | BIT["POWERS_G2"] | BIT["TWINS"] | BIT["XI_T"] | WIRE_BITS | lag
        return BIT["POWERS_G2"] | lag, BIT["POWERS_G1"] | BIT["POWERS_G2"] | BIT["XI_T"] | WIRE_BITS | lag
    if key == "xi_t_g1":
        return BIT["XI_T"] | lag, BIT["XI_T"] | lag
    if key == "sum_gamma_g1" or key == "gamma_g2":
        return BIT["WIRES"] | BIT["WIRES_GAMMA"], BIT["WIRES"] | BIT["WIRES_GAMMA"]
    if key == "sum_delta_g1":
        return BIT["WIRES"] | BIT["WIRES_DELTA"], BIT["WIRES"] | BIT["WIRES_DELTA"]
    if key == "alpha_g1":
        return BIT["WIRES"], WIRE_BITS
    if key in ("beta_g1", "delta_g1"):
        return BIT["TWINS"], BIT["TWINS"]
    if key == "beta_g2":
        return BIT["TWINS"], BIT["TWINS"] | WIRE_BITS
    if key == "delta_g2":
        return BIT["TWINS"], BIT["TWINS"] | (BIT["XI_T"] if n >= 2 else 0) | BIT["WIRES"] | BIT["WIRES_DELTA"]
    if key in ("lag1", "lag2", "lagS_t1"):
        return BIT["LAGRANGE"], BIT["LAGRANGE"]
    raise KeyError(key)
