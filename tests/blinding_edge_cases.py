"""Blinding scalars (r, s) that steer the closing additions of a proof into their special branches -- shared by
test_blinding_edges.py (host) and test_gpu_blinding_edges.py (device).  Python integers only.

A drawn (r, s) reaches an equal-operands, opposite-operands or infinity-operand branch of csrc/prove.hip's assembly with probability
2^-254.  The tests know the trapdoor (alpha, beta, gamma, delta, x), so every operand of those additions has a known discrete
logarithm to the base [1]_1 / [1]_2, and each branch is one linear equation mod R in r or s:

  k_assemble_pre   r_delta  = alpha + [r delta]                     (jac_madd_ni)
                   s_delta2 = beta2 + [s delta2]                    (jac_madd_ni over Fq2)
                   fixed_c  = ([s alpha] + [r beta]) + [r s delta]  (two jac_add_ni)
  k_assemble       a = A_msm + r_delta,   A_msm = [U]               (add_lazy)
                   b = B_msm + s_delta2,  B_msm = [V]_2             (add_lazy over Fq2)
                   c = (hb + l) + fixed_c                           (two jac_add_ni)
                       hb = [HT / delta + r V + s U], l = [L / delta] with option merge_lh = 0; with merge_lh = 1 hb holds their sum

with U = sum a_i u_i(x), V = sum a_i v_i(x), L = sum_{i > l} a_i (beta u_i + alpha v_i + w_i)(x) and HT = h(x) t(x), h the QUOTIENT of
U V - W by t with the remainder dropped (pyref.trapdoor_proof, groth16/mod.rs:277).  The proof's logarithms are

  a = alpha + U + r delta,  b = beta + V + s delta,  c = (L + HT) / delta + s (alpha + U) + r (beta + V) + r s delta.

cases() returns the named (r, s); for every case it asserts, in integers, the relation the case is named for, that every denominator it
divided by is non-zero, and which of a, b, c are zero (the elements encoded as infinity).  A case without a solution is an error."""
from collections import namedtuple

from zksnark_rs_amd import SplitMix64, limbs_to_int

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TWO_ADICITY = 28
OMEGA_2_28 = pow(5, (R - 1) >> TWO_ADICITY, R)

Scalars = namedtuple("Scalars", "U V L HT")
Case = namedtuple("Case", "name r s infinite")      # infinite: the subset of "abc" whose proof element is the point at infinity


def inv(a):
    assert a % R != 0, "a case divided by zero: pick another seed"
    return pow(a % R, -1, R)


def unity_roots(log_n):
    w = pow(OMEGA_2_28, 1 << (TWO_ADICITY - log_n), R)
    return [pow(w, j, R) for j in range(1 << log_n)]


# ---- U, V, L, HT from the trapdoor, the rows and the witness -----------------------------------------------------------------------
def lagrange_at(roots, x):
    """L_j(x) over distinct roots, by the product formula (n <= 64 here)"""
    out = []
    for j, rj in enumerate(roots):
        num = den = 1
        for k, rk in enumerate(roots):
            if k != j:
                num = num * (x - rk) % R
                den = den * (rj - rk) % R
        out.append(num * inv(den) % R)
    return out


def _rows(rows, m):
    ptr, gate, val = rows
    return [[(int(gate[e]), limbs_to_int(val[e])) for e in range(int(ptr[i]), int(ptr[i + 1]))] for i in range(m)]


def sparse_scalars(roots, m, l, u, v, w, trapdoor, weights):
    """rows (ptr, gate, val) by wire over `roots` (gate j sits at roots[j]); weights: (m, 4) limbs"""
    alpha, beta, gamma, delta, x = (int(e) % R for e in trapdoor)
    a = [limbs_to_int(e) for e in weights]
    assert len(a) == m
    lag = lagrange_at(roots, x)
    n = len(roots)
    at_x, at_gates = [], []
    for rows in (u, v, w):
        rr = _rows(rows, m)
        at_x.append([sum(val * lag[g] for g, val in row) % R for row in rr])
        gates = [0] * n
        for i, row in enumerate(rr):
            for g, val in row:
                gates[g] = (gates[g] + a[i] * val) % R
        at_gates.append(gates)
    ux, vx, wx = at_x
    U, V, W = (sum(ai * e for ai, e in zip(a, col)) % R for col in at_x)
    # U V - W = h t + rem, rem the polynomial of degree < n with the values U_j V_j - W_j on the roots
    rem = sum((at_gates[0][j] * at_gates[1][j] - at_gates[2][j]) * lag[j] for j in range(n)) % R
    L = sum(a[i] * (beta * ux[i] + alpha * vx[i] + wx[i]) for i in range(l + 1, m)) % R
    return Scalars(U, V, L, (U * V - W - rem) % R)


def _poly_eval(c, x):
    acc = 0
    for y in reversed(c):
        acc = (acc * x + y) % R
    return acc


def dense_scalars(u, v, w, t, l, trapdoor, weights):
    """u, v, w: (m, n, 4) coefficient limbs, t: (n + 1, 4) -- the form of the .zk front end"""
    alpha, beta, gamma, delta, x = (int(e) % R for e in trapdoor)
    a = [limbs_to_int(e) for e in weights]
    m, n = u.shape[0], u.shape[1]
    assert len(a) == m
    mats = [[[limbs_to_int(e) for e in row] for row in mat] for mat in (u, v, w)]
    tc = [limbs_to_int(e) for e in t]
    while tc and tc[-1] == 0:
        tc.pop()
    ux, vx, wx = ([_poly_eval(row, x) for row in mat] for mat in mats)
    Uc, Vc, Wc = ([sum(a[i] * mat[i][k] for i in range(m)) % R for k in range(n)] for mat in mats)
    num = [0] * (2 * n - 1)
    for i, p in enumerate(Uc):
        for j, q in enumerate(Vc):
            num[i + j] = (num[i + j] + p * q) % R
    for k, c in enumerate(Wc):
        num[k] = (num[k] - c) % R
    at_x = _poly_eval(num, x)
    d = len(tc) - 1
    lead = inv(tc[d])
    for k in range(len(num) - 1, d - 1, -1):       # long division: what is left below degree d is the remainder
        q = num[k] * lead % R
        for e in range(d + 1):
            num[k - d + e] = (num[k - d + e] - q * tc[e]) % R
    L = sum(a[i] * (beta * ux[i] + alpha * vx[i] + wx[i]) for i in range(l + 1, m)) % R
    U, V = _poly_eval(Uc, x), _poly_eval(Vc, x)
    return Scalars(U, V, L, (at_x - _poly_eval(num[:d], x)) % R)


def proof_logs(trapdoor, sc, r, s):
    """the discrete logarithms (a, b, c) of the honest proof: pyref.trapdoor_proof's closed form"""
    alpha, beta, gamma, delta, x = (int(e) % R for e in trapdoor)
    a = (alpha + sc.U + r * delta) % R
    b = (beta + sc.V + s * delta) % R
    c = ((sc.L + sc.HT) * inv(delta) + s * a + r * b - r * s * delta) % R
    return a, b, c


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _nibbles(pattern):
    return int(pattern * 32, 16) % R


# digit edges of the 4-bit fixed-base tables (64 windows; the top window of a scalar < R holds 0..3).  15 * 16^0 is the entry "15".
DIGIT_VALUES = (("0", 0), ("1", 1), ("2", 2), ("15", 15), ("16", 16), ("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2),
                ("2^253", 1 << 253), ("15*16^31", 15 * 16 ** 31), ("15*16^62", 15 * 16 ** 62), ("3*16^63", 3 * 16 ** 63),
                ("0x0f0f..", _nibbles("0f")), ("0xf0f0..", _nibbles("f0")))
# every value serves once as r and once as s: entry i is paired with entry i + 1
DIGIT_NAMES = tuple("digits:r=%s,s=%s" % (DIGIT_VALUES[i][0], DIGIT_VALUES[(i + 1) % len(DIGIT_VALUES)][0]) for i in range(len(DIGIT_VALUES)))
PAIR_NAMES = ("pair:0,0", "pair:0,s", "pair:r,0", "pair:r*s=1", "pair:r*s=r-1")
PRE_NAMES = ("pre:r*delta=alpha", "pre:r*delta=-alpha", "pre:s*delta=beta", "pre:s*delta=-beta")
FIXED_C_NAMES = ("fixed_c:s*alpha=r*beta", "fixed_c:s*alpha=-r*beta", "fixed_c:s*alpha+r*beta=r*s*delta", "fixed_c:s*alpha+r*beta=-r*s*delta")
AB_NAMES = ("a:U=alpha+r*delta", "a:infinity", "b:V=beta+s*delta", "b:infinity", "ab:both-infinity")
C_NAMES = ("c:hb=l", "c:hb=-l", "c:hb+l=fixed_c", "c:infinity")
CASE_NAMES = DIGIT_NAMES + PAIR_NAMES + PRE_NAMES + FIXED_C_NAMES + AB_NAMES + C_NAMES


def cases(trapdoor, sc, seed):
    """[Case] in the order of CASE_NAMES for one trapdoor and one witness's Scalars; `seed` draws the scalar a relation leaves free"""
    alpha, beta, gamma, delta, x = (int(e) % R for e in trapdoor)
    assert alpha and beta and delta
    U, V, L, HT = sc
    rng = SplitMix64(seed)
    di = inv(delta)
    out = []

    def add(name, r, s, holds, infinite=""):
        r, s = r % R, s % R
        assert holds(r, s), name
        a, b, c = proof_logs(trapdoor, sc, r, s)
        zero = "".join(k for k, e in zip("abc", (a, b, c)) if e == 0)
        assert zero == infinite, (name, zero, infinite)
        out.append(Case(name, r, s, infinite))

    hb = lambda r, s: (HT * di + r * V + s * U) % R              # noqa: E731  merge_lh = 0
    lq = L * di % R
    fixed_c = lambda r, s: (s * alpha + r * beta + r * s * delta) % R   # noqa: E731

    for i, name in enumerate(DIGIT_NAMES):
        r, s = DIGIT_VALUES[i][1], DIGIT_VALUES[(i + 1) % len(DIGIT_VALUES)][1]
        assert 0 <= r < R and 0 <= s < R
        add(name, r, s, lambda r_, s_, r=r, s=s: (r_, s_) == (r, s))
    assert [v for k, v in DIGIT_VALUES if k in ("15*16^31", "15*16^62", "3*16^63")] == [15 << 124, 15 << 248, 3 << 252]

    r, s = rng.fr(), rng.fr()
    add("pair:0,0", 0, 0, lambda r, s: r == 0 and s == 0)
    add("pair:0,s", 0, s, lambda r, s: r == 0 and s != 0)
    add("pair:r,0", r, 0, lambda r, s: r != 0 and s == 0)
    add("pair:r*s=1", r, inv(r), lambda r, s: r * s % R == 1)
    add("pair:r*s=r-1", r, -inv(r), lambda r, s: r * s % R == R - 1)

    # the pre-sums: [r delta] meets alpha, [s delta2] meets beta2
    add("pre:r*delta=alpha", alpha * di, rng.fr(), lambda r, s: r * delta % R == alpha)
    add("pre:r*delta=-alpha", -alpha * di, rng.fr(), lambda r, s: (r * delta + alpha) % R == 0)
    add("pre:s*delta=beta", rng.fr(), beta * di, lambda r, s: s * delta % R == beta)
    add("pre:s*delta=-beta", rng.fr(), -beta * di, lambda r, s: (s * delta + beta) % R == 0)

    # fixed_c = ([s alpha] + [r beta]) + [r s delta]
    r = rng.fr()
    add("fixed_c:s*alpha=r*beta", r, r * beta * inv(alpha), lambda r, s: s * alpha % R == r * beta % R)
    r = rng.fr()
    add("fixed_c:s*alpha=-r*beta", r, -r * beta * inv(alpha), lambda r, s: (s * alpha + r * beta) % R == 0 and r * s % R != 0)
    r = rng.fr()
    add("fixed_c:s*alpha+r*beta=r*s*delta", r, r * beta * inv(r * delta - alpha),
        lambda r, s: (s * alpha + r * beta) % R == r * s * delta % R and (s * alpha + r * beta) % R != 0)
    r = rng.fr()
    add("fixed_c:s*alpha+r*beta=-r*s*delta", r, -r * beta * inv(alpha + r * delta),
        lambda r, s: fixed_c(r, s) == 0 and (s * alpha + r * beta) % R != 0)

    # a = [U] + [alpha + r delta],  b = [V]_2 + [beta + s delta]_2
    assert U and V
    add("a:U=alpha+r*delta", (U - alpha) * di, rng.fr(), lambda r, s: U == (alpha + r * delta) % R)
    add("a:infinity", -(alpha + U) * di, rng.fr(), lambda r, s: (alpha + U + r * delta) % R == 0, "a")
    add("b:V=beta+s*delta", rng.fr(), (V - beta) * di, lambda r, s: V == (beta + s * delta) % R)
    add("b:infinity", rng.fr(), -(beta + V) * di, lambda r, s: (beta + V + s * delta) % R == 0, "b")
    add("ab:both-infinity", -(alpha + U) * di, -(beta + V) * di,
        lambda r, s: (alpha + U + r * delta) % R == 0 and (beta + V + s * delta) % R == 0, "ab")

    # c = (hb + l) + fixed_c: for a drawn r, the s of each relation
    r = rng.fr()
    add("c:hb=l", r, (lq - HT * di - r * V) * inv(U), lambda r, s: hb(r, s) == lq and lq != 0)
    r = rng.fr()
    add("c:hb=-l", r, (-lq - HT * di - r * V) * inv(U), lambda r, s: (hb(r, s) + lq) % R == 0 and lq != 0)
    r = rng.fr()
    add("c:hb+l=fixed_c", r, (r * (beta - V) - (HT + L) * di) * inv(U - alpha - r * delta),
        lambda r, s: (hb(r, s) + lq) % R == fixed_c(r, s) and fixed_c(r, s) != 0)
    r = rng.fr()
    add("c:infinity", r, -((L + HT) * di + r * (beta + V)) * inv(alpha + U + r * delta),
        lambda r, s: (hb(r, s) + lq + fixed_c(r, s)) % R == 0 and (hb(r, s) + lq) % R != 0, "c")

    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the circuits both test modules use: same seeds, so the same bytes on the host and on the device ------------------------------------
WITNESSES = ("satisfying", "broken")


def _finish(inst, trapdoor, honest, broken, scalars, seed):
    inst.update(td=trapdoor, witnesses=dict(satisfying=honest, broken=broken), inputs=[limbs_to_int(e) for e in honest[1:1 + inst["l"]]])
    inst["scalars"] = {k: scalars(w) for k, w in inst["witnesses"].items()}
    inst["cases"] = {k: cases(trapdoor, inst["scalars"][k], seed + j) for j, k in enumerate(WITNESSES)}
    assert inst["scalars"]["satisfying"].HT != inst["scalars"]["broken"].HT
    return inst


def chain_instance(log_n):
    """the chain circuit over the roots of unity, 2^log_n >= 2 gates; the broken witness has bit 0 of a_1 flipped: gate 1 fails alone"""
    import numpy as np
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    n = 1 << log_n
    rng = SplitMix64(88000 + log_n)
    m, l, u, v, w = chain_rows(log_n)
    honest = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    broken = honest.copy()
    broken[4, 0] ^= np.uint64(1)
    td = [rng.fr() for _ in range(5)]
    roots = unity_roots(log_n)
    inst = dict(kind="unity", log_n=log_n, n=n, m=m, l=l, rows=(u, v, w), roots=roots)
    return _finish(inst, td, honest, broken, lambda wts: sparse_scalars(roots, m, l, u, v, w, td, wts), 88100 + 10 * log_n)


def integers_instance(n):
    """the same circuit over the roots 1..n"""
    import numpy as np
    from test_integer_roots import chain_rows_integers, chain_weights_integers
    rng = SplitMix64(88500 + n)
    m, l, u, v, w = chain_rows_integers(n)
    honest = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    broken = honest.copy()
    broken[4, 0] ^= np.uint64(1)
    td = [rng.fr() for _ in range(5)]
    roots = list(range(1, n + 1))
    inst = dict(kind="integers", n=n, m=m, l=l, rows=(u, v, w), roots=roots)
    return _finish(inst, td, honest, broken, lambda wts: sparse_scalars(roots, m, l, u, v, w, td, wts), 88600 + 10 * n)


def dense_instance(orc, code):
    """a .zk program in the reference's coefficient form (simple.zk: inputs 3, 2, 4); the broken witness has its first private wire
    raised by one"""
    import numpy as np
    from zksnark_rs_amd import ints_to_limbs
    q = orc.zk_qap_dense(code)
    rng = SplitMix64(88900)
    honest = orc.zk_weights(code, ints_to_limbs([3, 2, 4]), q["m"])
    broken = honest.copy()
    broken[q["input"] + 1, 0] += np.uint64(1)
    td = [rng.fr() for _ in range(5)]
    inst = dict(kind="dense", n=q["n"], m=q["m"], l=q["input"], dense=q)
    return _finish(inst, td, honest, broken, lambda wts: dense_scalars(q["u"], q["v"], q["w"], q["t"], q["input"], td, wts), 88950)
