"""Helpers shared by the zk_crs_from_powers tests: a powers-of-tau transcript built from a KNOWN (alpha, beta, x) -- the project's
generators times the scalars x^k, alpha x^k, beta x^k -- so that the derived CRS can be compared, byte for byte, with zk_setup's for
the trapdoor (alpha, beta, 1, 1, x); sparse rows assembled from (wire, gate, value) triples; and a Python-integer model of the
derivation itself (Lagrange values from the powers' exponents, row sums, the correlation behind xi_t)."""
import numpy as np

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs

R = zk.R_MODULUS


def trapdoor(alpha, beta, x):
    """(alpha, beta, gamma = 1, delta = 1, x) as (5, 4) limbs: the trapdoor whose CRS zk_crs_from_powers derives"""
    return ints_to_limbs([alpha % R, beta % R, 1, 1, x % R])


def transcript_scalars(alpha, beta, x, n, extra=0):
    """the exponents of a transcript for n gates: (x^k for k < 2n-1+extra, x^k, alpha x^k, beta x^k for k < n+extra)"""
    xs = [1] * (2 * n - 1 + extra)
    for k in range(1, len(xs)):
        xs[k] = xs[k - 1] * x % R
    rest = xs[:n + extra]
    return xs, rest, [alpha * v % R for v in rest], [beta * v % R for v in rest]


def transcript(mul1, mul2, g1, g2, alpha, beta, x, n, extra=0):
    """dict(tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2) of canonical affine limbs.  mul1 / mul2: (points, scalars) -> points
    (Context.g1_mul_batch / g2_mul_batch, or the oracle's); g1, g2: the generators (xi_g1[0], xi_g2[0] of any zk_setup CRS)."""
    xs, rest, arest, brest = transcript_scalars(alpha, beta, x, n, extra)
    rep1 = lambda ks: mul1(np.tile(g1, (len(ks), 1)), ints_to_limbs(ks))   # noqa: E731
    return dict(tau_g1=rep1(xs), tau_g2=mul2(np.tile(g2, (len(rest), 1)), ints_to_limbs(rest)), alpha_tau_g1=rep1(arest),
                beta_tau_g1=rep1(brest), beta_g2=mul2(np.asarray(g2).reshape(1, 16), ints_to_limbs([beta % R]))[0])


def rows_from_triples(m, triples):
    """(ptr, gate, val) by wire from [(wire, gate, value)]; entries of a wire keep their order, a (wire, gate) pair may repeat"""
    by_wire = [[] for _ in range(m)]
    for wire, gate, value in triples:
        by_wire[wire].append((gate, value % R))
    ptr, gate, val = [0], [], []
    for entries in by_wire:
        for g, v in entries:
            gate.append(g)
            val.append(v)
        ptr.append(len(gate))
    return (np.array(ptr, np.uint64), np.array(gate, np.uint32), ints_to_limbs(val) if val else np.zeros((0, 4), np.uint64))


# ---- the derivation on scalars -------------------------------------------------------------------------------------------------------
def t_integers(n):
    """coefficients t_0 .. t_n of prod_{k=1..n} (X - k)"""
    t = [1]
    for k in range(1, n + 1):
        nxt = [0] * (len(t) + 1)
        for i, c in enumerate(t):
            nxt[i + 1] = (nxt[i + 1] + c) % R
            nxt[i] = (nxt[i] - k * c) % R
        t = nxt
    return t


def lagrange_coefficients_integers(n):
    """c[k][i]: coefficient i of the Lagrange polynomial of node k + 1 over 1..n (t / (X - node) by synthetic division, over t'(node))"""
    t = t_integers(n)
    out = []
    for node in range(1, n + 1):
        q, carry = [0] * n, 0
        for i in range(n, 0, -1):           # t = (X - node) q: q_{i-1} = t_i + node q_i
            carry = (t[i] + node * carry) % R
            q[i - 1] = carry
        den = 1
        for j in range(1, n + 1):
            if j != node:
                den = den * (node - j) % R
        inv = pow(den, -1, R)
        out.append([c * inv % R for c in q])
    return out


def lagrange_from_powers(powers, coeffs):
    """sum_i c[k][i] powers[i] for every k: what the three Lagrange arrays hold, on exponents"""
    return [sum(c * p for c, p in zip(ck, powers)) % R for ck in coeffs]


def lagrange_coefficients_unity(n, w):
    """c[j][k] = w^(-j k) / n over the roots w^j of X^n - 1"""
    ninv, winv = pow(n, -1, R), pow(w, -1, R)
    return [[pow(winv, j * k, R) * ninv % R for k in range(n)] for j in range(n)]


def correlation_cyclic(t, powers, n):
    """xi_t exponents the way the device forms them: the cyclic convolution of size N = 2^ceil(log2(2n - 1)) of the 2n - 1 powers with
    rev[i] = t[n - i], read at n .. 2n - 2.  Returns (values, N)."""
    N = 1
    while N < 2 * n - 1:
        N *= 2
    a = list(powers[:2 * n - 1]) + [0] * (N - (2 * n - 1))
    rev = [t[n - i] if i <= n else 0 for i in range(N)]
    c = [0] * N
    for i, ri in enumerate(rev):
        if ri:
            for s, av in enumerate(a):
                if av:
                    c[(i + s) % N] = (c[(i + s) % N] + ri * av) % R
    return [c[n + k] for k in range(n - 1)], N


def correlation_direct(t, powers, n):
    return [sum(t[j] * powers[k + j] for j in range(n + 1)) % R for k in range(n - 1)]


def wire_scalars(rows3, m, L, alpha, beta):
    """beta u_i + alpha v_i + w_i on exponents, from the three Lagrange value lists (L, alpha L, beta L are formed here)"""
    from degenerate_crs_cases import row_values
    u, v, w = rows3
    La, Lb = [alpha * e % R for e in L], [beta * e % R for e in L]
    U, V, W = row_values(u, m, Lb), row_values(v, m, La), row_values(w, m, L)
    return [(U[i] + V[i] + W[i]) % R for i in range(m)]
