"""The derivation behind zk_crs_from_powers on Python integers, independent of the device code (tests/powers_cases.py): Lagrange
values as linear combinations of the powers' exponents, row sums, and the correlation behind xi_t with its cyclic size.  Every scalar
is turned into a point with the oracle's multiplication and the eleven arrays are compared with

  * degenerate_crs_cases.scalar_crs (prefix / suffix products of x - j: shares no formula with the coefficient route taken here), and
  * the oracle's faithful setup over the dense QAP of the same rows,

for the trapdoor (alpha, beta, 1, 1, x) at n = 2, 5, 17, with a drawn x and with x on a root.  Words only, no GPU."""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs, limbs_to_int

import degenerate_crs_cases as dc
import powers_cases as pc
from test_degenerate_crs import dense

R = zk.R_MODULUS
SIZES = (2, 5, 17)


def model_crs(orc, n, m, l, rows3, alpha, beta, x, coeffs, t):
    """the eleven arrays the way zk_crs_from_powers forms them, on exponents: nothing here evaluates a polynomial at x"""
    xs, rest, arest, brest = pc.transcript_scalars(alpha, beta, x, n)
    L = pc.lagrange_from_powers(rest, coeffs)
    La, Lb = pc.lagrange_from_powers(arest, coeffs), pc.lagrange_from_powers(brest, coeffs)
    assert La == [alpha * e % R for e in L] and Lb == [beta * e % R for e in L]        # one linear map over three arrays
    y = pc.wire_scalars(rows3, m, L, alpha, beta)
    xi_t, N = pc.correlation_cyclic(t, xs, n)
    g1, g2 = orc.enc_base_g1(), orc.enc_base_g2()
    mul1 = lambda ks: orc.g1_mul_batch(np.tile(g1, (len(ks), 1)), ints_to_limbs(ks)) if ks else np.zeros((0, 8), np.uint64)   # noqa: E731
    mul2 = lambda ks: orc.g2_mul_batch(np.tile(g2, (len(ks), 1)), ints_to_limbs(ks))                                          # noqa: E731
    return dict(alpha_g1=mul1([arest[0]])[0], beta_g1=mul1([brest[0]])[0], delta_g1=mul1([xs[0]])[0], xi_g1=mul1(rest),
                sum_gamma_g1=mul1(y[:l + 1]), sum_delta_g1=mul1(y[l + 1:]), xi_t_g1=mul1(xi_t), beta_g2=mul2([beta])[0],
                gamma_g2=mul2([rest[0]])[0], delta_g2=mul2([rest[0]])[0], xi_g2=mul2(rest)), L, xi_t, N


def cases(n):
    rng = SplitMix64(89000 + n)
    out = [("drawn", rng.fr()), ("2n", 2 * n), ("on a root", n), ("minus one", R - 1)]
    assert out[0][1] > 2 * n
    return [(name, rng.fr(), rng.fr(), x) for name, x in out]


@pytest.mark.parametrize("n", SIZES)
def test_model_over_the_integer_roots_is_scalar_crs_and_the_oracles_setup(orc, n):
    m, l, u, v, w, _ = dc.chain(n)
    du, dv, dw, dt = dense(n)
    coeffs, t = pc.lagrange_coefficients_integers(n), pc.t_integers(n)
    assert [limbs_to_int(c) for c in dt] == t                     # the t the oracle divides by
    for name, alpha, beta, x in cases(n):
        got, L, xi_t, N = model_crs(orc, n, m, l, (u, v, w), alpha, beta, x, coeffs, t)
        assert L == dc.lagrange_values(n, x)[0], name
        td = [alpha, beta, 1, 1, x]
        for label, want in (("scalar_crs", dc.scalar_crs(orc, n, m, l, u, v, w, td)), ("oracle", orc.setup_dense(du, dv, dw, dt, l, ints_to_limbs(td)))):
            assert sorted(got) == sorted(want) and len(want) == 11
            for key in want:
                assert np.array_equal(got[key], want[key]), (name, label, key)
        assert (not any(xi_t)) == (name == "on a root"), name


@pytest.mark.parametrize("n", SIZES + (3, 4, 8, 9))
def test_the_cyclic_size_of_the_correlation(n):
    """N = 2^ceil(log2(2n - 1)) is enough, and the next smaller power of two is not: the linear convolution of rev(t) (n + 1 terms)
    with 2n - 1 powers ends at index 3n - 2, the wanted indices are n .. 2n - 2, and n + N > 3n - 2 iff N >= 2n - 1"""
    rng = SplitMix64(89100 + n)
    x = rng.fr()
    xs = [pow(x, k, R) for k in range(2 * n - 1)]
    t = pc.t_integers(n)
    assert len(t) == n + 1 and t[n] == 1
    tx = sum(c * pow(x, j, R) for j, c in enumerate(t)) % R
    direct = pc.correlation_direct(t, xs, n)
    assert direct == [xs[k] * tx % R for k in range(n - 1)]       # [x^k t(x)]
    cyc, N = pc.correlation_cyclic(t, xs, n)
    assert N >= 2 * n - 1 > N // 2 and cyc == direct
    if n >= 2:                                                    # half the size folds index 2n - 2 + ... onto the wanted ones
        half = N // 2
        a = xs + [0] * max(0, half - len(xs))
        c = [0] * half
        for i in range(n + 1):
            for s_, av in enumerate(a):
                c[(i + s_) % half] = (c[(i + s_) % half] + t[n - i] * av) % R
        assert [c[(n + k) % half] for k in range(n - 1)] != direct


@pytest.mark.parametrize("log_n", [1, 2, 4])
def test_model_over_the_roots_of_unity(orc, log_n):
    """[L_j] = 1/n sum_k w^-jk [x^k] and xi_t[k] = x^(n+k) - x^k, against the closed form zk_setup uses (k_lagrange_at:
    (x^n - 1)/n w^j / (x - w^j))"""
    n = 1 << log_n
    w = limbs_to_int(orc.root_of_unity(log_n))
    assert pow(w, n, R) == 1 and pow(w, n // 2, R) == R - 1
    coeffs = pc.lagrange_coefficients_unity(n, w)
    rng = SplitMix64(89200 + n)
    for x in (rng.fr(), pow(w, 3 % n, R), 1, R - 1):
        xs = [pow(x, k, R) for k in range(2 * n - 1)]
        L = pc.lagrange_from_powers(xs[:n], coeffs)
        tx = (pow(x, n, R) - 1) % R
        for j in range(n):
            wj = pow(w, j, R)
            want = 1 if x == wj else tx * pow(n, -1, R) % R * wj % R * pow((x - wj) % R, -1, R) % R
            assert L[j] == want, (x, j)
        assert [(xs[n + k] - xs[k]) % R for k in range(n - 1)] == [xs[k] * tx % R for k in range(n - 1)]
