"""The coefficient-form quotient h = (U V - W) div t at its switch and edges (csrc/prove.hip, csrc/qap.hip).

The dense form and the arbitrary-roots form end in the same step, which has two implementations: the reference's long division
(k_poly_divide, one workgroup of 1024 lanes) below ZK_NEWTON_MIN_QUOTIENT = 512 quotient coefficients, and the power-series
inverse of rev(t) (poly_rev_inverse_ntt once per QAP, poly_divide_newton per proof) from there on.  With t of degree n the
quotient has K = n - 1 coefficients.  Pinned here, by equality of the 259 proof bytes and nothing weaker:

  * the switch (K = 510, 511 | 512, 513), K a power of two and K = 2^k + 1 (the last Newton step gains one coefficient),
    n = 2^k (2n - 1 product coefficients in a transform of exactly 2n);
  * divisors that are not the monic prod (x - k) every larger test uses: non-monic (the start 1 / lead(t) of the iteration),
    t = x^n and t = c x^n + t0 (rev(t) constant / sparse), a zero constant term; dividends of degree below n (zero quotient);
  * the long division around its 1024-lane stride, the cache of the inverse series per QAP, option changes, two tickets.

The reference of the GPU tests is the oracle's closed form from the trapdoor (orc.trapdoor_proof_dense: plain long division on
the host, no CRS); the CPU test below shows on every divisor shape that it is the faithful prover's bytes.  Divisors of degree
below n are not pinned here: the reference sizes the CRS by deg t, the product by n."""
import functools

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs

from test_arbitrary_roots import dense_from_rows, distinct_roots, root_poly
from test_gpu_prove import assert_crs_equal
from test_integer_roots import random_rows

R = zk.R_MODULUS
M, L = 4, 1
DIVISORS = ["roots", "monic", "lead2", "lead_rm1", "lead_rand", "xn", "binomial", "zero_const"]
WITNESSES = ["random", "short", "zero_tail", "low_degree"]


@functools.lru_cache(maxsize=None)
def integer_root_poly(n):
    t = root_poly(list(range(1, n + 1)))
    t.setflags(write=False)
    return t


def divisor(rng, n, shape):
    """n + 1 coefficient limbs of a divisor of degree exactly n"""
    if shape == "roots":
        return integer_root_poly(n)
    if shape == "xn":
        c = [0] * n + [1]
    elif shape == "binomial":
        c = [rng.fr()] + [0] * (n - 1) + [rng.fr()]
    elif shape == "zero_const":
        c = [0] + [rng.fr() for _ in range(n)]
    else:
        lead = {"monic": 1, "lead2": 2, "lead_rm1": R - 1, "lead_rand": rng.fr()}[shape]
        c = [rng.fr() for _ in range(n)] + [lead]
    assert len(c) == n + 1 and c[n] != 0
    return ints_to_limbs(c)


def instance(n, shape, witness="random", seed=0):
    """a hand-made dense QAP (m = 4 wires, l = 1; random coefficients, so U V - W leaves a remainder), its divisor, a witness, a
    trapdoor and (r, s)"""
    rng = SplitMix64(9100 + 1000 * DIVISORS.index(shape) + 100000 * WITNESSES.index(witness) + 10000000 * seed + n)
    u, v, w = (ints_to_limbs([rng.fr() for _ in range(M * n)]).reshape(M, n, 4) for _ in range(3))
    if witness == "low_degree":          # deg (U V - W) <= 4 < n: the quotient is zero
        for x in (u, v, w):
            x[:, 3:] = 0
    t = divisor(rng, n, shape)
    wts = {"random": [1] + [rng.fr() for _ in range(M - 1)], "low_degree": [1] + [rng.fr() for _ in range(M - 1)],
           "short": [1] + [rng.fr() for _ in range(M - 2)], "zero_tail": [1] + [0] * (M - 1)}[witness]
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    return dict(n=n, u=u, v=v, w=w, t=t, wts=ints_to_limbs(wts), td=td, r=rng.fr(), s=rng.fr())


def closed_form(orc, i, wts=None, r=None, s=None):
    return orc.trapdoor_proof_dense(i["u"], i["v"], i["w"], i["t"], L, i["td"], i["wts"] if wts is None else wts,
                                    i["r"] if r is None else r, i["s"] if s is None else s)


def upload(ctx, i):
    qap = ctx.qap_dense(i["u"], i["v"], i["w"], i["t"], L)
    return qap, ctx.setup(qap, i["td"])


def long_division(ctx, on):
    ctx.set_option("dense_long_division", int(on))


def prove_both_ways(ctx, crs, qap, wts, r, s):
    """(bytes under the default option, bytes with the long division forced)"""
    got = ctx.prove(crs, qap, wts, r, s)
    long_division(ctx, True)
    try:
        return got, ctx.prove(crs, qap, wts, r, s)
    finally:
        long_division(ctx, False)


# ---- the yardstick: no GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 40, 513])
def test_closed_form_is_the_faithful_prover_for_every_divisor_shape(orc, n):
    """groth16::prove restated over the CRS of groth16::setup restated (both by the reference's own long division and its inner
    products) == the closed form from the trapdoor, on all eight divisor shapes -- which is what entitles the GPU tests to the
    closed form at sizes where setup + prove on the host take seconds.  Every witness shape at n = 5; the random one at 40; at 513,
    where one faithful setup + prove takes seconds, the random one over a monic and a non-monic divisor."""
    for shape in (DIVISORS if n < 100 else ["monic", "lead_rm1"]):
        for witness in (WITNESSES if n == 5 else WITNESSES[:1]):
            i = instance(n, shape, witness)
            arrs = orc.setup_dense(i["u"], i["v"], i["w"], i["t"], L, i["td"])
            cdesc = zk.Context.crs_desc(n, M, L, arrs)
            got = orc.prove_dense(i["u"], i["v"], i["w"], i["t"], L, cdesc, i["wts"], i["r"], i["s"])
            assert got == closed_form(orc, i), (shape, witness)


# ---- the dense form ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["roots", "lead_rand"])
@pytest.mark.parametrize("n", [511, 512, 513, 514, 1025, 1026, 2048, 2049, 2050])
def test_dense_quotient_at_the_switch_and_newton_edges(ctx, orc, n, shape):
    """K = n - 1 = 510, 511 | 512, 513 (the switch), 1024, 2048 (K a power of two), 513, 1025, 2049 (one coefficient from the last
    Newton step), 2047 with n = 2^11 (the product fills its transform): both quotient paths == the closed form.  At n = 513 also
    the faithful prover over the faithful CRS, array for array."""
    i = instance(n, shape)
    qap, crs = upload(ctx, i)
    want = closed_form(orc, i)
    got, got_long = prove_both_ways(ctx, crs, qap, i["wts"], i["r"], i["s"])
    assert got == want
    assert got_long == want
    if n == 513:
        arrs = orc.setup_dense(i["u"], i["v"], i["w"], i["t"], L, i["td"])
        assert_crs_equal(ctx.crs_download(crs), arrs)
        assert got == orc.prove_dense(i["u"], i["v"], i["w"], i["t"], L, ctx.crs_desc(n, M, L, arrs), i["wts"], i["r"], i["s"])


@pytest.mark.gpu
@pytest.mark.parametrize("witness", WITNESSES)
@pytest.mark.parametrize("shape", DIVISORS)
@pytest.mark.parametrize("n", [512, 514])
def test_dense_quotient_every_divisor_shape(ctx, orc, n, shape, witness):
    """one size on each side of the switch, every divisor shape, every witness shape (low_degree: a zero quotient, so the first
    n - 1 scalars of the H product must stay zero whatever the padded buffers held): both paths == the closed form"""
    i = instance(n, shape, witness)
    qap, crs = upload(ctx, i)
    want = closed_form(orc, i)
    got, got_long = prove_both_ways(ctx, crs, qap, i["wts"], i["r"], i["s"])
    assert got == want
    assert got_long == want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["monic", "lead_rm1"])
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_long_division_around_the_workgroup_stride(ctx, orc, n, shape):
    """k_poly_divide's inner loop j <= d strides by its 1024 lanes: d + 1 = 1024 (one pass, full), 1025 and 1026 (a second pass of
    one and two lanes)"""
    i = instance(n, shape)
    qap, crs = upload(ctx, i)
    long_division(ctx, True)
    try:
        got = ctx.prove(crs, qap, i["wts"], i["r"], i["s"])
    finally:
        long_division(ctx, False)
    assert got == closed_form(orc, i)


@pytest.mark.gpu
def test_inverse_series_cache_and_option_changes(ctx, orc):
    import torch
    n = 513
    # the cached series belongs to its QAP
    a, b = instance(n, "lead_rand", seed=1), instance(n, "zero_const", seed=2)
    (qa, ca), (qb, cb) = upload(ctx, a), upload(ctx, b)
    want_a, want_b = closed_form(orc, a), closed_form(orc, b)
    assert want_a != want_b
    for i, qap, crs, want in ((a, qa, ca, want_a), (b, qb, cb, want_b), (a, qa, ca, want_a), (b, qb, cb, want_b)):
        assert ctx.prove(crs, qap, i["wts"], i["r"], i["s"]) == want
    # built on first need, undisturbed by the option
    c = instance(n, "lead2", seed=3)
    qc, cc = upload(ctx, c)
    want_c = closed_form(orc, c)
    try:
        for on in (True, False, True):
            long_division(ctx, on)
            assert ctx.prove(cc, qc, c["wts"], c["r"], c["s"]) == want_c, on
    finally:
        long_division(ctx, False)
    # two tickets in flight share the series of one QAP, each in its own work buffer
    rng = SplitMix64(9199)
    jobs = [(ints_to_limbs([1] + [rng.fr() for _ in range(M - 1)]), rng.fr(), rng.fr()) for _ in range(2)]
    dev = [torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda() for wts, _, _ in jobs]
    torch.cuda.synchronize()
    tickets = [ctx.prove_submit(cc, qc, d.data_ptr(), M, r, s) for d, (_, r, s) in zip(dev, jobs)]
    got = [ctx.prove_wait(t) for t in tickets]
    assert got[0] != got[1]
    for g, (wts, r, s) in zip(got, jobs):
        assert g == ctx.prove(cc, qc, wts, r, s)
        assert g == closed_form(orc, c, wts, r, s)


# ---- the arbitrary-roots form ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [512, 513, 514, 1025, 1026])
def test_arbitrary_roots_quotient_at_the_switch(ctx, n):
    """The form over the roots 1..n as caller data divides U V by t; the integer-roots form (pinned to the oracle by
    test_integer_roots) never divides: same CRS, same bytes, on both quotient paths.  At n = 513 and 514 also random distinct roots (0
    and 1 among them) against the dense device form over the Lagrange sums of the same rows, which the tests above tie to the oracle."""
    rng = SplitMix64(9300 + n)
    m, l = 2 * n + 7, 2
    u, v, w = (random_rows(rng, n, m, 3) for _ in range(3))
    qi = ctx.qap_sparse_integers(n, m, l, u, v, w)
    qa = ctx.qap_sparse_roots(ints_to_limbs(list(range(1, n + 1))).reshape(n, 4), m, l, u, v, w)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    ci, ca = ctx.setup(qi, td), ctx.setup(qa, td)
    assert_crs_equal(ctx.crs_download(ci), ctx.crs_download(ca))
    r, s = rng.fr(), rng.fr()
    for count in (m, m - 3):
        wts = ints_to_limbs([1] + [rng.fr() for _ in range(count - 1)])
        want = ctx.prove(ci, qi, wts, r, s)
        got, got_long = prove_both_ways(ctx, ca, qa, wts, r, s)
        assert got == want, count
        assert got_long == want, count
    if n in (513, 514):
        m = 4                  # every non-empty row costs the Python Lagrange sums n^2 steps
        roots = distinct_roots(rng, n)
        roots[0], roots[1] = 0, 1
        while True:
            u, v, w = (random_rows(rng, n, m, 3) for _ in range(3))
            if u[0][m - 1] and v[0][m - 1]:      # U and V are not zero for the shorter witness either
                break
        qs = ctx.qap_sparse_roots(ints_to_limbs(roots).reshape(n, 4), m, l, u, v, w)
        qd = ctx.qap_dense(dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots), l)
        cs, cd = ctx.setup(qs, td), ctx.setup(qd, td)
        assert_crs_equal(ctx.crs_download(cs), ctx.crs_download(cd))
        for count in (m, m - 1):
            wts = ints_to_limbs([1] + [rng.fr() for _ in range(count - 1)])
            want, want_long = prove_both_ways(ctx, cd, qd, wts, r, s)
            got, got_long = prove_both_ways(ctx, cs, qs, wts, r, s)
            assert want == want_long, count
            assert got == want, count
            assert got_long == want, count
