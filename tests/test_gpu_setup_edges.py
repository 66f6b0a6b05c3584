"""zk_setup at the trapdoor's edges (csrc/crs.hip, csrc/aproots.hip, csrc/arbroots.hip): the special cases no random draw reaches.

  * x on the domain, roots of unity (k_setup_consts: lag_c = 0, tx_dinv = 0; k_lagrange_at: the den.is_zero() lane): the CRS with an
    all-infinity xi_t_g1 that the reference emits, array for array, and proofs over it through every entry point -- the prover's
    H product then runs over a table of nothing but infinity;
  * the refusals of the integer-roots and arbitrary-roots forms (ZK_ERR_UNSUPPORTED) at the ends of their ranges, the dense form's
    acceptance of the same x, and the argument rules (zero, >= r) for each of the five elements; nothing leaks into the next call;
  * alpha, beta, gamma, delta at 1, r - 1, (r - 1) / 2, 2^253 and equal to each other;
  * every entry of the fixed-base tables (k_fixed_table / k_fixed_base_mul) against plain scalar multiplications on the host, which
    share nothing with either setup: with x on the domain the scalars of the CRS are the caller's.

References: the oracle's setup / prover (faithful where it is fast enough, else the fast twin) and the closed form from the trapdoor;
tests/test_setup_edges.py ties these three to each other on exactly these trapdoors.  Equality of words and of proof bytes only."""
import ctypes as C

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, _lib, ints_to_limbs, limbs_to_int
from zksnark_rs_amd.circuits import chain_weights

import setup_edge_cases as sec
from setup_edge_cases import R, chain_sparse, chain_witnesses, is_infinity, on_domain_trapdoor
from test_arbitrary_roots import dense_from_rows, distinct_roots, root_poly
from test_gpu_prove import assert_crs_equal
from test_integer_roots import chain_rows_integers, chain_weights_integers, random_rows

pytestmark = pytest.mark.gpu


def status_of(call):
    with pytest.raises(zk.ZkError) as e:
        call()
    return e.value.status


def generic_trapdoor(seed):
    rng = SplitMix64(38000 + seed)
    return ints_to_limbs([rng.fr() for _ in range(5)])


def with_x(td, x):
    out = np.array(td, dtype=np.uint64).reshape(5, 4).copy()
    out[4] = ints_to_limbs([x])[0]
    return out


def to_device(wts):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


# ---- 2. x on the domain, roots of unity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", sorted(sec.GPU_ON_DOMAIN))
def test_setup_with_x_on_the_domain_matches_oracle(ctx, orc, log_n):
    """x = w^j: all eleven arrays == the oracle's (faithful up to 2^3, fast above), xi_t_g1 all zero words; between the first two
    on-domain setups one with a generic x on the same context and QAP handle, compared as well"""
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    faithful = log_n <= 3
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    for k, j in enumerate(sec.GPU_ON_DOMAIN[log_n]):
        td = on_domain_trapdoor(orc, log_n, j)
        got = ctx.crs_download(ctx.setup(qap, td))
        assert_crs_equal(got, orc.setup_sparse(desc, td, n, m, l, faithful))
        assert got["xi_t_g1"].shape == (n - 1, 8) and not got["xi_t_g1"].any(), j
        assert not is_infinity(got["xi_g1"]).any() and not is_infinity(got["xi_g2"]).any(), j
        if k == 0:
            tg = generic_trapdoor(log_n)
            got = ctx.crs_download(ctx.setup(qap, tg))
            assert_crs_equal(got, orc.setup_sparse(desc, tg, n, m, l, faithful))
            assert not is_infinity(got["xi_t_g1"]).any()


@pytest.mark.parametrize("log_n,j", [(log_n, j) for log_n in sorted(sec.GPU_ON_DOMAIN_PROVE) for j in sec.GPU_ON_DOMAIN_PROVE[log_n]])
def test_prove_and_verify_over_the_degenerate_crs(ctx, orc, log_n, j):
    """Proofs over the CRS of x = w^j (xi_t | the Lagrange-basis H points all infinity, sum_delta almost all): zk_prove with the merged
    and the separate L / H products, over the set-up and over the uploaded CRS, == the oracle's fast prover == the closed form, for
    the honest witness, one whose gate j fails and one whose only failing gate is another; zk_verify and zk_verify_batch accept,
    reject, accept (tests/test_setup_edges.py: only the gate at x is checked -- the third proof is the first one's bytes).  At 2^9
    also the pipelined entry point and a batch of the three."""
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    td = on_domain_trapdoor(orc, log_n, j)
    crs = ctx.setup(qap, td)
    arrs = ctx.crs_download(crs)
    assert not arrs["xi_t_g1"].any()
    cdesc = ctx.crs_desc(n, m, l, arrs)
    up = ctx.crs_upload(n, m, l, arrs)            # zk_crs_upload accepts the all-infinity xi_t_g1
    assert_crs_equal(ctx.crs_download(up), arrs)
    rng = SplitMix64(39000 + 100 * log_n + j)
    r, s = rng.fr(), rng.fr()
    witnesses = chain_witnesses(log_n, j)
    want = []
    for wts in witnesses:
        want.append(orc.prove_sparse(desc, cdesc, wts, r, s, False))
        assert want[-1] == orc.trapdoor_proof_sparse(desc, td, wts, r, s)
    assert want[1] != want[0] and want[2] == want[0]
    try:
        for merge in (1, 0):
            ctx.set_option("merge_lh", merge)
            for c in (crs, up):
                for wts, wp in zip(witnesses, want):
                    assert ctx.prove(c, qap, wts, r, s) == wp, merge
    finally:
        ctx.set_option("merge_lh", 1)
    if log_n == 9:
        dev = [to_device(wts) for wts in witnesses]
        tickets = [ctx.prove_submit(crs, qap, d.data_ptr(), m, r, s) for d in dev[:2]]
        assert [ctx.prove_wait(t) for t in tickets] == want[:2]
        assert ctx.prove_wait(ctx.prove_submit(up, qap, dev[2].data_ptr(), m, r, s)) == want[2]
        t = ctx.prove_batch_submit(crs, qap, [d.data_ptr() for d in dev], [m] * 3, [r] * 3, [s] * 3)
        assert ctx.prove_batch_wait(t, 3) == want
    pub = [wts[1:1 + l] for wts in witnesses]
    for c in (crs, up):
        single = [ctx.verify(c, p, pf) for p, pf in zip(pub, want)]
        assert tuple(single) == sec.VERDICTS
        assert tuple(ctx.verify_batch(c, np.stack(pub), want)) == sec.VERDICTS


# ---- 3. refusals and their ends --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sec.INTEGER_SIZES)
def test_integer_roots_refusals_at_the_ends_of_their_range(ctx, orc, n):
    """k_ap_lagrange raises its flag for x in 1..2n-1 (the roots 1..n and the second set n+1..2n-1 of the Lagrange-basis H points):
    ZK_ERR_UNSUPPORTED at 1, n, n + 1, 2n - 1; 2n and r - 1 are accepted with the reference's CRS.  After every refusal the same
    context and QAP handle set up with a generic x exactly as before."""
    if n <= 5:
        m, l, u, v, w = chain_rows_integers(n)
    else:
        rng = SplitMix64(40000 + n)
        m, l = 4, 1                          # every non-empty row costs the Python Lagrange sums n^2 steps
        u, v, w = (random_rows(rng, n, m, 3) for _ in range(3))
    roots = list(range(1, n + 1))
    du, dv, dw, dt = dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots)
    desc = ctx.sparse_desc(0, m, l, u, v, w)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    tg = generic_trapdoor(100 + n)
    before = ctx.crs_download(ctx.setup(qap, tg))
    refused = sec.integer_refused(n)
    assert refused[0] == 1 and refused[-1] == 2 * n - 1
    for x in refused:
        assert status_of(lambda: ctx.setup(qap, with_x(tg, x))) == _lib.ZK_ERR_UNSUPPORTED, x
        assert_crs_equal(ctx.crs_download(ctx.setup(qap, tg)), before)
    rng = SplitMix64(41000 + n)
    r, s = rng.fr(), rng.fr()
    wts = ints_to_limbs([1] + [rng.fr() for _ in range(m - 1)])
    for x in sec.integer_accepted(n):
        td = with_x(tg, x)
        crs = ctx.setup(qap, td)
        got = ctx.crs_download(crs)
        if n <= 5:
            assert_crs_equal(got, orc.setup_dense(du, dv, dw, dt, l, td))
        else:
            qd = ctx.qap_dense(du, dv, dw, dt, l)
            assert_crs_equal(got, ctx.crs_download(ctx.setup(qd, td)))
        assert ctx.prove(crs, qap, wts, r, s) == orc.trapdoor_proof_integers(desc, n, td, wts, r, s), x


@pytest.mark.parametrize("n", sec.ARBITRARY_SIZES)
def test_arbitrary_roots_refusals(ctx, orc, n):
    """k_arb_lagrange: x on the first, the middle and the last root is refused with ZK_ERR_UNSUPPORTED (at 257 roots the last one is
    the only lane of the second block); x = a root + 1 is accepted and gives the dense form's CRS (up to 5 gates: the oracle's)"""
    rng = SplitMix64(42000 + n)
    roots = distinct_roots(rng, n)
    m, l = 4, 1
    u, v, w = (random_rows(rng, n, m, 3) for _ in range(3))
    du, dv, dw, dt = dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots)
    qs = ctx.qap_sparse_roots(ints_to_limbs(roots).reshape(n, 4), m, l, u, v, w)
    qd = ctx.qap_dense(du, dv, dw, dt, l)
    tg = generic_trapdoor(200 + n)
    before = ctx.crs_download(ctx.setup(qs, tg))
    for k in sorted({0, n // 2, n - 1}):
        assert status_of(lambda: ctx.setup(qs, with_x(tg, roots[k]))) == _lib.ZK_ERR_UNSUPPORTED, k
        assert_crs_equal(ctx.crs_download(ctx.setup(qs, tg)), before)
        x = next(y for y in ((roots[k] + d) % R for d in range(1, n + 2)) if y and y not in roots)
        td = with_x(tg, x)
        got = ctx.crs_download(ctx.setup(qs, td))
        assert_crs_equal(got, ctx.crs_download(ctx.setup(qd, td)))
        if n <= 5:
            assert_crs_equal(got, orc.setup_dense(du, dv, dw, dt, l, td))


def chain_dense(n, roots):
    m, l, u, v, w = chain_rows_integers(n)
    return m, l, dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots)


@pytest.mark.parametrize("kind,n", [("integers", 1), ("integers", 2), ("integers", 5), ("arbitrary", 5)])
def test_dense_form_accepts_x_on_a_root(ctx, orc, kind, n):
    """the coefficient form over the same roots takes the x the sparse forms refuse: Horner gives t(x) = 0, xi_t_g1 is all infinity,
    the CRS and the proofs (honest witness, altered witness) are the faithful oracle's"""
    rng = SplitMix64(43000 + n + (100 if kind == "arbitrary" else 0))
    roots = list(range(1, n + 1)) if kind == "integers" else distinct_roots(rng, n)
    m, l, du, dv, dw, dt = chain_dense(n, roots)
    qd = ctx.qap_dense(du, dv, dw, dt, l)
    honest = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    bad = honest.copy()
    bad[m - 1] = ints_to_limbs([(limbs_to_int(honest[m - 1]) + 1) % R])[0]
    for k in sorted({0, n // 2, n - 1}):
        td = with_x(generic_trapdoor(300 + 10 * n + k), roots[k])
        crs = ctx.setup(qd, td)
        got = ctx.crs_download(crs)
        assert_crs_equal(got, orc.setup_dense(du, dv, dw, dt, l, td))
        assert got["xi_t_g1"].shape == (n - 1, 8) and not got["xi_t_g1"].any(), k
        cdesc = ctx.crs_desc(n, m, l, got)
        r, s = rng.fr(), rng.fr()
        for wts in (honest, bad):
            want = orc.prove_dense(du, dv, dw, dt, l, cdesc, wts, r, s)
            assert ctx.prove(crs, qd, wts, r, s) == want, k
            assert want == orc.trapdoor_proof_dense(du, dv, dw, dt, l, td, wts, r, s), k


def test_dense_form_accepts_x_on_a_root_past_the_newton_switch(ctx, orc):
    """n = 600 (599 quotient coefficients: the power-series division): x = 1, 300, 600 on a root of t = prod (x - k); all 599 points
    of xi_t_g1 are infinity and a proof == the closed form from the trapdoor, for two witnesses"""
    n, m, l = 600, 4, 1
    rng = SplitMix64(44000)
    u, v, w = (ints_to_limbs([rng.fr() for _ in range(m * n)]).reshape(m, n, 4) for _ in range(3))
    t = root_poly(list(range(1, n + 1)))
    qd = ctx.qap_dense(u, v, w, t, l)
    first = ints_to_limbs([1] + [rng.fr() for _ in range(m - 1)])
    second = first.copy()
    second[m - 1, 0] ^= np.uint64(1)
    r, s = rng.fr(), rng.fr()
    for x in (1, 300, 600):
        td = with_x(generic_trapdoor(400 + x), x)
        crs = ctx.setup(qd, td)
        got = ctx.crs_download(crs)
        assert got["xi_t_g1"].shape == (n - 1, 8) and not got["xi_t_g1"].any(), x
        assert not is_infinity(got["xi_g1"]).any() and not is_infinity(got["sum_delta_g1"]).any(), x
        for wts in ((first, second) if x == 300 else (first,)):
            assert ctx.prove(crs, qd, wts, r, s) == orc.trapdoor_proof_dense(u, v, w, t, l, td, wts, r, s), x


def test_argument_rules_for_each_of_the_five_elements(ctx, orc):
    """alpha, beta, gamma, delta, x in turn: 0 -> ZK_ERR_DIV_BY_ZERO, r and 2^256 - 1 -> ZK_ERR_RANGE, *out left NULL; the context and
    the QAP handle serve the next call"""
    log_n = 1
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    tg = generic_trapdoor(500)
    want = orc.setup_sparse(desc, tg, n, m, l, True)
    for pos in range(5):
        for value, name in sec.BAD_ELEMENTS:
            td = np.ascontiguousarray(tg.copy())
            td[pos] = ints_to_limbs([value])[0]
            out = C.c_void_p(0x1234)
            rc = ctx.lib.zk_setup(ctx.ptr, qap.ptr, td.ctypes.data_as(_lib.u64p), C.byref(out))
            assert rc == getattr(_lib, name), (pos, name)
            assert not out.value, (pos, name)
            assert status_of(lambda: ctx.setup(qap, td)) == rc
        assert_crs_equal(ctx.crs_download(ctx.setup(qap, tg)), want)


# ---- 4. trapdoor scalars at their ends -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", sec.SCALAR_EDGES, ids=[name for name, _ in sec.SCALAR_EDGES])
def test_trapdoor_scalars_at_their_ends(ctx, orc, name, spec):
    """alpha .. delta at 1 (the inverses are 1), r - 1 (= -1), (r - 1) / 2, 2^253 (top digit 2, all others 0), gamma = delta with
    alpha = beta, each alone at r - 1: all eleven arrays and one proof == the faithful oracle's"""
    log_n = 3
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    td = sec.scalar_edge_trapdoor(spec, [k for k, _ in sec.SCALAR_EDGES].index(name))
    crs = ctx.setup(qap, td)
    got = ctx.crs_download(crs)
    assert_crs_equal(got, orc.setup_sparse(desc, td, n, m, l, True))
    rng = SplitMix64(45000 + len(name))
    wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    r, s = rng.fr(), rng.fr()
    assert ctx.prove(crs, qap, wts, r, s) == orc.prove_sparse(desc, ctx.crs_desc(n, m, l, got), wts, r, s, True)


# ---- 5. every entry of the fixed-base tables -------------------------------------------------------------------------------------
def test_every_g1_table_entry_against_plain_scalar_multiplication(ctx, orc):
    """One-gate QAP, x = 1 = w^0 (L = [1]), gamma = delta = 1, one wire per scalar with the single entry w_i(gate 0) = s_i:
    sum_gamma | sum_delta = [s_i]_1, which must be the host's double-and-add s_i * base -- no setup code on the reference side.
    The scalars select every entry FT[w][d] of k_fixed_table that a scalar < r can (the top window has d <= 3 only), each as the
    only digit of one scalar, then long runs of digit 15, 0, 1 and r - 1."""
    scalars = sec.digit_scalars()
    reached = set().union(*(sec.digits(s) for s in scalars))
    assert reached >= set(sec.table_entries()) and len(sec.table_entries()) == 63 * 15 + 3     # the inputs cannot silently shrink
    m, l, u, v, w = sec.unit_w_qap(scalars)
    qap = ctx.qap_sparse(0, m, l, u, v, w)
    rng = SplitMix64(46000)
    td = ints_to_limbs([rng.fr(), rng.fr(), 1, 1, 1])
    got = ctx.crs_download(ctx.setup(qap, td))
    want = orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (m, 1)), ints_to_limbs(scalars))
    both = np.concatenate([got["sum_gamma_g1"], got["sum_delta_g1"]])
    assert both.shape == want.shape
    wrong = np.flatnonzero((both != want).any(axis=1))
    assert wrong.size == 0, [hex(scalars[i]) for i in wrong[:8]]
    assert is_infinity(both).sum() == 1 and is_infinity(both)[scalars.index(0)]
    assert got["xi_t_g1"].shape == (0, 8)
    assert np.array_equal(got["xi_g1"][0], orc.enc_base_g1()) and np.array_equal(got["xi_g2"][0], orc.enc_base_g2())
    assert_crs_equal(got, orc.setup_sparse(ctx.sparse_desc(0, m, l, u, v, w), td, 1, m, l, False))


@pytest.mark.parametrize("log_n,x", sec.G2_POWER_CASES)
def test_power_arrays_against_plain_scalar_multiplication(ctx, orc, log_n, x):
    """x = 2 at 2^8 gates (scalars 2^i: one bit each, reduced mod r from i = 254) and x = 16 at 2^6 (16^i: digit 1 of window i, the G2
    table's diagonal): xi_g2[i] and xi_g1[i] == the host's (x^i mod r) * base"""
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    got = ctx.crs_download(ctx.setup(qap, with_x(generic_trapdoor(600 + x), x)))
    powers = ints_to_limbs([pow(x, i, R) for i in range(n)])
    assert np.array_equal(got["xi_g2"], orc.g2_mul_batch(np.tile(orc.enc_base_g2(), (n, 1)), powers))
    assert np.array_equal(got["xi_g1"], orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (n, 1)), powers))


def test_g2_elements_against_plain_scalar_multiplication(ctx, orc):
    """beta = gamma = delta at 15 16^w (w = 0, 31, 62), 3 16^63 (the top window's last entry), r - 1 and 1, one gate: beta_g2,
    gamma_g2, delta_g2 (and beta_g1, delta_g1) == the host's scalar multiplication of the base"""
    n, m, l, u, v, w, desc = chain_sparse(0)
    qap = ctx.qap_sparse(0, m, l, u, v, w)
    for k, e in enumerate(sec.G2_ELEMENTS):
        tg = generic_trapdoor(700 + k)
        td = ints_to_limbs([limbs_to_int(tg[0]), e, e, e, limbs_to_int(tg[4])])
        got = ctx.crs_download(ctx.setup(qap, td))
        want2 = orc.g2_mul_batch(orc.enc_base_g2(), ints_to_limbs([e]))[0]
        want1 = orc.g1_mul_batch(orc.enc_base_g1(), ints_to_limbs([e]))[0]
        for key in ("beta_g2", "gamma_g2", "delta_g2"):
            assert np.array_equal(got[key], want2), (hex(e), key)
        for key in ("beta_g1", "delta_g1"):
            assert np.array_equal(got[key], want1), (hex(e), key)
