"""-m "not gpu": the yardstick of tests/test_gpu_setup_edges.py -- the oracle tied to itself where the trapdoor's x is a root of t.

With x = w^j on the domain t(x) = 0: xi_t_g1 = [x^i t(x) / delta]_1 is all infinity, L_k(x) = [k == j], so u_i(x) = u_i(w^j) and every
sum_gamma / sum_delta point whose wire has no entry at gate j is infinity too.  The GPU module compares zk_setup / zk_prove with the
oracle's FAST setup and prover on such trapdoors at sizes the faithful restatement of mod.rs:134-296 cannot reach; here the fast twin,
the faithful restatement and the closed form from the trapdoor are shown to agree on exactly these edges (roots of unity up to 2^5,
integer roots up to n = 5), and the verdict rule that follows from t(x) = 0 is checked with the host verifier (csrc/vk.hip: no
context, no GPU)."""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs
from zksnark_rs_amd.circuits import chain_weights

from setup_edge_cases import (HOST_ON_DOMAIN, VERDICT_LOG_N, VERDICT_J, VERDICTS, R, chain_sparse, chain_witnesses, digit_scalars, digits,
                              is_infinity, on_domain_trapdoor, table_entries, unit_w_qap)
from test_arbitrary_roots import dense_from_rows, root_poly
from test_gpu_prove import assert_crs_equal
from test_integer_roots import chain_rows_integers, chain_weights_integers


@pytest.mark.parametrize("log_n", sorted(HOST_ON_DOMAIN))
def test_oracle_fast_equals_faithful_with_x_on_the_domain(orc, log_n):
    """x = w^j: fast setup == faithful setup on all eleven arrays; xi_t_g1 is all infinity, the powers and the four elements nowhere;
    fast prove == faithful prove == closed form, for the honest witness and (n >= 2) the two altered ones"""
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    for j in HOST_ON_DOMAIN[log_n]:
        td = on_domain_trapdoor(orc, log_n, j)
        fast = orc.setup_sparse(desc, td, n, m, l, False)
        faithful = orc.setup_sparse(desc, td, n, m, l, True)
        assert_crs_equal(fast, faithful)
        assert fast["xi_t_g1"].shape == (n - 1, 8) and is_infinity(fast["xi_t_g1"]).all(), j
        assert not is_infinity(fast["xi_g1"]).any() and not is_infinity(fast["xi_g2"]).any(), j
        for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2"):
            assert fast[k].any(), (j, k)
        # only the wires with an entry at gate j keep a finite point
        assert is_infinity(fast["sum_delta_g1"]).sum() >= (m - l - 1) - 3, j
        cdesc = zk.Context.crs_desc(n, m, l, fast)
        rng = SplitMix64(34000 + 100 * log_n + j)
        r, s = rng.fr(), rng.fr()
        if n >= 2:
            witnesses = chain_witnesses(log_n, j)
        else:
            witnesses = (chain_weights(0, rng.fr(), [rng.fr()]),)
        proofs = []
        for wts in witnesses:
            want = orc.trapdoor_proof_sparse(desc, td, wts, r, s)
            assert orc.prove_sparse(desc, cdesc, wts, r, s, True) == want, j
            assert orc.prove_sparse(desc, cdesc, wts, r, s, False) == want, j
            proofs.append(want)
        if n >= 2:      # a_k of another gate multiplies v_i(x) = L_k(x) = 0 and the quotient meets only infinity: the SAME bytes
            assert proofs[1] != proofs[0] and proofs[2] == proofs[0], j


@pytest.mark.parametrize("n", [1, 2, 5])
def test_oracle_dense_setup_with_x_on_an_integer_root(orc, n):
    """the reference's coefficient form over the roots 1..n with x = 1 and x = n: Horner gives t(x) = 0, setup succeeds with an
    all-infinity xi_t_g1, and the faithful prover over that CRS gives the closed form's bytes"""
    m, l, u, v, w = chain_rows_integers(n)
    roots = list(range(1, n + 1))
    du, dv, dw, dt = dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots)
    rng = SplitMix64(35000 + n)
    honest = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    bad = honest.copy()
    bad[m - 1, 0] ^= np.uint64(1)
    for x in sorted({1, n}):
        td = ints_to_limbs([rng.fr() for _ in range(4)] + [x])
        arrs = orc.setup_dense(du, dv, dw, dt, l, td)
        assert arrs["xi_t_g1"].shape == (n - 1, 8) and is_infinity(arrs["xi_t_g1"]).all(), x
        assert not is_infinity(arrs["xi_g1"]).any() and not is_infinity(arrs["xi_g2"]).any(), x
        cdesc = zk.Context.crs_desc(n, m, l, arrs)
        r, s = rng.fr(), rng.fr()
        for wts in (honest, bad):
            assert orc.prove_dense(du, dv, dw, dt, l, cdesc, wts, r, s) == orc.trapdoor_proof_dense(du, dv, dw, dt, l, td, wts, r, s), x


@pytest.mark.parametrize("j", VERDICT_J)
def test_only_the_gate_at_x_is_checked(orc, j):
    """The verdict rule of a CRS with x = w^j.  The pairing equation says A B = alpha beta + gamma (sum over the public wires) +
    delta C in the exponent, which for the prover's A, B, C is U(x) V(x) = W(x) + h(x) t(x); with t(x) = 0 and L_k(x) = [k == j] that
    is U_j V_j = W_j, the constraint of gate j alone.  So over this CRS: an honest witness verifies; one whose gate j fails is
    rejected; one whose only failing gate is another one (same public inputs) VERIFIES.  That is what the reference does on such a
    CRS (groth16::verify, mod.rs:299-320, has no other input than these points), which is why a trapdoor on the domain must never be
    used -- the device reproduces it rather than hiding it.  Checked with the host verifier over the oracle's CRS."""
    log_n = VERDICT_LOG_N
    n, m, l, u, v, w, desc = chain_sparse(log_n)
    td = on_domain_trapdoor(orc, log_n, j)
    arrs = orc.setup_sparse(desc, td, n, m, l, True)
    key = zk.VerifyingKey.from_points(arrs["alpha_g1"], arrs["beta_g2"], arrs["gamma_g2"], arrs["delta_g2"], arrs["sum_gamma_g1"])
    cdesc = zk.Context.crs_desc(n, m, l, arrs)
    rng = SplitMix64(36000 + j)
    r, s = rng.fr(), rng.fr()
    witnesses = chain_witnesses(log_n, j)
    got = [key.verify(wts[1:1 + l], orc.prove_sparse(desc, cdesc, wts, r, s, True)) for wts in witnesses]
    assert tuple(got) == VERDICTS
    # the same three proofs over a CRS with a generic x: both altered witnesses are rejected
    td2 = td.copy()
    td2[4] = ints_to_limbs([rng.fr()])[0]
    arrs2 = orc.setup_sparse(desc, td2, n, m, l, True)
    key2 = zk.VerifyingKey.from_points(arrs2["alpha_g1"], arrs2["beta_g2"], arrs2["gamma_g2"], arrs2["delta_g2"], arrs2["sum_gamma_g1"])
    cdesc2 = zk.Context.crs_desc(n, m, l, arrs2)
    got2 = [key2.verify(wts[1:1 + l], orc.prove_sparse(desc, cdesc2, wts, r, s, True)) for wts in witnesses]
    assert got2 == [True, False, False]


def test_digit_scalars_reach_every_table_entry(orc):
    """the inputs of the fixed-base table test: every (window, digit) entry a scalar < r can select is the ONLY digit of one scalar,
    the top window has exactly the digits 1..3, and with gamma = delta = 1, x = 1 the oracle's setup of the one-gate QAP built from
    them gives sum_gamma | sum_delta = [s_i]_1 -- the identity the device test relies on"""
    entries = table_entries()
    assert len(entries) == 63 * 15 + 3 and [d for w_, d in entries if w_ == 63] == [1, 2, 3]
    scalars = digit_scalars()
    alone = {next(iter(digits(s))) for s in scalars if len(digits(s)) == 1}
    assert alone == set(entries)
    assert {0, 1, R - 1} <= set(scalars) and len(scalars) <= 1100
    m, l, u, v, w = unit_w_qap(scalars)
    desc = zk.Context.sparse_desc(0, m, l, u, v, w)
    rng = SplitMix64(37000)
    td = ints_to_limbs([rng.fr(), rng.fr(), 1, 1, 1])
    want = orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (m, 1)), ints_to_limbs(scalars))
    for faithful in (True, False):
        arrs = orc.setup_sparse(desc, td, 1, m, l, faithful)
        assert arrs["xi_t_g1"].shape == (0, 8)
        assert np.array_equal(np.concatenate([arrs["sum_gamma_g1"], arrs["sum_delta_g1"]]), want), faithful
    assert is_infinity(want).sum() == 1 and is_infinity(want)[scalars.index(0)]
