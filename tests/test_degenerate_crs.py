"""The references of test_gpu_degenerate_crs.py tied to the faithful oracle, on exactly the trapdoors of degenerate_crs_cases.py
(x = 0, 1, -1, of short period, the tree's own twiddle, on the roots 1..n, on the second node set n+1..2n-1):

  * scalar_crs (Python integers, Lagrange values by prefix and suffix products) == the oracle's setup over the dense QAP that
    QAP::from builds from the same rows, all eleven arrays;
  * crs_check_model.lagrange_arrays satisfies the transpose identity sum_k k^i [L_k(x)] == [x^i] against the oracle's MSM, which shares
    nothing with the model's product formula;
  * the closed form trapdoor_proof_integers == the faithful prove_dense over the scalar_crs arrays, satisfying and broken witnesses.

Equality of words and of proof bytes only."""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs

import crs_check_model as ccm
import degenerate_crs_cases as dc
from degenerate_crs_cases import R
from test_arbitrary_roots import dense_from_rows, root_poly

_dense = {}


def dense(n):
    """the chain circuit over 1..n as coefficient matrices: the only use of dense_from_rows here (n <= 17)"""
    if n not in _dense:
        assert n <= 17
        m, l, u, v, w, _ = dc.chain(n)
        roots = list(range(1, n + 1))
        _dense[n] = (dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots))
    return _dense[n]


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


@pytest.mark.parametrize("n", dc.HOST_SIZES)
def test_scalar_crs_is_the_oracles_setup(orc, n):
    m, l, u, v, w, _ = dc.chain(n)
    du, dv, dw, dt = dense(n)
    classes = dc.x_classes(orc, n)
    assert len(classes) == dc.CLASS_COUNT[n]
    for index, (name, x) in enumerate(classes):
        td = dc.trapdoor(n, index, x)
        got = dc.scalar_crs(orc, n, m, l, u, v, w, td)
        want = orc.setup_dense(du, dv, dw, dt, l, ints_to_limbs(td))
        assert sorted(got) == sorted(want) and len(want) == 11
        for key in want:
            assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (name, x, key)
        if dc.on_roots(n, x):
            assert not got["xi_t_g1"].any(), (name, x)
        else:
            assert got["xi_t_g1"][0].any(), (name, x)


def test_class_lists_are_complete(orc):
    """per n: the stated number of distinct x, every class of the table (n = 2: those whose x exists there), the two trapdoors the
    device test contributes to, and the twiddle of the padded tree"""
    for n in sorted(set(dc.HOST_SIZES) | set(dc.GPU_SIZES)):
        classes = dc.x_classes(orc, n)
        xs = [x for _, x in classes]
        assert len(classes) == dc.CLASS_COUNT[n] == len(set(xs)) and all(0 <= x < R for x in xs)
        small = ["zero", "one", "minus one", "on R", "on S", "control"]
        assert sorted({c for c, _ in classes}) == sorted(small + (["short period", "tree twiddle"] if n >= 5 else []))
        assert {0, 1, R - 1, n, n + 1, 2 * n - 1, 2 * n} <= set(xs) and (n < 65 or {64, 65} <= set(xs))
        assert sum(dc.on_roots(n, x) for x in xs) == len({1, n} | ({64, 65} if n >= 65 else set()))
        for c, x in classes:
            if c == "short period":
                assert pow(x, 4, R) == 1 and pow(x, 2, R) != 1
            if c == "tree twiddle":
                size = max(64, 1 << (n - 1).bit_length())
                assert pow(x, size, R) == 1 and pow(x, size // 2, R) == R - 1
                assert n <= size and (size == 64 or size // 2 < n)


def test_class_lists_name_what_they_force(orc):
    """the shapes the table promises, read off the arrays at n = 5"""
    n = 5
    m, l, u, v, w, _ = dc.chain(n)
    inf = lambda a: ~np.asarray(a).any(axis=1)   # noqa: E731
    seen = {}
    for index, (name, x) in enumerate(dc.x_classes(orc, n)):
        arrs = dc.scalar_crs(orc, n, m, l, u, v, w, dc.trapdoor(n, index, x))
        seen.setdefault(name, []).append((x, arrs))
    (_, zero), = seen["zero"]
    assert list(inf(zero["xi_g1"])) == [False] + [True] * (n - 1) and list(inf(zero["xi_t_g1"])) == [False] + [True] * (n - 2)
    (_, one), = seen["one"]
    assert all(np.array_equal(p, one["xi_g1"][0]) for p in one["xi_g1"]) and inf(one["xi_t_g1"]).all()
    (_, minus), = seen["minus one"]
    assert np.array_equal(minus["xi_g1"][0], minus["xi_g1"][2]) and np.array_equal(minus["xi_g1"][1], minus["xi_g1"][3])
    assert not np.array_equal(minus["xi_g1"][0], minus["xi_g1"][1])
    (_, short), = seen["short period"]
    assert np.array_equal(short["xi_g2"][0], short["xi_g2"][4]) and len({p.tobytes() for p in short["xi_g2"][:4]}) == 4
    for x, arrs in seen["on R"]:
        assert inf(arrs["xi_t_g1"]).all() and not inf(arrs["xi_g1"]).any()
    for x, arrs in seen["on S"] + seen["control"] + seen["tree twiddle"]:
        assert not inf(arrs["xi_t_g1"]).any() and not inf(arrs["xi_g1"]).any()


@pytest.mark.parametrize("n", [5, 65])
def test_model_lagrange_arrays_satisfy_the_transpose_identity(orc, grp, n):
    """sum_k k^i lag1[k - 1] == xi_g1[i], the same for lag2, and sum_s s^i lagS_t1[s - n - 1] == xi_t_g1[i]: x^i is its own interpolant
    over n nodes for i <= n - 1, and over the n - 1 nodes of S for i <= n - 2 (xi_t_g1 has n - 1 entries), so the last exponent is
    n - 1 for the roots and n - 2 for S.  On a node the arrays are unit vectors, which the class table relies on."""
    m, l, u, v, w, _ = dc.chain(n)
    inf = lambda a: ~np.asarray(a).any(axis=1)   # noqa: E731
    for index, (name, x) in enumerate(dc.x_classes(orc, n)):
        td = dc.trapdoor(n, index, x)
        arrs = dc.scalar_crs(orc, n, m, l, u, v, w, td)
        lag = ccm.lagrange_arrays(grp, n, td)
        assert lag["lag1"].shape == (n, 8) and lag["lag2"].shape == (n, 16) and lag["lagS_t1"].shape == (n - 1, 8)
        for i in (0, 1, n - 1):
            scalars = ints_to_limbs([pow(k, i, R) for k in range(1, n + 1)])
            assert np.array_equal(orc.msm_g1(lag["lag1"], scalars), arrs["xi_g1"][i]), (name, x, i)
            assert np.array_equal(orc.msm_g2(lag["lag2"], scalars), arrs["xi_g2"][i]), (name, x, i)
        for i in (0, 1, n - 2):
            scalars = ints_to_limbs([pow(s, i, R) for s in range(n + 1, 2 * n)])
            assert np.array_equal(orc.msm_g1(lag["lagS_t1"], scalars), arrs["xi_t_g1"][i]), (name, x, i)
        if dc.on_roots(n, x):
            assert list(np.flatnonzero(~inf(lag["lag1"]))) == [x - 1] and inf(lag["lagS_t1"]).all()
            assert np.array_equal(lag["lag1"][x - 1], orc.enc_base_g1()) and np.array_equal(lag["lag2"][x - 1], orc.enc_base_g2())
        elif name == "on S":
            assert not inf(lag["lag1"]).any() and list(np.flatnonzero(~inf(lag["lagS_t1"]))) == [x - n - 1]
            assert np.array_equal(lag["lagS_t1"][x - n - 1], arrs["xi_t_g1"][0])


@pytest.mark.parametrize("n", [5, 17])
def test_closed_form_is_the_faithful_prover_on_these_trapdoors(orc, n):
    m, l, u, v, w, desc = dc.chain(n)
    du, dv, dw, dt = dense(n)
    classes = dc.x_classes(orc, n)
    assert len(classes) == dc.CLASS_COUNT[n]
    proofs = 0
    for index, (name, x) in enumerate(classes):
        td = dc.trapdoor(n, index, x)
        arrs = dc.scalar_crs(orc, n, m, l, u, v, w, td)
        cdesc = zk.Context.crs_desc(n, m, l, arrs)
        rng = SplitMix64(74000 + 100 * n + index)
        r, s = rng.fr(), rng.fr()
        wits = dc.witnesses(n, x, index)
        assert [g for g, _ in wits] == [None] + sorted({1, n} | ({x} if dc.on_roots(n, x) else set()))
        got = {}
        for gate, wts in wits:
            want = orc.prove_dense(du, dv, dw, dt, l, cdesc, wts, r, s)
            assert isinstance(want, bytes), (name, x, gate, want)
            got[gate] = orc.trapdoor_proof_integers(desc, n, ints_to_limbs(td), wts, r, s)
            assert got[gate] == want, (name, x, gate)
            assert got[gate] == orc.trapdoor_proof_dense(du, dv, dw, dt, l, ints_to_limbs(td), wts, r, s), (name, x, gate)
            proofs += 1
        for gate in got:                      # with t(x) = 0 a gate other than x leaves no trace in the proof
            if gate is not None:
                assert (got[gate] == got[None]) == dc.verdict(n, x, gate), (name, x, gate)
    assert proofs == sum(3 + (1 < x < n) for _, x in classes)
