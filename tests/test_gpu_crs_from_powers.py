"""zk_crs_from_powers on the device (csrc/crs_from_powers.hip): the CRS of a circuit derived from a powers-of-tau transcript by group
operations only.  The yardstick is zk_setup as it stood before this call existed -- the derived CRS for a transcript built from a KNOWN
(alpha, beta, x) is byte-equal, array by array, to zk_setup(qap, (alpha, beta, 1, 1, x)) -- and tests/degenerate_crs_cases.scalar_crs
where zk_setup refuses x.  No tolerance anywhere: bytes and bits only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import CrsCheck, SplitMix64, _lib, groth16, ints_to_limbs, limbs_to_int
from zksnark_rs_amd.circuits import chain_rows, chain_weights

import crs_check_model as ccm
import powers_cases as pc
from crs_container import read_v2
from degenerate_crs_cases import scalar_crs
from test_integer_roots import GOLD, chain_rows_integers, chain_weights_integers

pytestmark = pytest.mark.gpu
R = zk.R_MODULUS
TAG = bytes(range(32, 64))
SPLIT = 32          # WP_SPLIT of csrc/crs_from_powers.hip: rows with more entries are summed by a work-group


def test_the_library_exports_the_call():
    """the ABI surface of this feature, by name"""
    lib = _lib.load()
    assert "zk_crs_from_powers" in _lib.SIGNATURES and lib.zk_crs_from_powers is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zkgpu.h")).read()
    assert "int zk_crs_from_powers(zk_ctx* ctx, const zk_qap* qap, const zk_powers_desc* powers, zk_crs** out);" in header


@pytest.fixture(scope="module")
def gens(ctx):
    """the project's generators: xi_g1[0], xi_g2[0] of any zk_setup CRS"""
    m, l, u, v, w = chain_rows(1)
    a = ctx.crs_download(ctx.setup(ctx.qap_sparse(1, m, l, u, v, w), ints_to_limbs([3, 5, 7, 11, 13])))
    return a["xi_g1"][0].copy(), a["xi_g2"][0].copy()


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def zk_code(name):
    return open(os.path.join(GOLD, "zk", name)).read()


def draw(seed, n):
    """(alpha, beta, x): drawn, non-zero, x above 2n so that zk_setup takes it for the integer roots too"""
    rng = SplitMix64(88000 + seed)
    alpha, beta, x = rng.fr(), rng.fr(), rng.fr()
    assert alpha and beta and x > 2 * n
    return alpha, beta, x


def powers_for(ctx, gens, abx, n, extra=0):
    return pc.transcript(ctx.g1_mul_batch, ctx.g2_mul_batch, gens[0], gens[1], abx[0], abx[1], abx[2], n, extra)


def derive(ctx, qap, p):
    return ctx.crs_from_powers(qap, p["tau_g1"], p["tau_g2"], p["alpha_tau_g1"], p["beta_tau_g1"], p["beta_g2"])


def assert_same_arrays(got, want):
    assert sorted(got) == sorted(want)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


def assert_same_crs(ctx, got, want, tmp_path=None):
    assert_same_arrays(ctx.crs_download(got), ctx.crs_download(want))
    if tmp_path is not None:          # the container carries the three Lagrange-basis arrays of an integer-roots CRS
        ctx.crs_save(got, tmp_path / "got.crs")
        ctx.crs_save(want, tmp_path / "want.crs")
        assert open(tmp_path / "got.crs", "rb").read(8) == b"ZKCRSv2\0"
        assert open(tmp_path / "got.crs", "rb").read() == open(tmp_path / "want.crs", "rb").read()


def derive_and_compare(ctx, gens, qap, n, seed, tmp_path=None, abx=None):
    abx = abx or draw(seed, n)
    got = derive(ctx, qap, powers_for(ctx, gens, abx, n))
    assert_same_crs(ctx, got, ctx.setup(qap, pc.trapdoor(*abx)), tmp_path)
    return got, abx


# ---- equality with setup -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 6, 7, 10])
def test_equality_roots_of_unity(ctx, gens, log_n):
    """the chain circuit: n = 2, 4 (rows within one lane), 64, 128, 1024 (x's row of n entries goes to a work-group: the split is 32)"""
    m, l, u, v, w = chain_rows(log_n)
    derive_and_compare(ctx, gens, ctx.qap_sparse(log_n, m, l, u, v, w), 1 << log_n, log_n)


@pytest.mark.parametrize("n", [2, 5, 64, 65, 129, 200, 1025])
def test_equality_integer_roots_with_the_lagrange_arrays(ctx, gens, n, tmp_path):
    """one block, a full block, a one-leaf right child, two levels, and the convolution sizes 4 .. 4096; the saved ZKCRSv2 files --
    lag1, lagS_t1 and lag2 included -- are byte-equal"""
    m, l, u, v, w = chain_rows_integers(n)
    derive_and_compare(ctx, gens, ctx.qap_sparse_integers(n, m, l, u, v, w), n, 100 + n, tmp_path)


def test_one_gate(ctx, gens):
    """n = 1: no xi_t point, one power of each kind"""
    m, l, u, v, w = chain_rows(0)
    derive_and_compare(ctx, gens, ctx.qap_sparse(0, m, l, u, v, w), 1, 1)
    m, l, u, v, w = chain_rows_integers(1)
    derive_and_compare(ctx, gens, ctx.qap_sparse_integers(1, m, l, u, v, w), 1, 2)


# ---- circuit shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple.zk", "deg_15.zk", "lispesque_cubic.zk"])
def test_zk_goldens(ctx, gens, name, tmp_path):
    qap = groth16.QAP.from_zk(ctx, zk_code(name), sparse=True)
    derive_and_compare(ctx, gens, qap.handle, qap.handle.n, 300 + len(name), tmp_path)


EMPTY, CANCELS, TWO, TWICE, FULL, LONG, AGAIN = 10, 11, 12, 13, 14, 15, 16


def shaped_rows(n, m, alpha, beta):
    """(u, v, w) over n gates whose wires 10..16 are the shapes k_wire_points can go wrong on (the others: +1, -1 and a small value)"""
    special = range(EMPTY, AGAIN + 1)
    u = [(i, i % n, 1) for i in range(m) if i not in special]
    v = [(i, (7 * i + 1) % n, -1) for i in range(m) if i not in special]
    w = [(i, (3 * i + 2) % n, 3 + i) for i in range(m) if i not in special]
    # EMPTY: a wire in no gate.  CANCELS: beta 5 L_3 + alpha c L_3 = 0 with c = -5 beta / alpha (a full-width value): the row sums to infinity
    u.append((CANCELS, 3, 5))
    v.append((CANCELS, 3, -5 * beta * pow(alpha, -1, R)))
    w.append((TWO, 2, 2))                                     # one entry of value 2: a doubling inside the short double-and-add
    w += [(TWICE, 5, 1), (TWICE, 5, 1)]                       # the same Lagrange point reached twice: the mixed addition meets P + P
    u += [(FULL, 0, R - 1), (FULL, 1, (R - 1) // 2), (FULL, 2, 1), (FULL, 3, (1 << 200) + 12345), (FULL, 4, -1), (FULL, 5, 1 << 32)]
    w += [(LONG, g, 1) for g in range(n)] + [(LONG, 7, (1 << 253) + 9), (LONG, 9, -77)]        # n + 2 > SPLIT entries, mixed classes
    v += [(LONG, g, -1) for g in range(0, n, 2)]
    w += [(AGAIN, 1, 1), (AGAIN, 2, 1), (AGAIN, 2, -1), (AGAIN, 1, 1)]                        # P1 + P2 - P2 + P1: P + P after cancellation
    u += [(0, g, 1) for g in range(n)]                        # the constant wire: a long row among the public wires
    return tuple(pc.rows_from_triples(m, t) for t in (u, v, w))


@pytest.mark.parametrize("form", ["unity", "integers"])
def test_rows_the_kernel_can_go_wrong_on(ctx, gens, form, tmp_path):
    n, m, l = 64, 80, 2
    assert n + 2 > SPLIT
    abx = draw(400 + len(form), n)
    u, v, w = shaped_rows(n, m, abx[0], abx[1])
    qap = ctx.qap_sparse(6, m, l, u, v, w) if form == "unity" else ctx.qap_sparse_integers(n, m, l, u, v, w)
    got, _ = derive_and_compare(ctx, gens, qap, n, 0, tmp_path if form == "integers" else None, abx)
    sd = ctx.crs_download(got)["sum_delta_g1"]
    inf = ~sd.any(axis=1)
    assert inf[EMPTY - l - 1] and inf[CANCELS - l - 1] and inf.sum() == 2


def test_the_chain_circuit_has_a_long_row():
    """what test_equality_* rely on: x multiplies every gate but the last"""
    m, l, u, v, w = chain_rows(7)
    assert int(u[0][2] - u[0][1]) == 127 > SPLIT


# ---- degenerate transcripts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "minus one", "w^3"])
def test_x_on_the_domain_roots_of_unity(ctx, orc, gens, which):
    """t(x) = 0: every butterfly of the inverse transform meets equal, opposite or vanishing points; xi_t_g1 is all infinity as
    zk_setup's, and zk_crs_check says T_ZERO"""
    log_n = 3
    w3 = limbs_to_int(orc.root_of_unity(log_n))
    x = {"one": 1, "minus one": R - 1, "w^3": pow(w3, 3, R)}[which]
    assert pow(x, 1 << log_n, R) == 1
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    a, b, _ = draw(500, 8)
    got, _ = derive_and_compare(ctx, gens, qap, 8, 0, None, (a, b, x))
    assert not ctx.crs_download(got)["xi_t_g1"].any()
    res = ctx.crs_check(got, qap, 12345)
    assert res.failed == 0 and res.flags & _lib.CRS_CHECK_T_ZERO


@pytest.mark.parametrize("which", ["one", "minus one", "2n"])
def test_x_at_the_edges_integer_roots(ctx, orc, gens, which):
    """x = 1 is a root (zk_setup refuses it: scalar_crs is the yardstick, xi_t all infinity, T_ZERO); x = -1 and x = 2n are accepted by
    zk_setup and compared with it"""
    n = 5
    m, l, u, v, w = chain_rows_integers(n)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    a, b, _ = draw(510, n)
    x = {"one": 1, "minus one": R - 1, "2n": 2 * n}[which]
    if which != "one":
        derive_and_compare(ctx, gens, qap, n, 0, None, (a, b, x))
        return
    got = derive(ctx, qap, powers_for(ctx, gens, (a, b, x), n))
    arrs = ctx.crs_download(got)
    assert_same_arrays(arrs, scalar_crs(orc, n, m, l, u, v, w, [a, b, 1, 1, x]))
    assert not arrs["xi_t_g1"].any()
    res = ctx.crs_check(got, qap, 12345)
    assert res.failed == 0 and res.flags & _lib.CRS_CHECK_T_ZERO


# ---- use -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["unity", "integers"])
def test_the_derived_crs_proves_verifies_and_takes_contributions(ctx, gens, form):
    rng = SplitMix64(88600 + len(form))
    if form == "unity":
        log_n, n = 4, 16
        m, l, u, v, w = chain_rows(log_n)
        qap = ctx.qap_sparse(log_n, m, l, u, v, w)
        wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    else:
        n = 5
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
        wts = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    abx = draw(600 + n, n)
    got = derive(ctx, qap, powers_for(ctx, gens, abx, n))
    want = ctx.setup(qap, pc.trapdoor(*abx))
    r, s = rng.fr(), rng.fr()
    proof = ctx.prove(got, qap, wts, r, s)
    assert proof == ctx.prove(want, qap, wts, r, s)
    assert ctx.verify(got, wts[1:1 + l], proof)
    res = ctx.crs_check(got, qap, rng.fr())
    assert res.failed == 0 and res.ok
    nxt, rec = ctx.crs_contribute(got, rng.fr(), TAG)
    assert ctx.crs_contribution_check(got, nxt, rec, TAG, rng.fr()).failed == 0
    assert ctx.crs_check(nxt, qap, rng.fr()).ok
    assert ctx.verify(nxt, wts[1:1 + l], ctx.prove(nxt, qap, wts, r, s))


def test_setup_from_powers_returns_the_two_sigma_views(ctx, gens):
    qap = groth16.QAP.from_zk(ctx, zk_code("simple.zk"), sparse=True)
    n = qap.handle.n
    abx = draw(700, n)
    s1, s2 = groth16.setup_from_powers(qap, powers_for(ctx, gens, abx, n))
    want = ctx.crs_download(ctx.setup(qap.handle, pc.trapdoor(*abx)))
    assert np.array_equal(s1.sum_delta, want["sum_delta_g1"]) and np.array_equal(s1.xi_t, want["xi_t_g1"])
    assert np.array_equal(s2.xi, want["xi_g2"]) and np.array_equal(s2.gamma, s2.delta) and np.array_equal(s2.delta, want["xi_g2"][0])
    assert groth16.check_setup(qap, (s1, s2), 99).ok


# ---- tampering -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["unity", "integers"])
def test_a_transcript_that_is_no_sequence_of_powers_fails_the_check(ctx, gens, grp, form):
    """the call derives, it does not judge: zk_crs_check on the result names the array"""
    if form == "unity":
        n = 8
        m, l, u, v, w = chain_rows(3)
        qap = ctx.qap_sparse(3, m, l, u, v, w)
    else:
        n = 5
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    p = powers_for(ctx, gens, draw(800 + n, n), n)
    assert ctx.crs_check(derive(ctx, qap, p), qap, 777).failed == 0
    bad = ccm.tampered(grp, p, "tau_g1", n + 1)
    assert ctx.crs_check(derive(ctx, qap, bad), qap, 777).failed == CrsCheck.XI_T
    bad = ccm.tampered(grp, p, "alpha_tau_g1", 1)
    failed = ctx.crs_check(derive(ctx, qap, bad), qap, 777).failed
    assert failed & CrsCheck.WIRES and not failed & ~ccm.WIRE_BITS


# ---- oversized transcript ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["unity", "integers"])
def test_powers_beyond_what_the_circuit_needs_are_ignored(ctx, gens, form, tmp_path):
    if form == "unity":
        n = 4
        m, l, u, v, w = chain_rows(2)
        qap = ctx.qap_sparse(2, m, l, u, v, w)
    else:
        n = 5
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    abx = draw(900 + n, n)
    big = powers_for(ctx, gens, abx, n, extra=3)
    assert big["tau_g1"].shape[0] == 2 * n + 2 and big["tau_g2"].shape[0] == n + 3
    assert_same_crs(ctx, derive(ctx, qap, big), derive(ctx, qap, powers_for(ctx, gens, abx, n)), tmp_path if form == "integers" else None)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, c, q, p, n1, nr, null=None, no_out=False):
    keep = {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in p.items()}
    ptr = {k: (None if k == null else keep[k].ctypes.data_as(_lib.u64p)) for k in keep}
    d = _lib.PowersDesc(n1, nr, ptr["tau_g1"], ptr["tau_g2"], ptr["alpha_tau_g1"], ptr["beta_tau_g1"], ptr["beta_g2"])
    out = C.c_void_p(0xDEAD)
    status = ctx.lib.zk_crs_from_powers(c, q, C.byref(d), None if no_out else C.byref(out))
    return status, out.value


def test_refusals_leave_out_null_and_the_context_usable(ctx, gens, orc):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    from test_verify import twist_point_outside_g2
    n = 4
    m, l, u, v, w = chain_rows(2)
    qap = ctx.qap_sparse(2, m, l, u, v, w)
    rng = SplitMix64(88950)
    wts = chain_weights(2, rng.fr(), [rng.fr() for _ in range(n)])
    abx = draw(950, n)
    p = powers_for(ctx, gens, abx, n)
    good = ctx.setup(qap, pc.trapdoor(*abx))
    r, s = rng.fr(), rng.fr()
    proof = ctx.prove(good, qap, wts, r, s)

    def still_proves():
        assert ctx.prove(good, qap, wts, r, s) == proof
        assert_same_crs(ctx, derive(ctx, qap, p), good)

    def with_point(key, pos, words):
        out = {k: np.array(v, copy=True) for k, v in p.items()}
        out[key].reshape(-1, len(words))[pos] = words
        return out

    n1, nr = 2 * n - 1, n
    P = twist_point_outside_g2(77)
    outside = ints_to_limbs([P[0][0], P[0][1], P[1][0], P[1][1]]).reshape(16)
    off1 = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.uint64)                 # (1, 1): 1 != 1 + 3
    big = np.full(8, 2 ** 64 - 1, np.uint64)                             # both coordinates 2^256 - 1 >= q
    ARG, RANGE, UNSUP = _lib.ZK_ERR_ARG, _lib.ZK_ERR_RANGE, _lib.ZK_ERR_UNSUPPORTED
    cases = [("tau_g1 one short", (ctx.ptr, qap.ptr, p, n1 - 1, nr), ARG), ("the rest one short", (ctx.ptr, qap.ptr, p, n1, nr - 1), ARG),
             ("null ctx", (None, qap.ptr, p, n1, nr), ARG), ("null qap", (ctx.ptr, None, p, n1, nr), ARG)]
    cases += [("null " + k, (ctx.ptr, qap.ptr, p, n1, nr, k), ARG) for k in p]
    cases += [("off the curve: " + k, (ctx.ptr, qap.ptr, with_point(k, pos, off1), n1, nr), RANGE)
              for k, pos in (("tau_g1", 2 * n - 2), ("alpha_tau_g1", 0), ("beta_tau_g1", n - 1))]
    cases += [("coordinate >= q", (ctx.ptr, qap.ptr, with_point("tau_g1", 1, big), n1, nr), RANGE),
              ("tau_g2 outside the subgroup", (ctx.ptr, qap.ptr, with_point("tau_g2", 2, outside), n1, nr), RANGE),
              ("beta_g2 outside the subgroup", (ctx.ptr, qap.ptr, with_point("beta_g2", 0, outside), n1, nr), RANGE)]
    for name, args, status in cases:
        got, out = raw_call(ctx, *args)
        assert (got, out) == (status, None), name
        if got != ARG or "null ctx" != name:
            assert ctx.lib.zk_last_error(ctx.ptr), name
        still_proves()
    assert raw_call(ctx, ctx.ptr, qap.ptr, p, n1, nr, no_out=True)[0] == ARG
    assert ctx.lib.zk_crs_from_powers(ctx.ptr, qap.ptr, None, C.byref(C.c_void_p())) == ARG
    # a point beyond the powers that are read is not looked at
    spare = powers_for(ctx, gens, abx, n, extra=1)
    spare["tau_g1"][2 * n - 1] = off1
    assert_same_crs(ctx, derive(ctx, qap, spare), good)
    # a QAP of another context
    ctx2 = zk.Context(0)
    try:
        qap2 = ctx2.qap_sparse(2, m, l, u, v, w)
        assert raw_call(ctx, ctx.ptr, qap2.ptr, p, n1, nr) == (ARG, None)
        del qap2
    finally:
        ctx2.close()
    still_proves()
    # the two forms that are out of scope
    from test_gpu_crs_check import device_case
    for kind, size in (("arbitrary", 4), ("dense", 3)):
        other = device_case(ctx, orc, kind, size)[0]
        po = powers_for(ctx, gens, abx, other.n)
        got, out = raw_call(ctx, ctx.ptr, other.ptr, po, 2 * other.n - 1, other.n)
        assert (got, out) == (UNSUP, None), kind
        assert b"zk_crs_from_powers" in ctx.lib.zk_last_error(ctx.ptr)
        still_proves()


def test_an_infinity_inside_the_transcript_is_accepted(ctx, gens):
    """the call derives from whatever points it is given; the check then refuses the result"""
    n = 4
    m, l, u, v, w = chain_rows(2)
    qap = ctx.qap_sparse(2, m, l, u, v, w)
    p = powers_for(ctx, gens, draw(960, n), n)
    p["tau_g1"][2] = 0
    p["beta_tau_g1"][1] = 0
    got = derive(ctx, qap, p)
    assert not ctx.crs_download(got)["xi_g1"][2].any()
    assert ctx.crs_check(got, qap, 4242).failed != 0


# ---- isolation -----------------------------------------------------------------------------------------------------------------------
def test_an_outstanding_ticket_is_not_disturbed(ctx, gens):
    import torch
    log_n, n = 4, 16
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    rng = SplitMix64(88970)
    wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    abx = draw(970, n)
    p = powers_for(ctx, gens, abx, n)
    crs = ctx.setup(qap, pc.trapdoor(*abx))
    r, s = rng.fr(), rng.fr()
    before = ctx.prove(crs, qap, wts, r, s)
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ticket = ctx.prove_submit(crs, qap, d.data_ptr(), m, r, s)
    got = derive(ctx, qap, p)
    assert ctx.prove_wait(ticket) == before
    assert ctx.prove(got, qap, wts, r, s) == before


@pytest.mark.parametrize("n", [5, 65])
def test_the_change_of_basis_of_an_uploaded_crs_is_what_it_was(ctx, grp, n, tmp_path):
    """gbasis.hip's other caller: an uploaded integer-roots CRS (powers only) still gets the lag1 / lagS_t1 / lag2 of its trapdoor
    from the transposed tree at its first proof"""
    m, l, u, v, w = chain_rows_integers(n)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    rng = SplitMix64(88980 + n)
    td = [rng.fr() for _ in range(5)]
    up = ctx.crs_upload(n, m, l, ctx.crs_download(ctx.setup(qap, ints_to_limbs(td))))
    wts = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    saved = ctx.get_option("basis_tree_min")
    ctx.set_option("basis_tree_min", 1)           # the tree at every size
    try:
        proof = ctx.prove(up, qap, wts, rng.fr(), rng.fr())
    finally:
        ctx.set_option("basis_tree_min", saved)
    assert ctx.verify(up, wts[1:1 + l], proof)
    ctx.crs_save(up, tmp_path / "up.crs")
    lag = read_v2(tmp_path / "up.crs", n)[2]
    want = ccm.lagrange_arrays(grp, n, td)
    for k in ("lag1", "lagS_t1", "lag2"):
        assert np.array_equal(lag[k], want[k]), k
