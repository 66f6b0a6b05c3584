"""zk_crs_contribute and zk_crs_contribution_check on the device (csrc/crs_contribute.hip).  Ground truth is by construction: the
contributed CRS is byte-equal, array by array, to zk_setup's for the trapdoor with delta d in the place of delta; where the sizes
allow the verdict bits of the check are compared with tests/crs_contribute_model.py for the same challenge.  No tolerance anywhere:
bytes and bits only."""
import ctypes as C

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ContributionCheck, SplitMix64, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuits import chain_rows, chain_weights

import crs_check_model as ccm
import crs_contribute_model as cm
from setup_edge_cases import on_domain_trapdoor
from test_circuit_shapes import default_m, shaped_circuit
from test_gpu_crs_check import chain_unity, device_case
from test_integer_roots import chain_rows_integers, chain_weights_integers

pytestmark = pytest.mark.gpu
R = zk.R_MODULUS
TAG = bytes(range(32))


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def rekeyed(td, d):
    """the trapdoor (5, 4) limbs with delta d in the place of delta"""
    t = limbs_to_ints(np.asarray(td).reshape(5, 4))
    t[3] = t[3] * d % R
    return ints_to_limbs(t)


def assert_same_crs(ctx, got, want, tmp_path=None):
    a, b = ctx.crs_download(got), ctx.crs_download(want)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    if tmp_path is not None:          # the container carries the three Lagrange-basis arrays of an integer-roots CRS
        ctx.crs_save(got, tmp_path / "got.crs")
        ctx.crs_save(want, tmp_path / "want.crs")
        assert open(tmp_path / "got.crs", "rb").read() == open(tmp_path / "want.crs", "rb").read()


def contribute_and_compare(ctx, qap, td, seed, tmp_path=None):
    rng = SplitMix64(67000 + seed)
    d, s = rng.fr(), rng.fr()
    src = ctx.setup(qap, td)
    new, rec = ctx.crs_contribute(src, d, TAG)
    assert_same_crs(ctx, new, ctx.setup(qap, rekeyed(td, d)), tmp_path)
    assert rec.verify(TAG) and not rec.verify(None)
    assert np.array_equal(rec.delta_before_g1, ctx.crs_download(src)["delta_g1"])
    res = ctx.crs_contribution_check(src, new, rec, TAG, s)
    assert (res.failed, res.flags, res.ok, res.names) == (0, 0, True, [])
    return src, new, rec, d


# ---- parity with setup -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 4, 13])
def test_parity_roots_of_unity(ctx, log_n):
    """the chain circuit; 2^13 is above the 4096-point switch of crs.hip and spans 32 work-groups of k_g1_scale"""
    qap, td, _ = chain_unity(ctx, log_n, 20 + log_n)
    src, new, rec, d = contribute_and_compare(ctx, qap, td, log_n)
    assert ctx.crs_check(new, qap, SplitMix64(log_n).fr()).ok


@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_parity_integer_roots_with_the_lagrange_arrays(ctx, n, tmp_path):
    m, l, u, v, w = chain_rows_integers(n)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    rng = SplitMix64(67100 + n)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    src, new, rec, d = contribute_and_compare(ctx, qap, td, 100 + n, tmp_path)
    assert open(tmp_path / "got.crs", "rb").read(8) == b"ZKCRSv2\0"
    res = ctx.crs_check(new, qap, rng.fr())
    assert res.ok and res.lagrange_present


@pytest.mark.parametrize("kind,n", [("arbitrary", 4), ("arbitrary", 6), ("dense", 3)])
def test_parity_scattered_roots_and_dense(ctx, orc, kind, n):
    qap, _, _, _, td = device_case(ctx, orc, kind, n)
    src, new, rec, d = contribute_and_compare(ctx, qap, ints_to_limbs(td), 200 + n)
    assert ctx.crs_check(new, qap).ok


@pytest.mark.parametrize("which", ["input=0", "input=m-1"])
def test_parity_at_the_ends_of_input(ctx, which):
    """input = m - 1: sum_delta is empty (k_g1_scale is not launched for it)"""
    log_n = 2
    m, _, u, v, w = chain_rows(log_n)
    l = 0 if which == "input=0" else m - 1
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    rng = SplitMix64(67200 + l)
    src, new, rec, d = contribute_and_compare(ctx, qap, ints_to_limbs([rng.fr() for _ in range(5)]), 300 + l)
    assert ctx.crs_download(new)["sum_delta_g1"].shape[0] == m - l - 1


def test_parity_with_x_on_the_domain(ctx, orc):
    """t(x) = 0: xi_t_g1 is all infinity before and after"""
    log_n = 3
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    src, new, rec, d = contribute_and_compare(ctx, qap, on_domain_trapdoor(orc, log_n, 5), 400)
    assert not ctx.crs_download(new)["xi_t_g1"].any() and ctx.crs_download(new)["sum_delta_g1"].any()


def test_parity_with_zero_columns(ctx):
    """the shaped circuit of tests/test_gpu_circuit_shapes.py: wires no gate uses give infinity entries inside sum_delta_g1"""
    n, L = 1024, 40
    c = shaped_circuit(n, default_m(n, L), L, 100 + n)
    qap = ctx.qap_sparse(10, c["m"], L, c["u"], c["v"], c["w"])
    rng = SplitMix64(67300)
    src, new, rec, d = contribute_and_compare(ctx, qap, ints_to_limbs([rng.fr() for _ in range(5)]), 500)
    sd = ctx.crs_download(new)["sum_delta_g1"]
    inf = ~sd.any(axis=1)
    assert inf.any() and not inf.all()
    assert np.array_equal(inf, ~ctx.crs_download(src)["sum_delta_g1"].any(axis=1))


# ---- chains, d = 1, drawn d ----------------------------------------------------------------------------------------------------------
def test_two_contributions_are_one_setup(ctx):
    qap, td, _ = chain_unity(ctx, 4, 31)
    rng = SplitMix64(67400)
    d1, d2 = rng.fr(), rng.fr()
    c0 = ctx.setup(qap, td)
    c1, r1 = ctx.crs_contribute(c0, d1, TAG)
    tag2 = bytes(r1.to_bytes()[:32])
    c2, r2 = ctx.crs_contribute(c1, d2, tag2)
    assert_same_crs(ctx, c2, ctx.setup(qap, rekeyed(td, d1 * d2 % R)))
    assert np.array_equal(r2.delta_before_g1, r1.delta_after_g1)
    assert ctx.crs_contribution_check(c0, c1, r1, TAG).ok and ctx.crs_contribution_check(c1, c2, r2, tag2).ok
    assert ctx.crs_contribution_check(c0, c2, r2, tag2).failed == ContributionCheck.RECORD      # r2 is not a record of c0 -> c2
    same, rec = ctx.crs_contribute(c0, 1, TAG)
    assert_same_crs(ctx, same, c0)
    assert rec.verify(TAG) and ctx.crs_contribution_check(c0, same, rec, TAG).ok


def test_drawn_d(ctx):
    qap, td, _ = chain_unity(ctx, 4, 32)
    src = ctx.setup(qap, td)
    new, rec = ctx.crs_contribute(src)
    other, rec2 = ctx.crs_contribute(src)
    a, b, c = ctx.crs_download(src), ctx.crs_download(new), ctx.crs_download(other)
    assert not np.array_equal(a["delta_g1"], b["delta_g1"]) and not np.array_equal(b["delta_g1"], c["delta_g1"])
    assert ctx.crs_check(new, qap).ok and ctx.crs_contribution_check(src, new, rec).ok and rec.verify()
    assert ctx.crs_contribution_check(src, other, rec).failed == ContributionCheck.RECORD      # a valid successor, another's record


# ---- proofs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unity", "integers"])
def test_proofs_over_both_crs(ctx, kind, tmp_path):
    import torch
    rng = SplitMix64(67500 + len(kind))
    if kind == "unity":
        log_n = 4
        m, l, u, v, w = chain_rows(log_n)
        qap = ctx.qap_sparse(log_n, m, l, u, v, w)
        wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    else:
        n = 5
        m, l, u, v, w = chain_rows_integers(n)
        qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
        wts = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    d, r, s = rng.fr(), rng.fr(), rng.fr()
    src = ctx.setup(qap, td)
    old_proof = ctx.prove(src, qap, wts, r, s)                   # builds the source's window tables
    dev = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ticket = ctx.prove_submit(src, qap, dev.data_ptr(), m, r, s)
    new, rec = ctx.crs_contribute(src, d, TAG)
    assert ctx.prove_wait(ticket) == old_proof                   # a ticket outstanding across the call
    assert ctx.prove(src, qap, wts, r, s) == old_proof           # the source before == after
    new_proof = ctx.prove(new, qap, wts, r, s)
    assert new_proof == ctx.prove(ctx.setup(qap, rekeyed(td, d)), qap, wts, r, s) and new_proof != old_proof
    inputs = wts[1:1 + l]
    assert ctx.verify(new, inputs, new_proof) and ctx.verify(src, inputs, old_proof)
    assert not ctx.verify(src, inputs, new_proof) and not ctx.verify(new, inputs, old_proof)
    vk = ctx.verifying_key(src)
    assert vk.verify(inputs, old_proof) and not vk.verify(inputs, new_proof)
    # file round trip, both container versions, then prove
    ctx.crs_save(new, tmp_path / "new.crs")
    assert open(tmp_path / "new.crs", "rb").read(8) == (b"ZKCRSv2\0" if kind == "integers" else b"ZKCRSv1\0")
    assert ctx.prove(ctx.crs_load(tmp_path / "new.crs"), qap, wts, r, s) == new_proof
    if kind == "unity":
        n = 1 << 4
        ctx.crs_save(ctx.crs_upload(n, m, l, ctx.crs_download(new)), tmp_path / "up.crs")
        assert ctx.prove(ctx.crs_load(tmp_path / "up.crs"), qap, wts, r, s) == new_proof


# ---- the check ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("unity", 4), ("integers", 5), ("arbitrary", 6), ("dense", 3), ("unity", 1), ("integers", 2)])
def test_every_alteration_gives_the_models_bits(ctx, orc, grp, kind, n):
    qap, src, before, _, td = device_case(ctx, orc, kind, n)
    rng = SplitMix64(67600 + n)
    d, s = rng.fr(), rng.fr()
    new, rec = ctx.crs_contribute(src, d, TAG)
    after = ctx.crs_download(new)
    assert all(np.array_equal(after[k], v) for k, v in cm.successor(grp, before, d).items())
    m, l = before["sum_gamma_g1"].shape[0] + before["sum_delta_g1"].shape[0], before["sum_gamma_g1"].shape[0] - 1
    up = lambda arrs: ctx.crs_upload(n, m, l, arrs)   # noqa: E731
    for ch in (s, rng.fr(), None):
        assert ctx.crs_contribution_check(src, new, rec, TAG, ch).failed == 0
        assert ctx.crs_contribution_check(up(before), up(after), rec, TAG, ch).failed == 0       # however the CRSs arrived
    assert cm.check(grp, before, after, rec, TAG, s) == 0
    for name, b, a, r_, t_, bits in cm.alterations(grp, before, after, rec, TAG, d):
        assert cm.check(grp, b, a, r_, t_, s) == bits, name
        got = ctx.crs_contribution_check(src if b is before else up(b), new if a is after else up(a), r_, t_, s)
        assert got.failed == bits, (name, got)
        assert not got.ok and got.names


def test_alterations_at_2_to_the_13(ctx, orc, grp):
    """by construction: one point of 8191 (the last, in the last work-group) and a whole array by another factor"""
    log_n = 13
    qap, td, (m, l, u, v, w) = chain_unity(ctx, log_n, 41)
    src = ctx.setup(qap, td)
    rng = SplitMix64(67700)
    d, s = rng.fr(), rng.fr()
    new, rec = ctx.crs_contribute(src, d, TAG)
    after = ctx.crs_download(new)
    G = after["xi_g1"][0]
    up = lambda arrs: ctx.crs_upload(1 << log_n, m, l, arrs)   # noqa: E731
    for key, pos, bit in [("sum_delta_g1", 0, ContributionCheck.SUM_DELTA), ("sum_delta_g1", -1, ContributionCheck.SUM_DELTA),
                          ("xi_t_g1", -1, ContributionCheck.XI_T), ("xi_g1", -1, ContributionCheck.UNCHANGED),
                          ("xi_g2", 4097, ContributionCheck.UNCHANGED)]:
        bad = cm.copy_arrs(after)
        bad[key][pos] = grp.add1(bad[key][pos], G) if key != "xi_g2" else grp.add2(bad[key][pos], bad[key][pos])
        assert ctx.crs_contribution_check(src, up(bad), rec, TAG, s).failed == bit, (key, pos)
    bad = cm.copy_arrs(after)
    bad["xi_t_g1"] = ctx.g1_scale_batch(after["xi_t_g1"], 3)
    assert ctx.crs_contribution_check(src, up(bad), rec, TAG, s).failed == ContributionCheck.XI_T
    assert ctx.crs_contribution_check(src, up(after), rec, TAG).ok


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    qap, td, (m, l, u, v, w) = chain_unity(ctx, 2, 51)
    src = ctx.setup(qap, td)
    new, rec = ctx.crs_contribute(src, 5, TAG)
    small, td1, _ = chain_unity(ctx, 1, 52)
    crs_small = ctx.setup(small, td1)
    limbs = lambda x: np.array([(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)   # noqa: E731
    ptr = lambda a: a.ctypes.data_as(_lib.u64p)   # noqa: E731
    one, zero, big = limbs(1), limbs(0), limbs(R)
    ctx2 = zk.Context(0)
    try:
        qap2, td2, _ = chain_unity(ctx2, 2, 51)
        crs2 = ctx2.setup(qap2, td2)
        sentinel = bytes([0xA5]) * 224
        for name, c, k, d, outp, status in [("null ctx", None, src.ptr, ptr(one), True, _lib.ZK_ERR_ARG), ("null crs", ctx.ptr, None, ptr(one), True, _lib.ZK_ERR_ARG),
                                            ("null out", ctx.ptr, src.ptr, ptr(one), False, _lib.ZK_ERR_ARG),
                                            ("crs of another context", ctx.ptr, crs2.ptr, ptr(one), True, _lib.ZK_ERR_ARG),
                                            ("d = 0", ctx.ptr, src.ptr, ptr(zero), True, _lib.ZK_ERR_DIV_BY_ZERO),
                                            ("d = r", ctx.ptr, src.ptr, ptr(big), True, _lib.ZK_ERR_RANGE)]:
            out = C.c_void_p(12345)
            record = _lib.CrsContribution.from_buffer_copy(sentinel)
            assert ctx.lib.zk_crs_contribute(c, k, d, None, C.byref(out) if outp else None, C.byref(record)) == status, name
            assert bytes(bytearray(record)) == sentinel, name
            if outp:
                assert not out.value, name
        out = C.c_void_p(12345)
        assert ctx.lib.zk_crs_contribute(ctx.ptr, src.ptr, ptr(one), None, C.byref(out), None) == _lib.ZK_ERR_ARG and not out.value
        cases = [("null ctx", None, src.ptr, new.ptr, True, ptr(one), _lib.ZK_ERR_ARG), ("null before", ctx.ptr, None, new.ptr, True, ptr(one), _lib.ZK_ERR_ARG),
                 ("null after", ctx.ptr, src.ptr, None, True, ptr(one), _lib.ZK_ERR_ARG), ("null record", ctx.ptr, src.ptr, new.ptr, False, ptr(one), _lib.ZK_ERR_ARG),
                 ("other n", ctx.ptr, crs_small.ptr, new.ptr, True, ptr(one), _lib.ZK_ERR_ARG),
                 ("before of another context", ctx.ptr, crs2.ptr, new.ptr, True, ptr(one), _lib.ZK_ERR_ARG),
                 ("after of another context", ctx.ptr, src.ptr, crs2.ptr, True, ptr(one), _lib.ZK_ERR_ARG),
                 ("challenge 0", ctx.ptr, src.ptr, new.ptr, True, ptr(zero), _lib.ZK_ERR_ARG),
                 ("challenge r", ctx.ptr, src.ptr, new.ptr, True, ptr(big), _lib.ZK_ERR_RANGE)]
        for name, c, b, a, with_rec, ch, status in cases:
            res = _lib.CrsContributionResult(0xA5A5A5A5, 0x5A5A5A5A)
            assert ctx.lib.zk_crs_contribution_check(c, b, a, C.byref(rec.raw) if with_rec else None, None, ch, C.byref(res)) == status, name
            assert (res.failed, res.flags) == (0xA5A5A5A5, 0x5A5A5A5A), name
        assert ctx.lib.zk_crs_contribution_check(ctx.ptr, src.ptr, new.ptr, C.byref(rec.raw), None, ptr(one), None) == _lib.ZK_ERR_ARG
        assert ctx.crs_contribution_check(src, new, rec, TAG, R - 1).ok and ctx.crs_contribution_check(src, new, rec, TAG, 1).ok
    finally:
        del crs2, qap2
        ctx2.close()
