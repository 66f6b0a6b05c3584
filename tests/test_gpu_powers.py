"""-m gpu: phase 1 of a setup -- the resident powers-of-tau transcript (zk_powers_*): a contribution is byte for byte the transcript
tests/powers_cases.py builds from the products of the scalars; zk_powers_check and zk_powers_contribution_check answer, for a fixed
challenge, exactly the bits of the exponent model (tests/powers_check_model.py) on good transcripts and on every alteration; the
inputs are read only; and a ceremony from zk_powers_initial runs through to a verified proof."""
import ctypes as C
import os

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import PowersCheck, PowersContribution, SplitMix64, ZkError, _lib, groth16, ints_to_limbs
from zksnark_rs_amd.circuits import chain_rows, chain_weights

import powers_cases as pc
import powers_check_model as pm
from crs_contribute_model import LAMBDA
from test_integer_roots import chain_rows_integers, chain_weights_integers

pytestmark = pytest.mark.gpu
R = zk.R_MODULUS
TAG = bytes(range(64, 96))
CHALLENGE = 0x1d2c3b4a5968778695a4b3c2d1e0f
# (N1, N2): the smallest, odd sizes, around one and four waves of points, N1 = N2, and N1 > 2 N2
SHAPES = [(2, 2), (3, 2), (5, 3), (127, 64), (129, 65), (511, 256), (513, 257), (300, 300), (40, 7)]
B = pm.BIT


def test_the_library_exports_the_calls():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zkgpu.h")).read()
    for name in ("zk_powers_upload", "zk_powers_initial", "zk_powers_dims", "zk_powers_download", "zk_powers_free", "zk_powers_check",
                 "zk_powers_contribute", "zk_powers_contribution_check", "zk_powers_contribution_prove", "zk_powers_contribution_verify"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header, name


@pytest.fixture(scope="module")
def gens(ctx):
    """the project's generators: xi_g1[0], xi_g2[0] of any zk_setup CRS"""
    m, l, u, v, w = chain_rows(1)
    a = ctx.crs_download(ctx.setup(ctx.qap_sparse(1, m, l, u, v, w), ints_to_limbs([3, 5, 7, 11, 13])))
    return a["xi_g1"][0].copy(), a["xi_g2"][0].copy()


@pytest.fixture(autouse=True)
def default_form(ctx):
    ctx.set_option("powers_mul_form", 0)
    ctx.set_option("powers_mul_ppl", 0)
    yield
    ctx.set_option("powers_mul_form", 0)
    ctx.set_option("powers_mul_ppl", 0)


def draw(seed):
    rng = SplitMix64(95000 + seed)
    return rng.fr(), rng.fr(), rng.fr()


def transcript(ctx, gens, alpha, beta, x, n1, n2):
    """powers_cases.transcript for N1 = 2n - 1 + extra, N2 = n + extra"""
    n = n1 - n2 + 1
    return pc.transcript(ctx.g1_mul_batch, ctx.g2_mul_batch, gens[0], gens[1], alpha, beta, x, n, 2 * n2 - n1 - 1)


def points_of(ctx, gens, e):
    """the points of a dict of exponents (powers_check_model's form); exponent 0 = infinity"""
    rep1 = lambda ks: ctx.g1_mul_batch(np.tile(gens[0], (len(ks), 1)), ints_to_limbs(ks))   # noqa: E731
    rep2 = lambda ks: ctx.g2_mul_batch(np.tile(gens[1], (len(ks), 1)), ints_to_limbs(ks))   # noqa: E731
    return dict(tau_g1=rep1(e["tau_g1"]), tau_g2=rep2(e["tau_g2"]), alpha_tau_g1=rep1(e["alpha_tau_g1"]), beta_tau_g1=rep1(e["beta_tau_g1"]),
                beta_g2=rep2([e["beta_g2"]])[0])


def upload(ctx, t):
    return ctx.powers_upload(t["tau_g1"], t["tau_g2"], t["alpha_tau_g1"], t["beta_tau_g1"], t["beta_g2"])


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


# ---- a contribution is the transcript of the products -------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_a_contribution_is_the_transcript_of_the_products(ctx, gens, n1, n2):
    alpha, beta, x = draw(n1)
    s, a, b = draw(1000 + n1)
    t = transcript(ctx, gens, alpha, beta, x, n1, n2)
    before = upload(ctx, t)
    assert (before.n_tau_g1, before.n_rest) == (n1, n2)
    same(ctx.powers_download(before), t)
    after, rec = ctx.powers_contribute(before, (s, a, b), TAG)
    same(ctx.powers_download(after), transcript(ctx, gens, alpha * a % R, beta * b % R, x * s % R, n1, n2))
    same(ctx.powers_download(before), t)                                           # the source is read only
    drawn = SplitMix64(96000 + n1).fr()
    for h in (before, after):
        assert ctx.powers_check(h, CHALLENGE).failed == 0 and ctx.powers_check(h, drawn).failed == 0
    assert ctx.powers_check(after).ok                                              # a challenge from the OS
    assert ctx.powers_contribution_check(before, after, rec, TAG, CHALLENGE).failed == 0
    assert ctx.powers_contribution_check(before, after, rec, TAG).ok
    same(ctx.powers_download(before), t)
    assert rec.verify(TAG) and not rec.verify(None)
    assert np.array_equal(rec.tau.delta_before_g1, t["tau_g1"][1]) and np.array_equal(rec.alpha.delta_before_g1, t["alpha_tau_g1"][0])
    for key, value in (("powers_mul_ppl", 4), ("powers_mul_ppl", 2), ("powers_mul_form", 1)):
        ctx.set_option(key, value)           # four and two points a lane (what long arrays take), then the comparator kernel: the same bytes
        other, _ = ctx.powers_contribute(before, (s, a, b), TAG)
        same(ctx.powers_download(other), ctx.powers_download(after))
        ctx.set_option(key, 0)


SECRETS = {"ones": (1, 1, 1), "s=r-1": (R - 1, 3, 5), "s=2": (2, 3, 5), "s=lambda": (LAMBDA, 3, 5), "a=r-1": (7, R - 1, 5),
           "b=(r-1)/2": (7, 3, (R - 1) // 2)}


@pytest.mark.parametrize("name", list(SECRETS))
def test_secrets_at_their_edges(ctx, gens, name):
    n1, n2 = 129, 65
    s, a, b = SECRETS[name]
    alpha, beta, x = draw(2000)
    t = transcript(ctx, gens, alpha, beta, x, n1, n2)
    before = upload(ctx, t)
    after, rec = ctx.powers_contribute(before, (s, a, b), TAG)
    got = ctx.powers_download(after)
    same(got, transcript(ctx, gens, alpha * a % R, beta * b % R, x * s % R, n1, n2))
    if name == "ones":
        same(got, t)                                                               # (1, 1, 1) gives an equal transcript
    assert ctx.powers_contribution_check(before, after, rec, TAG, CHALLENGE).failed == 0


def test_two_contributions_chained_equal_one_with_the_products(ctx, gens):
    n1, n2 = 40, 7
    alpha, beta, x = draw(3000)
    (s1, a1, b1), (s2, a2, b2) = draw(3001), draw(3002)
    before = upload(ctx, transcript(ctx, gens, alpha, beta, x, n1, n2))
    mid, rec1 = ctx.powers_contribute(before, (s1, a1, b1), TAG)
    end, rec2 = ctx.powers_contribute(mid, (s2, a2, b2), TAG)
    once, _ = ctx.powers_contribute(before, (s1 * s2 % R, a1 * a2 % R, b1 * b2 % R), TAG)
    same(ctx.powers_download(end), ctx.powers_download(once))
    assert ctx.powers_contribution_check(before, mid, rec1, TAG, CHALLENGE).failed == 0
    assert ctx.powers_contribution_check(mid, end, rec2, TAG, CHALLENGE).failed == 0


@pytest.mark.parametrize("n1,n2", [(5, 3), (129, 65)])
def test_a_contribution_over_the_initial_transcript(ctx, gens, n1, n2):
    head = ctx.powers_initial(n1, n2)
    got = ctx.powers_download(head)
    assert all(np.array_equal(p, gens[0]) for k in ("tau_g1", "alpha_tau_g1", "beta_tau_g1") for p in got[k])
    assert all(np.array_equal(p, gens[1]) for p in got["tau_g2"]) and np.array_equal(got["beta_g2"], gens[1])
    assert ctx.powers_check(head, CHALLENGE).failed == 0
    s, a, b = draw(4000 + n1)
    after, rec = ctx.powers_contribute(head, (s, a, b), TAG)
    same(ctx.powers_download(after), transcript(ctx, gens, a, b, s, n1, n2))       # the transcript of (a, b, s) itself
    assert ctx.powers_contribution_check(head, after, rec, TAG, CHALLENGE).failed == 0


def test_secrets_from_the_os_are_not_returned_and_differ(ctx, gens):
    head = ctx.powers_initial(9, 4)
    one, rec1 = ctx.powers_contribute(head, None, TAG)
    two, rec2 = ctx.powers_contribute(head, None, TAG)
    assert not np.array_equal(ctx.powers_download(one)["tau_g1"][1], ctx.powers_download(two)["tau_g1"][1])
    assert ctx.powers_contribution_check(head, one, rec1, TAG).ok and ctx.powers_contribution_check(head, two, rec2, TAG).ok
    assert ctx.powers_contribution_check(head, one, rec2, TAG, CHALLENGE).failed == B["RECORD"]   # a record from another pair


def test_infinity_entries_pass_through_and_are_flagged(ctx, gens):
    """x = 0: tau[k] is infinity for k >= 1.  The upload accepts it, a contribution leaves infinities infinities, every pairing
    relation still holds, and both checks say DEGENERATE (no proof of knowledge exists over an infinity: KNOWLEDGE as well)"""
    n1, n2 = 9, 4
    alpha, beta, _ = draw(5000)
    e = pm.exponents(alpha, beta, 0, n1, n2)
    t = points_of(ctx, gens, e)
    assert not t["tau_g1"][1:].any() and not t["tau_g2"][1:].any()
    before = upload(ctx, t)
    assert ctx.powers_check(before, CHALLENGE).failed == pm.check(e, CHALLENGE) == B["DEGENERATE"]
    after, rec = ctx.powers_contribute(before, (5, 6, 7), TAG)
    got = ctx.powers_download(after)
    e2, _ = pm.contributed(e, 5, 6, 7)
    same(got, points_of(ctx, gens, e2))
    assert not got["tau_g1"][1:].any()
    assert ctx.powers_check(after, CHALLENGE).failed == B["DEGENERATE"]
    want = pm.check_contribution(e, e2, pm.record_points(e), pm.record_points(e2), False, CHALLENGE)
    assert want == B["DEGENERATE"] | B["KNOWLEDGE"]
    assert ctx.powers_contribution_check(before, after, rec, TAG, CHALLENGE).failed == want


# ---- alterations: the device's bits are the model's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(9, 4), (129, 65), (12, 12)])
def test_every_alteration_sets_the_models_bits(ctx, gens, n1, n2):
    alpha, beta, x = draw(6000 + n1)
    e = pm.exponents(alpha, beta, x, n1, n2)
    assert ctx.powers_check(upload(ctx, points_of(ctx, gens, e)), CHALLENGE).failed == 0
    seen = 0
    for name, bad, bits in pm.alterations(e):
        assert pm.check(bad, CHALLENGE) == bits, name
        got = ctx.powers_check(upload(ctx, points_of(ctx, gens, bad)), CHALLENGE)
        assert got.failed == bits, (name, got)
        seen |= bits
    assert seen == sum(B[k] for k in ("GENERATORS", "POWERS_G1", "POWERS_G2", "ALPHA", "BETA", "BETA_TWINS"))
    assert PowersCheck(B["ALPHA"] | B["BETA_TWINS"]).names == ["ALPHA", "BETA_TWINS"]


def test_the_contribution_check_names_what_is_wrong(ctx, gens):
    n1, n2 = 40, 7
    alpha, beta, x = draw(7000)
    s, a, b = draw(7001)
    e = pm.exponents(alpha, beta, x, n1, n2)
    e2, _ = pm.contributed(e, s, a, b)
    before = upload(ctx, points_of(ctx, gens, e))
    after, rec = ctx.powers_contribute(before, (s, a, b), TAG)
    check = lambda bf, af, r, tag=TAG: ctx.powers_contribution_check(bf, af, r, tag, CHALLENGE).failed   # noqa: E731
    assert check(before, after, rec) == 0
    # a record from another pair
    other_after, other_rec = ctx.powers_contribute(before, draw(7002), TAG)
    assert check(before, after, other_rec) == B["RECORD"]
    assert check(before, other_after, other_rec) == 0
    # an altered response, a wrong tag
    raw = bytearray(rec.to_bytes())
    raw[2 * 224 + 200] ^= 1                                                        # a response word of the beta part
    assert check(before, after, PowersContribution.from_bytes(bytes(raw))) == B["KNOWLEDGE"]
    assert check(before, after, rec, bytes(32)) == B["KNOWLEDGE"]
    assert check(before, after, rec, None) == B["KNOWLEDGE"]
    # parts in each other's roles: the points no longer match and no part verifies under another role's tag
    parts = [rec.to_bytes()[224 * i:224 * (i + 1)] for i in range(3)]
    assert check(before, after, PowersContribution.from_bytes(parts[1] + parts[0] + parts[2])) == B["RECORD"] | B["KNOWLEDGE"]
    # an `after` with one altered entry: the check names its array
    bad = {k: (list(v) if isinstance(v, list) else v) for k, v in e2.items()}
    bad["alpha_tau_g1"][3] = (bad["alpha_tau_g1"][3] + 1) % R
    assert check(before, upload(ctx, points_of(ctx, gens, bad)), rec) == B["ALPHA"] == pm.check(bad, CHALLENGE)
    bad = {k: (list(v) if isinstance(v, list) else v) for k, v in e2.items()}
    bad["tau_g1"][n1 - 1] = (bad["tau_g1"][n1 - 1] + 1) % R
    assert check(before, upload(ctx, points_of(ctx, gens, bad)), rec) == B["POWERS_G1"]
    # before and after swapped: both are transcripts, but the record runs the other way
    assert check(after, before, rec) == B["RECORD"] == pm.check_contribution(e2, e, pm.record_points(e), pm.record_points(e2), True, CHALLENGE)


# ---- statuses ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, gens):
    lib = _lib.load()
    t = transcript(ctx, gens, 3, 5, 7, 5, 3)
    good = upload(ctx, t)
    code = lambda fn: pytest.raises(ZkError, fn).value.status   # noqa: E731
    # shapes: n_rest >= 2, n_tau_g1 >= n_rest
    assert code(lambda: ctx.powers_initial(1, 1)) == _lib.ZK_ERR_ARG
    assert code(lambda: ctx.powers_initial(2, 3)) == _lib.ZK_ERR_ARG
    assert code(lambda: ctx.powers_upload(t["tau_g1"][:2], t["tau_g2"], t["alpha_tau_g1"], t["beta_tau_g1"], t["beta_g2"])) == _lib.ZK_ERR_ARG
    assert code(lambda: ctx.powers_upload(t["tau_g1"], t["tau_g2"][:1], t["alpha_tau_g1"][:1], t["beta_tau_g1"][:1], t["beta_g2"])) == _lib.ZK_ERR_ARG
    # range and curve
    off = t["alpha_tau_g1"].copy()
    off[1, 4] ^= 1
    assert code(lambda: ctx.powers_upload(t["tau_g1"], t["tau_g2"], off, t["beta_tau_g1"], t["beta_g2"])) == _lib.ZK_ERR_RANGE
    big = t["tau_g1"].copy()
    big[4, :4] = ints_to_limbs([zk.Q_MODULUS]).reshape(4)
    assert code(lambda: ctx.powers_upload(big, t["tau_g2"], t["alpha_tau_g1"], t["beta_tau_g1"], t["beta_g2"])) == _lib.ZK_ERR_RANGE
    from test_verify import twist_point_outside_g2
    out2 = t["tau_g2"].copy()
    P = twist_point_outside_g2(78)
    out2[2] = ints_to_limbs([P[0][0], P[0][1], P[1][0], P[1][1]]).reshape(16)
    assert code(lambda: ctx.powers_upload(t["tau_g1"], out2, t["alpha_tau_g1"], t["beta_tau_g1"], t["beta_g2"])) == _lib.ZK_ERR_RANGE
    # secrets and challenges
    assert code(lambda: ctx.powers_contribute(good, (0, 1, 1))) == _lib.ZK_ERR_DIV_BY_ZERO
    assert code(lambda: ctx.powers_contribute(good, (1, 1, 0))) == _lib.ZK_ERR_DIV_BY_ZERO
    assert code(lambda: ctx.powers_contribute(good, (1, R, 1))) == _lib.ZK_ERR_RANGE
    assert code(lambda: ctx.powers_check(good, 0)) == _lib.ZK_ERR_ARG
    assert code(lambda: ctx.powers_check(good, R)) == _lib.ZK_ERR_RANGE
    after, rec = ctx.powers_contribute(good, (2, 3, 4))
    assert code(lambda: ctx.powers_contribution_check(good, after, rec, None, 0)) == _lib.ZK_ERR_ARG
    assert code(lambda: ctx.powers_contribution_check(good, after, rec, None, R + 5)) == _lib.ZK_ERR_RANGE
    assert code(lambda: ctx.powers_contribution_check(good, ctx.powers_initial(6, 3), rec)) == _lib.ZK_ERR_ARG     # different dims
    # null pointers; *out NULL and *record untouched on failure
    p, r_ = C.c_void_p(0x1234), _lib.PowersContribution()
    untouched = bytes(bytearray(r_))
    zero = np.zeros(12, np.uint64)
    assert lib.zk_powers_contribute(ctx.ptr, good.ptr, zero.ctypes.data_as(_lib.u64p), None, C.byref(p), C.byref(r_)) == _lib.ZK_ERR_DIV_BY_ZERO
    assert p.value is None and bytes(bytearray(r_)) == untouched
    assert lib.zk_powers_contribute(ctx.ptr, None, None, None, C.byref(p), C.byref(r_)) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_contribute(ctx.ptr, good.ptr, None, None, C.byref(p), None) == _lib.ZK_ERR_ARG
    res = _lib.PowersCheckResult(0xAAAAAAAA, 0xBBBBBBBB)
    assert lib.zk_powers_check(ctx.ptr, None, None, C.byref(res)) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_check(ctx.ptr, good.ptr, zero.ctypes.data_as(_lib.u64p), C.byref(res)) == _lib.ZK_ERR_ARG
    assert (res.failed, res.flags) == (0xAAAAAAAA, 0xBBBBBBBB)                      # untouched on error
    assert lib.zk_powers_dims(None, None, None) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_download(ctx.ptr, good.ptr, None) == _lib.ZK_ERR_ARG
    # download into chosen buffers only
    only = np.zeros(16, np.uint64)
    out = _lib.PowersOut(None, None, None, None, only.ctypes.data_as(_lib.u64p))
    assert lib.zk_powers_download(ctx.ptr, good.ptr, C.byref(out)) == 0 and np.array_equal(only, t["beta_g2"])
    lib.zk_powers_free(None)
    assert ctx.powers_check(good, CHALLENGE).failed == 0                            # the context and the handle are still usable


def test_a_handle_of_another_context_is_refused(ctx, gens):
    other = zk.Context(0)
    try:
        mine, theirs = ctx.powers_initial(5, 3), other.powers_initial(5, 3)
        code = lambda fn: pytest.raises(ZkError, fn).value.status   # noqa: E731
        assert code(lambda: ctx.powers_check(theirs, CHALLENGE)) == _lib.ZK_ERR_ARG
        assert code(lambda: ctx.powers_contribute(theirs, (2, 3, 4))) == _lib.ZK_ERR_ARG
        after, rec = ctx.powers_contribute(mine, (2, 3, 4))
        assert code(lambda: ctx.powers_contribution_check(theirs, after, rec)) == _lib.ZK_ERR_ARG
        theirs.close()
    finally:
        other.close()


# ---- isolation, end to end -----------------------------------------------------------------------------------------------------------
def test_an_outstanding_ticket_is_not_disturbed(ctx, gens):
    import torch
    log_n, n = 4, 16
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    rng = SplitMix64(98000)
    wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    r, s = rng.fr(), rng.fr()
    expected = ctx.prove(crs, qap, wts, r, s)
    t = transcript(ctx, gens, 3, 5, 7, 129, 65)
    before = upload(ctx, t)
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ticket = ctx.prove_submit(crs, qap, d.data_ptr(), m, r, s)
    after, rec = ctx.powers_contribute(before, (11, 12, 13), TAG)
    assert ctx.powers_check(after, CHALLENGE).failed == 0
    assert ctx.powers_contribution_check(before, after, rec, TAG, CHALLENGE).failed == 0
    assert ctx.prove_wait(ticket) == expected
    same(ctx.powers_download(before), t)


@pytest.mark.parametrize("form", ["integers", "unity"])
def test_a_ceremony_from_the_initial_transcript_to_a_verified_proof(ctx, form):
    rng = SplitMix64(99000 + len(form))
    if form == "unity":
        log_n, n = 4, 16
        m, l, u, v, w = chain_rows(log_n)
        qap = groth16.QAP(ctx, ctx.qap_sparse(log_n, m, l, u, v, w))
        wts = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    else:
        n = 8
        m, l, u, v, w = chain_rows_integers(n)
        qap = groth16.QAP(ctx, ctx.qap_sparse_integers(n, m, l, u, v, w))
        wts = chain_weights_integers(n, rng.fr(), [rng.fr() for _ in range(n)])
    powers = ctx.powers_initial(2 * n - 1, n)
    for party in range(2):                                                          # nobody fixes the secrets
        tag = bytes([party]) * 32
        nxt, rec = groth16.contribute_powers(powers, tag=tag)
        assert groth16.check_powers_contribution(powers, nxt, rec, tag).ok
        powers = nxt
    assert groth16.check_powers(powers).ok
    sigma = groth16.setup_from_powers(qap, powers)                                  # the handle itself: downloaded
    assert groth16.check_setup(qap, sigma).ok
    sigma2, drec = groth16.contribute(sigma, tag=TAG)
    assert groth16.check_contribution(sigma, sigma2, drec, TAG).ok
    proof = groth16.prove(qap, sigma2, wts)
    assert groth16.verify(sigma2, wts[1:1 + l], proof)
    assert not groth16.verify(sigma, wts[1:1 + l], proof)
