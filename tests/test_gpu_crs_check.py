"""zk_crs_check on the device (csrc/crs_check.hip).  Ground truth is by construction: a CRS is good iff it is byte-equal to zk_setup's
for a known trapdoor; every altered CRS below differs from that in a stated way.  Where the sizes allow, the verdict bits are also
compared with tests/crs_check_model.py (oracle group operations, host pairing, Python polynomials) for the same challenge.  No
tolerance anywhere: bits and proof bytes only."""
import ctypes as C
import struct

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import CrsCheck, SplitMix64, _lib, ints_to_limbs, limbs_to_int
from zksnark_rs_amd.circuits import chain_rows, chain_weights

import crs_check_model as ccm
from crs_container import read_v2
from setup_edge_cases import on_domain_trapdoor
from test_crs_check_model import build_case, challenges, tamper_targets
from test_integer_roots import chain_rows_integers, chain_weights_integers

pytestmark = pytest.mark.gpu
R = zk.R_MODULUS


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def upload_qap(ctx, recipe):
    kind, args = recipe
    if kind == "unity":
        return ctx.qap_sparse(*args)
    if kind == "integers":
        return ctx.qap_sparse_integers(*args)
    if kind == "arbitrary":
        return ctx.qap_sparse_roots(*args)
    return ctx.qap_dense(*args)


def device_case(ctx, orc, kind, n, seed=0):
    """the QAP of build_case on the device, zk_setup's CRS for its trapdoor and that CRS's arrays"""
    _, q, td, recipe = build_case(orc, kind, n, seed)
    qap = upload_qap(ctx, recipe)
    crs = ctx.setup(qap, ints_to_limbs(td))
    return qap, crs, ctx.crs_download(crs), q, td


def chain_unity(ctx, log_n, seed):
    m, l, u, v, w = chain_rows(log_n)
    rng = SplitMix64(53000 + seed)
    return ctx.qap_sparse(log_n, m, l, u, v, w), ints_to_limbs([rng.fr() for _ in range(5)]), (m, l, u, v, w)


# ---- the ZKCRSv1 / ZKCRSv2 container, read and rewritten on the host ----------------------------------------------------------------
def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def write_v2(path, dims, payload, lag):
    body = payload + lag["lag1"].tobytes() + lag["lagS_t1"].tobytes() + lag["lag2"].tobytes()
    with open(path, "wb") as f:
        f.write(b"ZKCRSv2\0" + dims + struct.pack("<Q", fnv1a(body)) + body)


# ---- honest CRSs pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 4, 13])
def test_honest_roots_of_unity(ctx, log_n):
    """the chain circuit; 2^13 is above the 4096-point switch of crs.hip and spans several blocks of the power kernel"""
    qap, td, _ = chain_unity(ctx, log_n, log_n)
    res = ctx.crs_check(ctx.setup(qap, td), qap, SplitMix64(log_n).fr())
    assert (res.failed, res.flags) == (0, 0) and res.ok and res.names == []


@pytest.mark.parametrize("n", [1, 2, 3, 5, 17])
def test_honest_integer_roots_with_and_without_lagrange_arrays(ctx, n):
    m, l, u, v, w = chain_rows_integers(n)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    rng = SplitMix64(54000 + n)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    s = rng.fr()
    res = ctx.crs_check(crs, qap, s)
    assert (res.failed, res.flags) == (0, CrsCheck.LAGRANGE_PRESENT) and res.ok and res.lagrange_present
    up = ctx.crs_upload(n, m, l, ctx.crs_download(crs))
    res = ctx.crs_check(up, qap, s)
    assert (res.failed, res.flags) == (0, 0)
    assert ctx.crs_check(up, qap).ok and ctx.crs_check(crs, qap).ok        # challenge drawn from the OS


@pytest.mark.parametrize("kind,n", [("arbitrary", 4), ("arbitrary", 6), ("dense", 3)])
def test_honest_scattered_roots_and_dense_with_a_non_monic_t(ctx, orc, kind, n):
    qap, crs, arrs, q, td = device_case(ctx, orc, kind, n)
    for s in challenges(kind, n):
        res = ctx.crs_check(crs, qap, s)
        assert (res.failed, res.flags) == (0, 0), res
    assert ctx.crs_check(crs, qap).ok


@pytest.mark.parametrize("which", ["input=0", "input=m-1"])
def test_honest_at_the_ends_of_input(ctx, grp, which):
    """input = m - 1: sum_delta is empty; input = 0: sum_gamma is the constant wire alone.  The last sum_gamma point replaced is found."""
    log_n = 2
    m, _, u, v, w = chain_rows(log_n)
    l = 0 if which == "input=0" else m - 1
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    rng = SplitMix64(55000 + l)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    s = rng.fr()
    assert ctx.crs_check(crs, qap, s).failed == 0
    arrs = ctx.crs_download(crs)
    assert arrs["sum_delta_g1"].shape[0] == m - l - 1
    bad = ctx.crs_upload(4, m, l, ccm.tampered(grp, arrs, "sum_gamma_g1", l))
    assert ctx.crs_check(bad, qap, s).failed == CrsCheck.WIRES | CrsCheck.WIRES_GAMMA


def test_honest_from_files_of_both_versions(ctx, tmp_path):
    n = 5
    m, l, u, v, w = chain_rows_integers(n)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    rng = SplitMix64(56000)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    s = rng.fr()
    ctx.crs_save(crs, tmp_path / "two.crs")
    ctx.crs_save(ctx.crs_upload(n, m, l, ctx.crs_download(crs)), tmp_path / "one.crs")
    assert open(tmp_path / "two.crs", "rb").read(8) == b"ZKCRSv2\0" and open(tmp_path / "one.crs", "rb").read(8) == b"ZKCRSv1\0"
    res = ctx.crs_check(ctx.crs_load(tmp_path / "two.crs"), qap, s)
    assert (res.failed, res.flags) == (0, CrsCheck.LAGRANGE_PRESENT)
    res = ctx.crs_check(ctx.crs_load(tmp_path / "one.crs"), qap, s)
    assert (res.failed, res.flags) == (0, 0)


def test_x_on_a_root_is_consistent_and_flagged(ctx, orc):
    log_n = 3
    m, l, u, v, w = chain_rows(log_n)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, on_domain_trapdoor(orc, log_n, 3))
    for s in (SplitMix64(1).fr(), None):
        res = ctx.crs_check(crs, qap, s)
        assert res.failed == 0 and res.flags == CrsCheck.T_ZERO and res.t_zero and not res.ok


# ---- one point replaced by another valid point -----------------------------------------------------------------------------------
TAMPER_SIZES = {"unity": 4, "dense": 4, "integers": 5, "arbitrary": 5}
TAMPER_KEYS = ("xi_g1", "xi_g2", "xi_t_g1", "sum_gamma_g1", "sum_delta_g1", "single points")


@pytest.mark.parametrize("kind", sorted(TAMPER_SIZES))
@pytest.mark.parametrize("key", TAMPER_KEYS)
def test_one_point_replaced(ctx, orc, grp, kind, key):
    """first, middle and last of each array and each of the six single points, through zk_crs_upload: the bit of the array's own
    relation is set, nothing outside the relations that read it, and the bits are the model's.  (An integer-roots CRS that went
    through zk_crs_upload carries no Lagrange-basis arrays; those have the test below.)"""
    n = TAMPER_SIZES[kind]
    qap, crs, arrs, q, td = device_case(ctx, orc, kind, n)
    s = challenges(kind, n)[0]
    targets = [t for t in tamper_targets(arrs, None) if (t[0] == key if key != "single points" else t[1] is None)]
    assert targets
    for k, pos in targets:
        bad = ccm.tampered(grp, arrs, k, pos)
        res = ctx.crs_check(ctx.crs_upload(n, q["m"], q["l"], bad), qap, s)
        required, allowed = ccm.expected_bits(k, pos, n, False)
        assert res.failed and res.failed & required == required and res.failed & ~allowed == 0, (k, pos, res)
        assert (res.failed, res.flags) == ccm.check(grp, bad, q, s), (k, pos, res)
        assert not res.ok


@pytest.mark.parametrize("key", ["lag1", "lagS_t1", "lag2"])
def test_one_lagrange_basis_point_replaced(ctx, orc, grp, key, tmp_path):
    """integer roots, n = 5: a ZKCRSv2 file rewritten with one Lagrange-basis point replaced and its checksum recomputed loads (every
    point is valid) and fails LAGRANGE, nothing else"""
    n = 5
    qap, crs, arrs, q, td = device_case(ctx, orc, "integers", n)
    s = challenges("integers", n)[0]
    path = tmp_path / "crs.v2"
    ctx.crs_save(crs, path)
    dims, payload, lag = read_v2(path, n)
    for name, want in ccm.lagrange_arrays(grp, n, td).items():
        assert np.array_equal(lag[name], want), name
    for pos in ccm.positions(len(lag[key])):
        bad = ccm.tampered(grp, lag, key, pos)
        write_v2(path, dims, payload, bad)
        res = ctx.crs_check(ctx.crs_load(path), qap, s)
        assert (res.failed, res.flags) == (CrsCheck.LAGRANGE, CrsCheck.LAGRANGE_PRESENT), (pos, res)
        assert (res.failed, res.flags) == ccm.check(grp, arrs, q, s, bad)
    write_v2(path, dims, payload, lag)
    assert ctx.crs_check(ctx.crs_load(path), qap, s).ok


# ---- consistent-looking wrong CRSs -----------------------------------------------------------------------------------------------
def with_element(td, pos, value):
    out = list(td)
    out[pos] = value
    return ints_to_limbs(out)


@pytest.mark.parametrize("case", ["xi_t swapped", "sum_delta scaled", "xi_t of another delta", "w differs in one entry", "gamma_g2 of another gamma",
                                  "delta_g1 of another delta"])
def test_wrong_crs_that_looks_consistent(ctx, orc, grp, case):
    kind, n = "arbitrary", 5
    _, q, td, recipe = build_case(orc, kind, n)
    qap = upload_qap(ctx, recipe)
    arrs = ctx.crs_download(ctx.setup(qap, ints_to_limbs(td)))
    bad = {k: v.copy() for k, v in arrs.items()}
    other = SplitMix64(57000).fr()
    if case == "xi_t swapped":
        bad["xi_t_g1"][[1, 2]] = bad["xi_t_g1"][[2, 1]]
        want = CrsCheck.XI_T
    elif case == "sum_delta scaled":
        k = len(bad["sum_delta_g1"])
        bad["sum_delta_g1"] = orc.g1_mul_batch(bad["sum_delta_g1"], np.tile(ints_to_limbs([other]), (k, 1)))
        want = CrsCheck.WIRES | CrsCheck.WIRES_DELTA
    elif case == "xi_t of another delta":
        bad["xi_t_g1"] = ctx.crs_download(ctx.setup(qap, with_element(td, 3, other)))["xi_t_g1"]
        want = CrsCheck.XI_T
    elif case == "w differs in one entry":
        rk, (roots, m, l, u, v, w) = recipe
        ptr, gate, val = w
        assert len(gate)
        val2 = val.copy()
        val2[len(gate) // 2] = ints_to_limbs([(limbs_to_int(val[len(gate) // 2]) + 1) % R])[0]
        bad = ctx.crs_download(ctx.setup(ctx.qap_sparse_roots(roots, m, l, u, v, (ptr, gate, val2)), ints_to_limbs(td)))
        assert sum(not np.array_equal(bad[k], arrs[k]) for k in arrs) == 1      # one of sum_gamma / sum_delta, nothing else
        want = CrsCheck.WIRES
    elif case == "gamma_g2 of another gamma":
        bad["gamma_g2"] = ctx.crs_download(ctx.setup(qap, with_element(td, 2, other)))["gamma_g2"]
        want = CrsCheck.WIRES | CrsCheck.WIRES_GAMMA
    else:
        bad["delta_g1"] = ctx.crs_download(ctx.setup(qap, with_element(td, 3, other)))["delta_g1"]
        want = CrsCheck.TWINS
    up = ctx.crs_upload(n, q["m"], q["l"], bad)
    for s in challenges(kind, n):
        res = ctx.crs_check(up, qap, s)
        if case == "w differs in one entry":
            assert res.failed in (CrsCheck.WIRES | CrsCheck.WIRES_GAMMA, CrsCheck.WIRES | CrsCheck.WIRES_DELTA), res
        else:
            assert res.failed == want, res
        assert (res.failed, res.flags) == ccm.check(grp, bad, q, s)
    assert ctx.crs_check(up, qap).failed == res.failed


def test_the_challenge_enters_with_its_own_power_per_entry(ctx, orc, grp):
    """xi_t[0] += D, xi_t[1] -= D / s: passes with exactly that s, fails with s + 1 and with a drawn challenge -- the counterpart of
    the cancellation pairs of test_gpu_verify_batch_all.py, and the reason the challenge must be secret"""
    log_n = 2
    qap, td, (m, l, u, v, w) = chain_unity(ctx, log_n, 99)
    arrs = ctx.crs_download(ctx.setup(qap, td))
    s = SplitMix64(58000).fr()
    D = grp.mul1(orc.enc_base_g1(), 0xD1FF)
    arrs["xi_t_g1"][0] = grp.add1(arrs["xi_t_g1"][0], D)
    arrs["xi_t_g1"][1] = grp.add1(arrs["xi_t_g1"][1], grp.mul1(D, R - pow(s, -1, R)))
    up = ctx.crs_upload(4, m, l, arrs)
    assert ctx.crs_check(up, qap, s).failed == 0
    assert ctx.crs_check(up, qap, (s + 1) % R).failed == CrsCheck.XI_T
    assert ctx.crs_check(up, qap, None).failed == CrsCheck.XI_T


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(ctx):
    qap, td, (m, l, u, v, w) = chain_unity(ctx, 2, 7)
    crs = ctx.setup(qap, td)
    small, td1, _ = chain_unity(ctx, 1, 8)
    crs_small = ctx.setup(small, td1)
    other_l = ctx.qap_sparse(2, m, l + 1, u, v, w)
    ctx2 = zk.Context(0)
    try:
        qap2, td2, _ = chain_unity(ctx2, 2, 7)
        crs2 = ctx2.setup(qap2, td2)
        one_limbs = np.ascontiguousarray(ints_to_limbs([1])[0])
        one = one_limbs.ctypes.data_as(_lib.u64p)
        limbs = lambda x: np.array([(x >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)   # noqa: E731
        cases = [("null ctx", None, crs.ptr, qap.ptr, one, _lib.ZK_ERR_ARG), ("null crs", ctx.ptr, None, qap.ptr, one, _lib.ZK_ERR_ARG),
                 ("null qap", ctx.ptr, crs.ptr, None, one, _lib.ZK_ERR_ARG),
                 ("other n", ctx.ptr, crs_small.ptr, qap.ptr, one, _lib.ZK_ERR_ARG), ("other input", ctx.ptr, crs.ptr, other_l.ptr, one, _lib.ZK_ERR_ARG),
                 ("crs of another context", ctx.ptr, crs2.ptr, qap.ptr, one, _lib.ZK_ERR_ARG),
                 ("qap of another context", ctx.ptr, crs.ptr, qap2.ptr, one, _lib.ZK_ERR_ARG)]
        for name, value, status in [("challenge 0", 0, _lib.ZK_ERR_ARG), ("challenge r", R, _lib.ZK_ERR_RANGE), ("challenge 2^256-1", 2 ** 256 - 1, _lib.ZK_ERR_RANGE)]:
            arr = limbs(value)
            cases.append((name, ctx.ptr, crs.ptr, qap.ptr, arr.ctypes.data_as(_lib.u64p), status))
            cases[-1] += (arr,)
        for case in cases:
            name, c, k, q, ch, status = case[:6]
            out = _lib.CrsCheckResult(0xA5A5A5A5, 0x5A5A5A5A)
            assert ctx.lib.zk_crs_check(c, k, q, ch, C.byref(out)) == status, name
            assert (out.failed, out.flags) == (0xA5A5A5A5, 0x5A5A5A5A), name
        assert ctx.lib.zk_crs_check(ctx.ptr, crs.ptr, qap.ptr, one, None) == _lib.ZK_ERR_ARG
        assert ctx.crs_check(crs, qap, R - 1).ok and ctx.crs_check(crs, qap, 1).failed == 0      # the ends of the range are accepted
    finally:
        del crs2, qap2
        ctx2.close()


# ---- read-only -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unity", "integers"])
def test_a_check_changes_no_proof(ctx, kind):
    """proof bytes before == after a check on the same handles, with a CRS that has its prover tables (built by the first proof) and
    with a fresh one; a zk_prove_submit ticket outstanding across a check gives the same bytes"""
    import torch
    rng = SplitMix64(59000 + len(kind))
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
    r, s = rng.fr(), rng.fr()
    crs = ctx.setup(qap, td)
    before = ctx.prove(crs, qap, wts, r, s)
    assert ctx.crs_check(crs, qap).ok
    assert ctx.prove(crs, qap, wts, r, s) == before
    fresh = ctx.setup(qap, td)
    assert ctx.crs_check(fresh, qap).ok               # before any proof: the check builds no prover table
    assert ctx.prove(fresh, qap, wts, r, s) == before
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ticket = ctx.prove_submit(crs, qap, d.data_ptr(), m, r, s)
    assert ctx.crs_check(crs, qap).ok
    assert ctx.prove_wait(ticket) == before
    assert ctx.verify(crs, wts[1:1 + l], before)
