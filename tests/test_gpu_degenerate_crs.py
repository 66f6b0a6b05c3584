"""The change of basis of an uploaded CRS (csrc/basis.hip: n^2 inner products; csrc/gbasis.hip: the transposed interpolation tree over
curve points) on the CRSs of tests/degenerate_crs_cases.py, which zk_setup cannot make for an integer-roots QAP: powers [x^i] that
are all one point, alternate between P and -P, repeat with a short period, cancel under the tree's own inverse transform or are
infinity from the second on, and x on a node of either node set.  These reach add_lazy's doubling and P + (-P) branches between
operands with Z != 1, madd_lazy's `false` inside k_gb_bottom, gb_mul and jac_to_affine of infinity, and grouped MSMs whose bases are
one repeated point.

References: the oracle's closed form from the trapdoor for proof bytes, crs_check_model.lagrange_arrays for the derived arrays, and
scalar_crs for the contributed CRS; tests/test_degenerate_crs.py ties all three to the faithful oracle on these trapdoors.  Equality
of words and of bytes only."""
import numpy as np
import pytest

from zksnark_rs_amd import CrsCheck, SplitMix64, ints_to_limbs

import crs_check_model as ccm
import degenerate_crs_cases as dc
from crs_container import read_v2

pytestmark = pytest.mark.gpu
FORMS = (("tree", 1), ("squares", 1 << 30))      # option basis_tree_min: gbasis.hip at every size, basis.hip at every size
TAG = bytes(range(32, 64))


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def to_device(wts):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(wts).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


def assert_lagrange(path, n, want, what):
    _, _, lag = read_v2(path, n)
    for key in ("lag1", "lagS_t1", "lag2"):
        assert lag[key].shape == want[key].shape and np.array_equal(lag[key], want[key]), what + (key,)


def check_class(ctx, orc, grp, tmp_path, n, circuit, qap, index, name, x):
    """one trapdoor through both device forms -> (uploads checked, batches run, contributions run)"""
    m, l, u, v, w, desc = circuit
    td = dc.trapdoor(n, index, x)
    tdl = ints_to_limbs(td)
    arrs = dc.scalar_crs(orc, n, m, l, u, v, w, td)
    lag = ccm.lagrange_arrays(grp, n, td)
    rng = SplitMix64(75000 + 100 * n + index)
    r, s, challenge = rng.fr(), rng.fr(), rng.fr()
    wits = dc.witnesses(n, x, index)
    want = [orc.trapdoor_proof_integers(desc, n, tdl, wts, r, s) for _, wts in wits]
    verdicts = [dc.verdict(n, x, gate) for gate, _ in wits]
    assert verdicts[0] and verdicts.count(False) == (1 if dc.on_roots(n, x) else len(wits) - 1)
    pub = [wts[1:1 + l] for _, wts in wits]
    containers, batches, contributions = {}, 0, 0
    for form, tree_min in FORMS:
        what = (name, x, form)
        ctx.set_option("basis_tree_min", tree_min)
        up = ctx.crs_upload(n, m, l, arrs)
        # 1. proofs (the first one derives the three arrays), 2. single verdicts
        for (gate, wts), wp, ok, p in zip(wits, want, verdicts, pub):
            assert ctx.prove(up, qap, wts, r, s) == wp, what + (gate,)
            assert ctx.verify(up, p, wp) == ok, what + (gate,)
        # 4. the derived arrays, as the container carries them
        path = tmp_path / ("%d_%s.zkcrs" % (index, form))
        ctx.crs_save(up, path)
        assert_lagrange(path, n, lag, what)
        containers[form] = path.read_bytes()
        # 5. zk_crs_check: its own device code over the same arrays
        res = ctx.crs_check(up, qap, challenge)
        assert res.failed == 0, what + (res,)
        assert res.flags == CrsCheck.LAGRANGE_PRESENT | (CrsCheck.T_ZERO if dc.on_roots(n, x) else 0), what + (res,)
        if x == 1:
            # 3. one batch of verdicts and one batch of three proofs over this CRS
            assert list(ctx.verify_batch(up, np.stack(pub), want)) == verdicts, what
            dev = [to_device(wts) for _, wts in wits[:3]]
            t = ctx.prove_batch_submit(up, qap, [d.data_ptr() for d in dev], [m] * 3, [r] * 3, [s] * 3)
            assert ctx.prove_batch_wait(t, 3) == want[:3], what
            batches += 1
        if x in (1, n + 1) and form == "tree":
            # 6. k_g1_scale over an all-infinity xi_t_g1 | lagS_t1 (x = 1) and over a unit-vector lagS_t1 (x = n + 1)
            new, rec = ctx.crs_contribute(up, dc.CONTRIBUTION_D, TAG)
            td2 = dc.rekeyed(td, dc.CONTRIBUTION_D)
            got, scaled = ctx.crs_download(new), dc.scalar_crs(orc, n, m, l, u, v, w, td2)
            for key in scaled:
                assert np.array_equal(got[key], scaled[key]), what + (key,)
            ctx.crs_save(new, tmp_path / "contributed.zkcrs")
            assert_lagrange(tmp_path / "contributed.zkcrs", n, ccm.lagrange_arrays(grp, n, td2), what + ("contributed",))
            chk = ctx.crs_contribution_check(up, new, rec, TAG, challenge)
            assert (chk.failed, chk.ok) == (0, True), what + (chk,)
            contributions += 1
    assert containers["tree"][:8] == b"ZKCRSv2\0" and containers["tree"] == containers["squares"], (name, x)
    if name == "control":        # zk_setup accepts this x: its container is a second reference
        ctx.crs_save(ctx.setup(qap, tdl), tmp_path / "setup.zkcrs")
        assert (tmp_path / "setup.zkcrs").read_bytes() == containers["tree"], (name, x)
    return len(containers), batches, contributions


# One case per (n, entry of x_classes(n)): a whole n in one test took 4 to 16 s against 1.3 s of
# test_gpu_change_of_basis_by_the_transposed_tree[1000] in the same session, so the loop over the x classes is pytest's.  Every index
# below CLASS_COUNT[n] is a case, and each case asserts that x_classes(n) has exactly that many entries.
CASES = [(n, index) for n in dc.GPU_SIZES for index in range(dc.CLASS_COUNT[n])]


@pytest.mark.parametrize("n,index", CASES, ids=["%d-%d" % c for c in CASES])
def test_gpu_change_of_basis_of_a_degenerate_crs(ctx, orc, grp, tmp_path, n, index):
    circuit = dc.chain(n)
    m, l, u, v, w, _ = circuit
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    classes = dc.x_classes(orc, n)
    assert len(classes) == dc.CLASS_COUNT[n] == sum(c[0] == n for c in CASES)
    name, x = classes[index]
    old = ctx.get_option("basis_tree_min")
    try:
        counts = check_class(ctx, orc, grp, tmp_path, n, circuit, qap, index, name, x)
    finally:
        ctx.set_option("basis_tree_min", old)
    # both forms ran; the batches over the x = 1 CRS in both forms; the contributions on x = 1 and x = n + 1 in the tree form
    assert counts == (len(FORMS), 2 if x == 1 else 0, 1 if x in (1, n + 1) else 0)
