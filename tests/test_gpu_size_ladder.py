"""-m gpu: a proof at EVERY size 2^0 .. 2^21 against the trapdoor closed form, and after each proof the plan the library recorded
for its inner products (Context.msm_plans()) against the restatement of tests/msm_plan_model.py at the device's compute-unit count.

The prover's size-dependent layer -- the window of each table, the run length and the rule that set it, the tail form, the chaining,
the column / row split of the fused two-pass transforms -- differs at every log_n.  2^7, 2^15, 2^17, 2^18, 2^19 and 2^21 were proven
by no test; three of them hold plans that exist nowhere else (tests/test_msm_plan.py lists them).  Those six sizes also run with
merge_lh = 0, with a boolean and a 32-bit witness (heavy buckets under each plan), with two proofs in flight, and through zk_verify.
The integer roots: one size inside the band where A and B take run_fill below RUN_MAX, and 2^18, whose merged table has 2^20 - 2
points.  Batches at the sizes the README quotes.  Everything compares bytes; the closed form shares no code with the prover."""
import numpy as np
import pytest
import torch

import msm_plan_model as M
from msm_plan_model import assert_plans, device_cu, limbs
import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs, R_MODULUS as R
from zksnark_rs_amd.circuits import chain_rows
from test_gpu_circuit_shapes import options
from test_integer_roots import chain_rows_integers

pytestmark = pytest.mark.gpu


def chain_witness(n, x, avals):
    """[1, x, y, t1, a1, t2, a2, .., a_n]: the wire order of the chain circuit over either domain"""
    t, out = 0, [1, x, 0]
    for k in range(n - 1):
        t = x * (t + avals[k]) % R
        out += [t, avals[k]]
    out[2] = (t + avals[n - 1]) % R
    return limbs(out + [avals[n - 1]])


def flipped(weights, m):
    bad = weights.copy()
    bad[max(3, m // 2), 1] ^= np.uint64(1)         # a private wire, +- 2^64: still below r, no longer satisfying
    return bad


@pytest.mark.parametrize("log_n", M.LADDER)
def test_prove_at_every_size(ctx, orc, log_n):
    """the chain circuit of 2^log_n gates: a valid witness and one with a flipped limb == the closed form, and the recorded plan of
    A, B and the merged product == the restatement.  At the six sizes no other test proves: the same with merge_lh = 0 (L, A, B, H),
    boolean and 32-bit inputs, two proofs in flight through zk_prove_submit, zk_verify accepting the one and rejecting the other."""
    cu = device_cu(ctx, orc)
    n, m, l = M.chain_dims(log_n)
    rows = chain_rows(log_n)
    assert rows[:2] == (m, l)
    rng = SplitMix64(7100 + log_n)
    gen = np.random.default_rng(7100 + log_n)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    r, s, x = rng.fr(), rng.fr(), rng.fr()
    desc = ctx.sparse_desc(log_n, *rows)
    qap = ctx.qap_sparse(log_n, *rows)
    crs = ctx.setup(qap, td)
    want_plan = M.proof_plans(n, m, l, cu)

    def check(weights, what, merge=True):
        ctx.msm_plan_reset()
        got = ctx.prove(crs, qap, weights, r, s)
        assert_plans(ctx, M.proof_plans(n, m, l, cu, merge_lh=merge), (log_n, what))
        want = orc.trapdoor_proof_sparse(desc, td, weights, r, s)
        assert got == want, (log_n, what)
        return got

    good = chain_witness(n, x, [int(v) for v in gen.integers(0, 1 << 63, size=n)])      # 63-bit inputs keep generation fast
    bad = flipped(good, m)
    p_good, p_bad = check(good, "valid"), check(bad, "flipped")
    assert p_good != p_bad
    if log_n not in M.NEW_SIZES:
        return
    with options(ctx, merge_lh=0):
        assert check(good, "merge_lh 0", merge=False) == p_good
        assert check(bad, "merge_lh 0, flipped", merge=False) == p_bad
    check(chain_witness(n, x, [int(v) for v in gen.integers(0, 2, size=n)]), "boolean")
    check(chain_witness(n, x, [int(v) for v in gen.integers(0, 1 << 32, size=n)]), "32-bit")
    dws = [torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda() for w in (good, bad)]
    torch.cuda.synchronize()
    ctx.msm_plan_reset()
    t1 = ctx.prove_submit(crs, qap, dws[0].data_ptr(), m, r, s)
    t2 = ctx.prove_submit(crs, qap, dws[1].data_ptr(), m, s, r)
    assert ctx.prove_wait(t1) == p_good
    assert ctx.prove_wait(t2) == orc.trapdoor_proof_sparse(desc, td, bad, s, r)
    assert_plans(ctx, want_plan + want_plan, (log_n, "two in flight"))
    assert ctx.verify(crs, good[1:1 + l], p_good)
    assert not ctx.verify(crs, bad[1:1 + l], p_bad)


@pytest.mark.parametrize("which", range(len(M.INTEGER_SIZES)))
def test_prove_over_the_integer_roots(ctx, orc, which):
    """the chain circuit over the roots 1 .. n.  Size 0: the first n at which the n-point products A and B leave the whole stretch of
    the c = 17 window -- run_fill with 32 < T < 256, in the unsharded prover reached by nothing else (563610 gates at 256 compute
    units: the smallest size of the band, which keeps the rows and the witness Python builds gate by gate short).  Size 1: 2^18 gates,
    merged table of 2^20 - 2 points: the first size the n + 8 >= 2^20 clause of the window rule takes."""
    cu = device_cu(ctx, orc)
    n = M.integer_sizes(cu)[which]
    m, l, u, v, w = chain_rows_integers(n)
    rng = SplitMix64(7300 + which)
    gen = np.random.default_rng(7300 + which)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    r, s, x = rng.fr(), rng.fr(), rng.fr()
    desc = ctx.sparse_desc(0, m, l, u, v, w)
    qap = ctx.qap_sparse_integers(n, m, l, u, v, w)
    crs = ctx.setup(qap, td)
    want_plan = M.proof_plans(n, m, l, cu, integers=True)
    if which == 0:
        assert want_plan[0]["run_branch"] == want_plan[1]["run_branch"] == M.FILL and 32 < want_plan[0]["run_len"] < 256
    else:
        assert want_plan[2]["n_used"] == (1 << 20) - 2 and want_plan[2]["c"] == 20
    good = chain_witness(n, x, [int(a) for a in gen.integers(0, 1 << 63, size=n)])
    bad = flipped(good, m)
    proofs = []
    for weights, what in ((good, "valid"), (bad, "flipped")):
        ctx.msm_plan_reset()
        got = ctx.prove(crs, qap, weights, r, s)
        assert_plans(ctx, want_plan, (n, what))
        assert got == orc.trapdoor_proof_integers(desc, n, td, weights, r, s), (n, what)
        proofs.append(got)
    assert ctx.verify(crs, good[1:1 + l], proofs[0]) and not ctx.verify(crs, bad[1:1 + l], proofs[1])


@pytest.mark.parametrize("log_n,count", M.BATCHES)
def test_prove_batches_at_the_advertised_sizes(ctx, orc, log_n, count):
    """zk_prove_batch_submit with ZK_MAX_BATCH = 64 proofs of 16 gates and of 2^16 gates (the README's figures; with 64 groups and
    c >= 10 the level-1 counters of the sort are exactly the 64 KiB of LDS msm_run accepts) and 17 proofs of 2^10 gates: a distinct
    (r, s) per proof, four distinct witnesses in turn; == zk_prove one by one == the closed form; the grouped products' plan == the
    restatement.  Were a count refused for size, the refusal must be ZK_ERR_SIZE and the largest accepted count is tested (64
    proofs of 2^16 gates are accepted: measured)."""
    assert count <= zk.MAX_BATCH
    cu = device_cu(ctx, orc)
    n, m, l = M.chain_dims(log_n)
    rows = chain_rows(log_n)
    rng = SplitMix64(7500 + log_n)
    gen = np.random.default_rng(7500 + log_n)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    desc = ctx.sparse_desc(log_n, *rows)
    qap = ctx.qap_sparse(log_n, *rows)
    crs = ctx.setup(qap, td)
    four = [chain_witness(n, rng.fr(), [int(a) for a in gen.integers(0, 1 << 63, size=n)]) for _ in range(3)]
    four.append(flipped(four[0], m))
    dws = [torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda() for w in four]
    torch.cuda.synchronize()
    rs, ss = [rng.fr() for _ in range(count)], [rng.fr() for _ in range(count)]
    assert len(set(zip(rs, ss))) == count
    while True:
        ctx.msm_plan_reset()
        try:
            t = ctx.prove_batch_submit(crs, qap, [dws[j % 4].data_ptr() for j in range(count)], [m] * count, rs[:count], ss[:count])
            break
        except zk.ZkError as e:
            assert e.status == zk._lib.ZK_ERR_SIZE and not M.batch_fits(n, m, l, count), (count, e)
            count -= 1
    print("batch of 2^%d gates: %d proofs accepted" % (log_n, count))
    got = ctx.prove_batch_wait(t, count)
    assert M.batch_fits(n, m, l, count)
    assert_plans(ctx, M.batch_plans(n, m, l, count, cu), (log_n, count))
    for j in range(count):
        assert got[j] == orc.trapdoor_proof_sparse(desc, td, four[j % 4], rs[j], ss[j]), j
        assert got[j] == ctx.prove(crs, qap, four[j % 4], rs[j], ss[j]), j
    assert len(set(got)) == count
