"""-m gpu: the closing additions of a proof (csrc/prove.hip: k_assemble_pre, k_assemble_pre_batch, k_assemble, k_assemble_batch,
k_sum_partials) on blinding scalars no draw reaches.

blinding_edge_cases.py solves, from the known trapdoor, the (r, s) that make two operands of one of those additions equal, opposite or
infinity, and the digit edges of the 4-bit fixed-base tables; tests/test_blinding_edges.py ties the expected bytes to the reference
restatements on the host.  Here every case goes through every way a proof is assembled -- zk_prove, zk_prove_dev, two tickets in flight
with two different cases, the host-witness submit, a batch with a different case in every block, the two-rank partial sums combined on
one device -- with option merge_lh at 1 and 0, over a CRS zk_setup made and over the oracle's arrays uploaded, for a satisfying witness
and for one broken at one gate, and must give the closed form's bytes.  The circuits are tiny on purpose: these branches do not depend
on the size.  The verdict calls agree on the proofs (those with an element at infinity included), the compressed form round-trips them,
and r or s equal to the modulus is still refused."""
import os
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs

import blinding_edge_cases as bec
from test_blinding_edges import closed_form, infinite_elements

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
ZK_DIR = os.path.join(ROOT, "tests", "golden", "zk")
CIRCUITS = ("chain-8", "chain-64", "integers-5", "simple.zk")
NAMES = bec.CASE_NAMES
MERGE = (1, 0)


def _build(ctx, orc, name):
    import torch
    from test_arbitrary_roots import dense_from_rows, root_poly
    from test_gpu_prove import assert_crs_equal
    if name.startswith("chain-"):
        inst = bec.chain_instance(int(name[6:]).bit_length() - 1)
    elif name.startswith("integers-"):
        inst = bec.integers_instance(int(name[9:]))
    else:
        inst = bec.dense_instance(orc, open(os.path.join(ZK_DIR, name)).read())
    n, m, l = inst["n"], inst["m"], inst["l"]
    tdl = ints_to_limbs(inst["td"])
    if inst["kind"] == "unity":
        qap = ctx.qap_sparse(inst["log_n"], m, l, *inst["rows"])
        arrs = orc.setup_sparse(ctx.sparse_desc(inst["log_n"], m, l, *inst["rows"]), tdl, n, m, l, inst["log_n"] <= 3)
    elif inst["kind"] == "integers":
        qap = ctx.qap_sparse_integers(n, m, l, *inst["rows"])
        dense = [dense_from_rows(inst["roots"], rows, m) for rows in inst["rows"]]
        arrs = orc.setup_dense(*dense, root_poly(inst["roots"]), l, tdl)
    else:
        q = inst["dense"]
        qap = ctx.qap_dense(q["u"], q["v"], q["w"], q["t"], l)
        arrs = orc.setup_dense(q["u"], q["v"], q["w"], q["t"], l, tdl)
    made = ctx.setup(qap, tdl)
    assert_crs_equal(ctx.crs_download(made), arrs)
    inst.update(qap=qap, crs=dict(made=made, uploaded=ctx.crs_upload(n, m, l, arrs)))
    inst["want"] = {k: [closed_form(orc, inst, inst["witnesses"][k], c.r, c.s) for c in inst["cases"][k]] for k in bec.WITNESSES}
    inst["dev"] = {k: torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda() for k, w in inst["witnesses"].items()}
    torch.cuda.synchronize()
    for k in bec.WITNESSES:     # the closed form's bytes show the predicted infinities (the host module ties both to the reference)
        assert [infinite_elements(p) for p in inst["want"][k]] == [c.infinite for c in inst["cases"][k]]
    return inst


@pytest.fixture(scope="module")
def circuits(ctx, orc):
    pytest.importorskip("torch")
    built = {}

    def get(name):
        if name not in built:
            built[name] = _build(ctx, orc, name)
        return built[name]
    yield get
    built.clear()


class merge_lh:
    """option merge_lh for a block, the default (1) restored afterwards"""

    def __init__(self, ctx, value):
        self.ctx, self.value = ctx, value

    def __enter__(self):
        self.ctx.set_option("merge_lh", self.value)
        assert self.ctx.get_option("merge_lh") == self.value

    def __exit__(self, *exc):
        self.ctx.set_option("merge_lh", 1)


def _case(inst, which, name):
    at = NAMES.index(name)
    case = inst["cases"][which][at]
    assert case.name == name
    return case, inst["want"][which][at]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("circuit", CIRCUITS)
def test_prove_and_prove_dev(ctx, circuits, circuit, name):
    """zk_prove and zk_prove_dev: k_assemble_pre with (r, s) as kernel arguments, k_assemble's first call site"""
    inst = circuits(circuit)
    for merge in MERGE:
        with merge_lh(ctx, merge):
            for kind, crs in inst["crs"].items():
                for which in bec.WITNESSES:
                    case, want = _case(inst, which, name)
                    where = (merge, kind, which)
                    assert ctx.prove(crs, inst["qap"], inst["witnesses"][which], case.r, case.s) == want, where
                    assert ctx.prove_dev(crs, inst["qap"], inst["dev"][which].data_ptr(), inst["m"], case.r, case.s) == want, where


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("circuit", CIRCUITS)
def test_two_tickets_in_flight(ctx, circuits, circuit, name):
    """zk_prove_submit / zk_prove_wait and zk_prove_submit_host with two tickets outstanding that carry two different cases (this one
    and the next of the list) and the two witnesses, in one order over the made CRS and in the other over the uploaded one: each slot
    keeps its own pre-sums"""
    inst = circuits(circuit)
    other = NAMES[(NAMES.index(name) + 1) % len(NAMES)]
    qap, m = inst["qap"], inst["m"]
    for merge in MERGE:
        with merge_lh(ctx, merge):
            for (first, second), crs in zip((bec.WITNESSES, bec.WITNESSES[::-1]), inst["crs"].values()):
                (c1, want1), (c2, want2) = _case(inst, first, name), _case(inst, second, other)
                t1 = ctx.prove_submit(crs, qap, inst["dev"][first].data_ptr(), m, c1.r, c1.s)
                t2 = ctx.prove_submit(crs, qap, inst["dev"][second].data_ptr(), m, c2.r, c2.s)
                got = ctx.prove_wait(t1), ctx.prove_wait(t2)      # both collected before either is judged: nothing stays in flight
                assert got == (want1, want2), (merge, first, other)
                h1, h2 = (np.ascontiguousarray(inst["witnesses"][k]) for k in (first, second))
                t1 = ctx.prove_submit_host(crs, qap, h1.ctypes.data, m, c1.r, c1.s)
                t2 = ctx.prove_submit_host(crs, qap, h2.ctypes.data, m, c2.r, c2.s)
                got = ctx.prove_wait(t1), ctx.prove_wait(t2)
                assert got == (want1, want2), (merge, first, other, "host")


@pytest.mark.parametrize("witness", bec.WITNESSES + ("alternating",))
@pytest.mark.parametrize("circuit", CIRCUITS)
def test_batch_with_a_different_case_in_every_block(ctx, circuits, circuit, witness):
    """zk_prove_batch_*: all cases of a circuit in ONE batch, so that k_assemble_pre_batch reads a different (r, s) from device memory
    in every block and k_assemble_batch takes a different branch per block; `alternating` also changes the witness from block to
    block"""
    inst = circuits(circuit)
    assert len(NAMES) <= zk.MAX_BATCH
    which = [witness if witness in bec.WITNESSES else bec.WITNESSES[j & 1] for j in range(len(NAMES))]
    picked = [_case(inst, k, name) for k, name in zip(which, NAMES)]
    ptrs = [inst["dev"][k].data_ptr() for k in which]
    rs, ss = [c.r for c, _ in picked], [c.s for c, _ in picked]
    qap = inst["qap"]
    if inst["kind"] == "dense":
        # batches take the sparse forms (zkgpu.h): the coefficient form is refused, and the same program kept as rows over the roots
        # 1..n is the same QAP -- the same CRS and the same expected bytes
        from zksnark_rs_amd.circuit import Circuit
        with pytest.raises(zk.ZkError) as e:
            ctx.prove_batch_submit(inst["crs"]["made"], qap, ptrs, [inst["m"]] * len(NAMES), rs, ss)
        assert e.value.status == zk._lib.ZK_ERR_UNSUPPORTED
        program = Circuit(open(os.path.join(ZK_DIR, circuit)).read())
        qap = program.qap_sparse(ctx)
        assert (qap.n, qap.m, qap.input) == (inst["n"], inst["m"], inst["l"])
    for merge in MERGE:
        with merge_lh(ctx, merge):
            for kind, crs in inst["crs"].items():
                t = ctx.prove_batch_submit(crs, qap, ptrs, [inst["m"]] * len(NAMES), rs, ss)
                got = ctx.prove_batch_wait(t, len(NAMES))
                wrong = [name for name, p, (_, want) in zip(NAMES, got, picked) if p != want]
                assert not wrong, (merge, kind, wrong)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("circuit", CIRCUITS)
def test_partial_sums_of_two_ranks(ctx, circuits, circuit, name):
    """zk_prove_partial for both ranks of a world of two, combined on one device: k_sum_partials and k_assemble's second call site"""
    import torch
    inst = circuits(circuit)
    qap, m, world = inst["qap"], inst["m"], 2
    for merge in MERGE:
        with merge_lh(ctx, merge):
            for which, crs in zip(bec.WITNESSES, inst["crs"].values()):      # made for the satisfying witness, uploaded for the broken
                case, want = _case(inst, which, name)
                buf = torch.zeros(world * zk.PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
                for rank in range(world):
                    ctx.prove_partial(crs, qap, inst["dev"][which].data_ptr(), m, case.r, case.s, rank, world, buf.data_ptr() + rank * zk.PARTIAL_BYTES)
                torch.cuda.synchronize()
                assert ctx.prove_combine(crs, buf.data_ptr(), world, case.r, case.s) == want, (merge, which)


@pytest.fixture(scope="module")
def reference_verdicts():
    """pyref.verify_bn over pyref's own CRS of the 8-gate chain (the same trapdoor, so the same points)"""
    import functools
    import pyref
    inst = bec.chain_instance(3)
    qap = pyref.qap_from_root_rep(pyref.FR, pyref.chain_root_rep(inst["n"], inst["roots"]))
    s1, s2 = pyref.setup_with_trapdoor(qap, inst["td"])
    ints = zk.limbs_to_ints(inst["witnesses"]["satisfying"])
    patch = pytest.MonkeyPatch()      # e(alpha, beta) and e(input sum, gamma) are the same for every case: paired once
    patch.setattr(pyref, "pairing", functools.lru_cache(maxsize=None)(pyref.pairing))

    def verdict(case, proof):
        points = pyref.trapdoor_proof(qap, inst["td"], ints, case.r, case.s)
        assert pyref.enc_proof(*points) == proof
        return pyref.verify_bn(s1, s2, inst["inputs"], points)
    yield verdict
    patch.undo()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("circuit", CIRCUITS)
def test_every_verdict_call_agrees(ctx, circuits, reference_verdicts, circuit, name):
    """the proof of the satisfying witness: zk_verify, zk_verify_batch, zk_verify_batch_all and the three verifying-key calls give one
    verdict -- accepted, as Groth16's completeness says of an honest proof whatever (r, s) -- and on the 8-gate chain pyref.verify_bn
    gives the same.  An element at infinity changes nothing: e(infinity, .) = 1 on both sides, the rule test_points_at_infinity pins."""
    inst = circuits(circuit)
    case, want = _case(inst, "satisfying", name)
    crs = inst["crs"]["made"]
    proof = ctx.prove(crs, inst["qap"], inst["witnesses"]["satisfying"], case.r, case.s)
    assert proof == want
    rows = [inst["inputs"]]
    key = ctx.verifying_key(crs)
    verdicts = [ctx.verify(crs, rows[0], proof), bool(ctx.verify_batch(crs, rows, [proof])[0]), ctx.verify_batch_all(crs, rows, [proof]),
                key.verify(rows[0], proof), bool(key.verify_batch(ctx, rows, [proof])[0]), key.verify_batch_all(ctx, rows, [proof])]
    key.close()
    assert verdicts == [True] * 6
    if circuit == "chain-8":
        assert reference_verdicts(case, proof) is True


@pytest.mark.parametrize("circuit", CIRCUITS)
def test_verdicts_of_all_cases_in_one_batch(ctx, circuits, circuit):
    """the batch calls over all cases at once: the proofs of the satisfying witness pass, those of the broken one fail one by one
    (and so does the batch as a whole), under the CRS and under its verifying key"""
    inst = circuits(circuit)
    crs = inst["crs"]["uploaded"]
    key = ctx.verifying_key(crs)
    good, bad = inst["want"]["satisfying"], inst["want"]["broken"]
    rows = [inst["inputs"]] * len(good)
    for owner, args in ((ctx, (crs,)), (key, (ctx,))):
        assert owner.verify_batch(*args, rows, good).all()
        assert owner.verify_batch_all(*args, rows, good) is True
        assert not owner.verify_batch(*args, rows, bad).any()
        assert owner.verify_batch_all(*args, rows, bad) is False
        mixed = good[:-1] + bad[-1:]
        assert list(owner.verify_batch(*args, rows, mixed)) == [True] * (len(good) - 1) + [False]
        assert owner.verify_batch_all(*args, rows, mixed) is False
    key.close()


@pytest.mark.parametrize("circuit", CIRCUITS)
def test_compressed_form_round_trips(ctx, circuits, circuit):
    """proof_compress / proof_decompress (host and device forms) give back every proof, those with an element at infinity among them"""
    inst = circuits(circuit)
    for which in bec.WITNESSES:
        proofs = inst["want"][which]
        with_infinity = [p for p, c in zip(proofs, inst["cases"][which]) if c.infinite]
        assert sorted(infinite_elements(p) for p in with_infinity) == ["a", "ab", "b", "c"]
        small = [zk.proof_compress(p) for p in proofs]
        assert [zk.proof_decompress(c) for c in small] == proofs
        packed, ok = ctx.proof_compress_batch(proofs)
        assert ok.all() and [bytes(row) for row in packed] == small
        back, ok = ctx.proof_decompress_batch(small)
        assert ok.all() and [bytes(row) for row in back] == proofs
        if which == "satisfying":
            rows = [inst["inputs"]] * len(proofs)
            assert ctx.verify_batch_compressed(inst["crs"]["made"], rows, small).all()


def test_the_modulus_is_still_refused(ctx, circuits):
    """r = R or s = R: ZK_ERR_RANGE from zk_prove / zk_prove_dev, the submit forms, the batch form and the partial / combine pair;
    nothing stays in flight and the context proves correctly afterwards"""
    import torch
    inst = circuits("chain-8")
    crs, qap, m = inst["crs"]["made"], inst["qap"], inst["m"]
    wts, dev = inst["witnesses"]["satisfying"], inst["dev"]["satisfying"]
    host = np.ascontiguousarray(wts)
    case, want = _case(inst, "satisfying", "pair:r*s=1")
    buf = torch.zeros(2 * zk.PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for r, s in ((bec.R, case.s), (case.r, bec.R), (bec.R, bec.R), (2 ** 256 - 1, case.s)):
        calls = [lambda: ctx.prove(crs, qap, wts, r, s),
                 lambda: ctx.prove_dev(crs, qap, dev.data_ptr(), m, r, s),
                 lambda: ctx.prove_wait(ctx.prove_submit(crs, qap, dev.data_ptr(), m, r, s)),
                 lambda: ctx.prove_wait(ctx.prove_submit_host(crs, qap, host.ctypes.data, m, r, s)),
                 lambda: ctx.prove_batch_wait(ctx.prove_batch_submit(crs, qap, [dev.data_ptr()] * 3, [m] * 3, [case.r, r, case.r], [case.s, s, case.s]), 3),
                 lambda: ctx.prove_partial(crs, qap, dev.data_ptr(), m, r, s, 0, 2, buf.data_ptr()),
                 lambda: ctx.prove_combine(crs, buf.data_ptr(), 2, r, s)]
        for k, call in enumerate(calls):
            with pytest.raises(zk.ZkError) as e:
                call()
            assert e.value.status == zk._lib.ZK_ERR_RANGE, (k, r == bec.R, s == bec.R)
        assert ctx.prove(crs, qap, wts, case.r, case.s) == want
    with pytest.raises(zk.ZkError):
        ctx.prove_wait(0)                         # no refused submit left a ticket behind
    t = ctx.prove_batch_submit(crs, qap, [dev.data_ptr()] * 2, [m] * 2, [case.r, bec.R - 1], [case.s, bec.R - 1])
    top = _case(inst, "satisfying", "digits:r=r-1,s=r-2")
    assert ctx.prove_batch_wait(t, 2)[0] == want
    assert ctx.prove_dev(crs, qap, dev.data_ptr(), m, top[0].r, top[0].s) == top[1]
