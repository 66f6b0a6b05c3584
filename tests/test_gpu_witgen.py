"""zk_witgen_*: circuit::weights for many input sets at once on the GPU (csrc/witgen.hip).  Every instance's m x 4 words must equal
Circuit.weights on that instance's inputs -- equality of 64-bit words, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib
from zksnark_rs_amd.circuit import Circuit, Witgen
from zksnark_rs_amd.circuits import chain_zk

import witgen_cases as wc

pytestmark = pytest.mark.gpu


def host_weights(c, inputs):
    return np.stack([c.weights(inputs[j]) for j in range(inputs.shape[0])])


@pytest.fixture(scope="module")
def cases():
    """per program: the circuit and, computed once, host witnesses of the most instances any test asks for (prefixes are shared)"""
    store = {}

    def get(name, code, count, seed):
        if name not in store:
            c = Circuit(code)
            ins = wc.random_inputs(seed, count, c.n_in)
            store[name] = (c, ins, host_weights(c, ins))
        c, ins, want = store[name]
        assert ins.shape[0] >= count
        return c, ins[:count], want[:count]
    return get


@pytest.mark.parametrize("prog", ["simple.zk", "deg_15.zk"])
def test_lane_and_group_edges(ctx, cases, prog):
    c, ins, want = cases(prog, wc.golden(prog), 129, 11)
    wg = Witgen(ctx, c)
    for count in (1, 63, 64, 65, 129):
        got = wg.run_numpy(ins[:count])
        assert got.shape == (count, c.m, 4)
        assert np.array_equal(got, want[:count]), count
    wg.close()


def test_barriers_with_idle_lanes_comparator(ctx, cases):
    c, ins, want = cases("cmp", wc.golden("8bit_comparator.zk"), 65, 12)
    assert np.array_equal(Witgen(ctx, c).run_numpy(ins), want)


@pytest.mark.parametrize("count", [1, 65])
def test_levels_wider_and_narrower_than_the_workgroup(ctx, cases, count):
    c, ins, want = cases("squares", wc.squares_zk(200), 65, 13)
    assert np.array_equal(Witgen(ctx, c).run_numpy(ins[:count]), want[:count])


def test_chain_takes_the_one_wave_path(ctx, cases):
    n = (1 << 10) + 1
    c, ins, want = cases("chain", chain_zk(n), 3, 14)
    assert c.tape_dims()["width"] == 1 and c.tape_dims()["depth"] == n
    assert np.array_equal(Witgen(ctx, c).run_numpy(ins), want)


def test_odd_programs_on_the_device(ctx):
    c = Circuit(wc.UNUSED_INPUT)
    got = Witgen(ctx, c).run_numpy(zk.ints_to_limbs([3, 4, 5, wc.R - 1]).reshape(2, 2, 4))
    assert zk.limbs_to_ints(got[0]) == [1, 9, 3] and zk.limbs_to_ints(got[1]) == [1, 25, 5]
    c = Circuit(wc.NESTED)
    got = Witgen(ctx, c).run_numpy(zk.ints_to_limbs([3, wc.R - 1]).reshape(2, 1, 4))
    assert zk.limbs_to_ints(got[0]) == [1, 54, 18, 3]
    assert np.array_equal(got[1], c.weights([wc.R - 1]))
    c = Circuit(wc.DEEP)
    a = zk.SplitMix64(7).fr()
    got = Witgen(ctx, c).run_numpy(zk.ints_to_limbs([3, a]).reshape(2, 1, 4))
    assert zk.limbs_to_ints(got[0]) == wc.deep_expected(3) and zk.limbs_to_ints(got[1]) == wc.deep_expected(a)


def test_range_errors_name_the_lowest_instance(ctx, cases):
    c, ins, want = cases("simple.zk", wc.golden("simple.zk"), 129, 11)
    wg = Witgen(ctx, c)
    r_limbs = zk.ints_to_limbs([wc.R])[0]
    bad = ins.copy()
    bad[70, 1] = r_limbs
    with pytest.raises(zk.ZkError) as e:
        wg.run_numpy(bad)
    assert e.value.status == _lib.ZK_ERR_RANGE and "70" in str(e.value)
    bad[5, 2] = r_limbs
    with pytest.raises(zk.ZkError) as e:
        wg.run_numpy(bad)
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 5" in str(e.value) and "70" not in str(e.value)
    assert np.array_equal(wg.run_numpy(ins), want)           # the handle is as good as new
    # an `in` variable the program never reads is checked as well
    c2 = Circuit(wc.UNUSED_INPUT)
    wg2 = Witgen(ctx, c2)
    with pytest.raises(zk.ZkError) as e:
        wg2.run_numpy(zk.ints_to_limbs([3, 4, 5, wc.R]).reshape(2, 2, 4))
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 1" in str(e.value)
    assert zk.limbs_to_ints(wg2.run_numpy(zk.ints_to_limbs([3, 4]).reshape(1, 2, 4))[0]) == [1, 9, 3]


def test_argument_errors(ctx):
    import torch
    lib = ctx.lib
    c = Circuit(wc.golden("simple.zk"))
    wg = Witgen(ctx, c)
    d_in = torch.zeros((2, c.n_in, 4), dtype=torch.int64, device="cuda")
    d_out = torch.zeros((2, c.m, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(zk.ZkError) as e:
        wg.run(d_in.data_ptr(), 2, d_out.data_ptr(), n_in=c.n_in - 1)
    assert e.value.status == _lib.ZK_ERR_ARG and "Wrong number of values supplied" in str(e.value)
    with pytest.raises(zk.ZkError) as e:
        wg.run(d_in.data_ptr(), 2, d_out.data_ptr(), m=c.m + 1)
    assert e.value.status == _lib.ZK_ERR_ARG and "weights buffer size mismatch" in str(e.value)
    assert lib.zk_witgen_run(wg.ptr, None, c.n_in, 0, None, c.m) == _lib.ZK_OK       # count == 0: nothing touched
    assert lib.zk_witgen_run(None, None, c.n_in, 0, None, c.m) == _lib.ZK_ERR_ARG
    for code, text in wc.STATIC_ERRORS:
        p = C.c_void_p()
        bad = Circuit(code)
        assert lib.zk_witgen_create(ctx.ptr, bad.ptr, C.byref(p)) == _lib.ZK_ERR_ARG and not p.value
        assert lib.zk_last_error(ctx.ptr).decode() == text
    lib.zk_witgen_free(None)
    # the circuit may go away before the generator runs
    c.close()
    assert zk.limbs_to_ints(wg.run_numpy(zk.ints_to_limbs([3, 2, 4]).reshape(1, 3, 4))[0]) == [1, 2, 34, 6, 3, 4]


def test_chunks_under_a_low_scratch_cap(ctx, cases):
    c = Circuit(wc.golden("deg_15.zk"))
    ins = wc.random_inputs(15, 200, c.n_in)
    want = host_weights(c, ins)
    group_kib = c.tape_dims()["slots"] * 2                   # slots x 64 lanes x 32 bytes
    wg = Witgen(ctx, c, scratch_kib=group_kib + 1)           # one group of 64 per chunk: four chunks, the last one partial
    assert np.array_equal(wg.run_numpy(ins), want)
    assert ctx.get_option("witgen_scratch_kib") == 8 << 20   # the handle's cap did not leak into the context
    with pytest.raises(zk.ZkError) as e:
        Witgen(ctx, c, scratch_kib=group_kib - 1).run_numpy(ins[:1])
    assert e.value.status == _lib.ZK_ERR_SIZE


def test_end_to_end_prove_and_verify_from_device_witnesses(ctx, cases):
    import torch
    c, ins, want = cases("cmp", wc.golden("8bit_comparator.zk"), 65, 12)
    count = 5
    qap = c.qap_sparse(ctx)
    rng = zk.SplitMix64(16)
    crs = ctx.setup(qap, [rng.fr() for _ in range(5)])
    rs, ss = [rng.fr() for _ in range(count)], [rng.fr() for _ in range(count)]
    d_in = torch.from_numpy(np.ascontiguousarray(ins[:count]).view(np.int64)).cuda()
    d_out = torch.zeros((count, c.m, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    wg = Witgen(ctx, c)
    wg.run(d_in.data_ptr(), count, d_out.data_ptr())
    base = d_out.data_ptr()
    t = ctx.prove_batch_submit(crs, qap, [base + j * c.m * 32 for j in range(count)], [c.m] * count, rs, ss)
    proofs = ctx.prove_batch_wait(t, count)
    for j in range(count):
        assert proofs[j] == ctx.prove(crs, qap, want[j], rs[j], ss[j]), j
    public = np.stack([want[j][1:1 + c.input] for j in range(count)])
    assert ctx.verify_batch(crs, public, proofs).tolist() == [True] * count
    # instance 0's proof against instance 1's public inputs
    mixed = np.concatenate([public, public[1:2]])
    assert ctx.verify_batch(crs, mixed, proofs + [proofs[0]]).tolist() == [True] * count + [False]
