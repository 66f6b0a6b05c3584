"""zk_boolgen_*: bit-sliced witnesses of boolean built circuits on the GPU (csrc/boolgen.hip) -- equality of 64-bit words with the
tape kernel (zk_witgen_run) on the same circuit and with the host evaluators, at the lane, word, workgroup and chunk edges; SHA3-256
digests against hashlib; proofs from its witnesses verify, and stop verifying when a digest bit or an internal wire is flipped."""
import hashlib

import numpy as np
import pytest
import torch

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ZkError, _lib
from zksnark_rs_amd.circuit import Boolgen, Circuit, Witgen

import builder_cases as bc
import builder_model as bm

pytestmark = pytest.mark.gpu

FORCED_G = 4                       # option boolgen_group_words: a workgroup of the evaluation owns 4 words = 256 instances
COUNTS = (1, 63, 64, 65, 129)
G_COUNTS = (64 * FORCED_G - 1, 64 * FORCED_G, 64 * FORCED_G + 1)


def lib_circuit(case):
    lib = bc.Lib()
    return lib.finish(case(lib))


def random_bits(seed, count, n_in):
    """instance 0 all zero, instance 1 all one, the rest drawn from SplitMix64"""
    rng = SplitMix64(seed)
    rows = [[0] * n_in, [1] * n_in]
    while len(rows) < count:
        word = [rng.next() for _ in range((n_in + 63) // 64)]
        rows.append([(word[i // 64] >> (i % 64)) & 1 for i in range(n_in)])
    return rows[:count]


def host_witnesses(circuit, rows):
    out = np.zeros((len(rows), circuit.m, 4), np.uint64)
    inputs = np.zeros((circuit.n_in, 4), np.uint64)
    for j, bits in enumerate(rows):
        inputs[:, 0] = bits
        out[j] = circuit.weights(inputs)
        if j < 2:
            assert np.array_equal(out[j], circuit.weights_tape(inputs))
    return out


def tape_witnesses(ctx, circuit, rows):
    inputs = np.zeros((len(rows), circuit.n_in, 4), np.uint64)
    inputs[:, :, 0] = np.array(rows, np.uint64).reshape(len(rows), circuit.n_in)
    wg = Witgen(ctx, circuit)
    try:
        return wg.run_numpy(inputs)
    finally:
        wg.close()


@pytest.fixture(scope="module")
def small():
    """the two small circuits with the host witnesses of the most instances any test asks for, computed once (prefixes are shared)"""
    store = {}
    for name, case, seed in (("all_gates", bc.all_gates, 71), ("less_than_eq_8", bc.comparator("less_than_eq", 8), 72)):
        c = lib_circuit(case)
        rows = random_bits(seed, max(G_COUNTS), c.n_in)
        store[name] = (c, rows, host_witnesses(c, rows))
    return store


# ---- packed against tape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_gates", "less_than_eq_8"])
def test_packed_against_tape_and_host(ctx, small, name):
    c, rows, want = small[name]
    assert np.array_equal(tape_witnesses(ctx, c, rows[:129]), want[:129])          # the yardstick itself, on a built circuit
    for group_words, counts in ((None, COUNTS + G_COUNTS), (FORCED_G, COUNTS + G_COUNTS), (1, (129,)), (2, (129,)), (8, (129, 257))):
        bg = Boolgen(ctx, c, group_words=group_words)
        for count in counts:
            got = bg.run_numpy(bc.pack_rows(rows[:count]))
            assert got.shape == (count, c.m, 4)
            assert np.array_equal(got, want[:count]), (group_words, count)
        bg.close()


def test_eval_returns_the_named_wires_packed(ctx, small):
    c, rows, want = small["less_than_eq_8"]
    bg = Boolgen(ctx, c)
    wires = [1, c.m - 1, 0, 5, 17, 2, 9, 30, 1, 3, 11]            # 11 wires: a partial last byte; repeats and the constant allowed
    for count in (1, 65, 129):
        got = bg.eval_numpy(bc.pack_rows(rows[:count]), wires)
        assert got.shape == (count, 2)
        for j in range(count):
            bits = [int(want[j, w, 0]) for w in wires]
            assert bytes(got[j]) == bm.bits_to_bytes(bits + [0] * 5), (count, j)
    # a wider output stride leaves the bytes behind the packed wires alone
    packed = torch.from_numpy(bc.pack_rows(rows[:3])).to("cuda:%d" % ctx.device)
    out = torch.full((3, 5), 0xEE, dtype=torch.uint8, device=packed.device)
    bg.eval(packed.data_ptr(), 3, wires, out.data_ptr(), out_stride=5)
    assert (out[:, 2:].cpu().numpy() == 0xEE).all()


# ---- chunking ---------------------------------------------------------------------------------------------------
def test_chunks_give_identical_witnesses(ctx, small):
    c, rows, want = small["less_than_eq_8"]
    need = (c.m + 1) * 8                                          # bytes of packed state per word of 64 instances
    kib = -(-need // 1024)
    assert kib * 1024 // need < 3                                 # 129 instances = 3 words: at least two chunks
    bg = Boolgen(ctx, c, scratch_kib=kib)
    assert np.array_equal(bg.run_numpy(bc.pack_rows(rows[:129])), want[:129])
    assert np.array_equal(bg.run_numpy(bc.pack_rows(rows[:257])), want[:257])
    digest = bg.eval_numpy(bc.pack_rows(rows[:129]), [1])
    assert [int(x) for x in digest[:, 0]] == [int(want[j, 1, 0]) for j in range(129)]
    bg.close()
    assert ctx.get_option("boolgen_scratch_kib") == 4 << 20       # the handle's cap did not leak into the context
    starved = Boolgen(ctx, c, scratch_kib=kib - 1)
    with pytest.raises(ZkError) as e:
        starved.run_numpy(bc.pack_rows(rows[:1]))
    assert e.value.status == _lib.ZK_ERR_SIZE and "boolgen_scratch_kib" in str(e.value)


# ---- level shapes -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes():
    store = {}

    def get(name, case, seed):
        if name not in store:
            c = lib_circuit(case)
            rows = random_bits(seed, 65, c.n_in)
            store[name] = (c, rows, host_witnesses(c, rows))
        return store[name]
    return get


@pytest.mark.parametrize("count", [1, 65])
@pytest.mark.parametrize("name", ["chain", "wide", "m63", "m64", "m65"])
def test_level_shapes(ctx, shapes, name, count):
    case = {"chain": bc.not_chain(1025), "wide": bc.wide_level(5000), "m63": bc.sized(63), "m64": bc.sized(64), "m65": bc.sized(65)}[name]
    c, rows, want = shapes(name, case, 80 + len(name))
    if name.startswith("m"):
        assert c.m == int(name[1:])
    guard = 3                                                     # elements behind the last witness must stay untouched
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(bc.pack_rows(rows[:count])).to(dev)
    for expand_form in (0, 1):                                    # a lane per wire, a lane pair per wire: the same bytes
        bg = Boolgen(ctx, c, expand_form=expand_form)
        d_out = torch.full((count * c.m + guard, 4), -1, dtype=torch.int64, device=dev)
        bg.run(d_in.data_ptr(), count, d_out.data_ptr())
        got = d_out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:count * c.m].reshape(count, c.m, 4), want[:count]), expand_form
        assert (got[count * c.m:] == 0xFFFFFFFFFFFFFFFF).all(), expand_form
        bg.close()


@pytest.mark.parametrize("count", [1, 65])
def test_input_count_not_a_multiple_of_eight(ctx, shapes, count):
    c, rows, want = shapes("odd", bc.odd_inputs, 90)
    assert c.n_in == 13
    bg = Boolgen(ctx, c)
    clean = bg.run_numpy(bc.pack_rows(rows[:count]))
    dirty = bg.run_numpy(bc.pack_rows(rows[:count], stride=5, fill=0xFF))      # garbage in the unused bits and behind the row
    assert np.array_equal(clean, want[:count]) and np.array_equal(dirty, want[:count])


# ---- full Keccak ------------------------------------------------------------------------------------------------------
def messages(seed, count, n_bytes=64):
    rng = SplitMix64(seed)
    return np.array([[rng.next() & 0xFF for _ in range(n_bytes)] for _ in range(count)], np.uint8)


@pytest.fixture(scope="module")
def sha3_64():
    c = lib_circuit(bc.keccak_case(64, 136, 0x06, 24))
    assert c.n == 8 * 64 + 16 + 9664 * 24 and c.input == 256 and c.boolean
    return c


@pytest.mark.parametrize("count", [1, 65])
def test_sha3_256_digests_against_hashlib(ctx, sha3_64, count):
    msgs = messages(100 + count, count)
    bg = Boolgen(ctx, sha3_64)
    got = bg.eval_numpy(msgs, range(1, 257))                      # a Keccak message is simply its bytes
    for j in range(count):
        assert bytes(got[j]) == hashlib.sha3_256(bytes(msgs[j])).digest(), j
    bg.close()


def test_sha3_256_witnesses_satisfy_the_qap(ctx, sha3_64):
    c = sha3_64
    msgs = messages(103, 3)
    bg = Boolgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(msgs).to(dev)
    d_out = torch.empty((3, c.m, 4), dtype=torch.int64, device=dev)
    bg.run(d_in.data_ptr(), 3, d_out.data_ptr())
    qap = c.qap_sparse_unity(ctx)
    assert qap.n == 1 << 18
    res = ctx.qap_check_dev(qap, d_out.data_ptr(), c.m, 3)
    assert [int(x) for x in res["bad_gates"]] == [0, 0, 0] and (res["first_bad"] == _lib.QAP_CHECK_NONE).all() and not res["flags"].any()
    d_out[1, c.m // 2, 0] ^= 1                                    # one internal wire of instance 1
    res = ctx.qap_check_dev(qap, d_out.data_ptr(), c.m, 3)
    assert int(res["bad_gates"][0]) == 0 and int(res["bad_gates"][1]) > 0 and int(res["bad_gates"][2]) == 0
    qap.close()
    bg.close()


# ---- end to end at 2 rounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["qap_sparse", "qap_sparse_unity"])
def test_prove_and_verify_from_packed_witnesses(ctx, form):
    c = lib_circuit(bc.keccak_case(64, 136, 0x06, 2))
    assert c.n == 8 * 64 + 16 + 9664 * 2 and c.input == 256
    msgs = messages(110, 3)
    bg = Boolgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(msgs).to(dev)
    d_w = torch.empty((3, c.m, 4), dtype=torch.int64, device=dev)
    bg.run(d_in.data_ptr(), 3, d_w.data_ptr())
    digests = bg.eval_numpy(msgs, range(1, 257))
    for j in range(3):
        assert bytes(digests[j]) == bm.sponge(bytes(msgs[j]), 136, 0x06, 2, 32)
    public = [bm.bytes_to_bits(bytes(digests[j])) for j in range(3)]

    qap = getattr(c, form)(ctx)
    rng = SplitMix64(111)
    crs = ctx.setup(qap, zk.ints_to_limbs([rng.fr() for _ in range(5)]))
    ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(3)]
    single = [ctx.prove_dev(crs, qap, ptrs[j], c.m, rng.fr(), rng.fr()) for j in range(3)]
    ticket = ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * 3, [rng.fr() for _ in range(3)], [rng.fr() for _ in range(3)])
    batch = ctx.prove_batch_wait(ticket, 3)
    for j in range(3):
        assert ctx.verify(crs, public[j], single[j]) and ctx.verify(crs, public[j], batch[j]), j
    wrong = list(public[0])
    wrong[77] ^= 1
    assert not ctx.verify(crs, wrong, single[0])                  # one digest bit flipped
    assert not ctx.verify(crs, public[1], single[0])              # another instance's digest
    d_w[2, 256 + 512 + 4000, 0] ^= 1                              # one internal wire of witness 2 (behind the digest and the inputs)
    forged = ctx.prove_dev(crs, qap, ptrs[2], c.m, rng.fr(), rng.fr())
    assert not ctx.verify(crs, public[2], forged)
    crs.close()
    qap.close()
    bg.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, small):
    parsed = Circuit("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n")
    lib = bc.Lib()
    x, y = lib.new_bits(2)
    general = lib.finish([lib.sub_circuit([(1, x)], [(1, y)])])
    for circuit in (parsed, general):
        with pytest.raises(ZkError) as e:
            Boolgen(ctx, circuit)
        assert e.value.status == _lib.ZK_ERR_UNSUPPORTED and "not boolean" in str(e.value)
    c, rows, want = small["all_gates"]
    with pytest.raises(ZkError) as e:
        Boolgen(ctx, c, group_words=3)
    assert e.value.status == _lib.ZK_ERR_ARG and ctx.get_option("boolgen_group_words") == 0
    bg = Boolgen(ctx, c)
    bg.run(0, 0, 0)                                               # count == 0: ZK_OK, nothing touched
    bg.eval(0, 0, [1], 0)
    dev = "cuda:%d" % ctx.device
    d_in = torch.zeros((2, 1), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((2, c.m, 4), dtype=torch.int64, device=dev)

    def refused(fn):
        with pytest.raises(ZkError) as e:
            fn()
        assert e.value.status == _lib.ZK_ERR_ARG

    refused(lambda: bg.run(d_in.data_ptr(), 2, d_out.data_ptr(), m=c.m - 1))
    refused(lambda: bg.run(d_in.data_ptr(), 2, d_out.data_ptr(), in_stride=0))
    refused(lambda: bg.run(0, 2, d_out.data_ptr()))
    refused(lambda: bg.run(d_in.data_ptr(), 2, 0))
    refused(lambda: bg.eval(d_in.data_ptr(), 2, [c.m], d_out.data_ptr()))
    refused(lambda: bg.eval(d_in.data_ptr(), 2, list(range(9)), d_out.data_ptr(), out_stride=1))
    refused(lambda: bg.eval(d_in.data_ptr(), 2, [1], 0))
    assert ctx.lib.zk_boolgen_run(None, None, 0, 0, None, 0) == _lib.ZK_ERR_ARG
    ctx.lib.zk_boolgen_free(None)
    bg.close()


def test_tape_kernel_names_a_bit_input_that_is_no_bit(ctx, small):
    c, rows, want = small["all_gates"]
    inputs = np.zeros((70, c.n_in, 4), np.uint64)
    inputs[:, :, 0] = np.array(rows[:70], np.uint64)
    inputs[66, 2, 0] = 2
    inputs[69, 0, 1] = 1
    wg = Witgen(ctx, c)
    with pytest.raises(ZkError) as e:
        wg.run_numpy(inputs)
    assert e.value.status == _lib.ZK_ERR_RANGE
    assert "input 2 (bit wire 4) of instance 66 is not 0 or 1" in str(e.value)
    inputs[66, 2, 0] = 1
    inputs[69, 0, 1] = 0
    assert wg.run_numpy(inputs).shape == (70, c.m, 4)
    wg.close()
