"""Packed wires (zk_builder_pack) on the bit-sliced witness path (csrc/boolgen.hip: k_bool_expand_packs, k_bool_pack_fields):
zk_boolgen_run against zk_witgen_run and zk_circuit_weights word for word at every limb, lane, word and chunk edge; zk_boolgen_eval_fields
against the witnesses' columns and against hashlib; proofs over two packed public inputs verify and stop verifying when an input or an
internal wire is changed."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ZkError, _lib, limbs_to_ints
from zksnark_rs_amd.circuit import Boolgen, Witgen

import builder_cases as bc
import builder_model as bm
import builder_pack_model as pm

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 129)
FILL = -0x0123456789ABCDF0                                  # what an output buffer holds before a call: no plausible witness word


def random_bits(seed, count, n_in):
    """instance 0 all zero, instance 1 all one, the rest drawn from SplitMix64"""
    rng = SplitMix64(seed)
    rows = [[0] * n_in, [1] * n_in]
    while len(rows) < count:
        word = [rng.next() for _ in range((n_in + 63) // 64)]
        rows.append([(word[i // 64] >> (i % 64)) & 1 for i in range(n_in)])
    return rows[:count]


def host_witnesses(circuit, rows):
    """zk_circuit_weights per instance (and the host tape on the first two)"""
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


def run_prefilled(ctx, bg, circuit, packed_rows, guard=3):
    """zk_boolgen_run into a buffer that held FILL everywhere -> (count, m, 4) uint64; the elements behind the last witness are checked"""
    dev = "cuda:%d" % ctx.device
    count = packed_rows.shape[0]
    d_in = torch.from_numpy(packed_rows).to(dev)
    d_out = torch.full((count * circuit.m + guard, 4), FILL, dtype=torch.int64, device=dev)
    bg.run(d_in.data_ptr(), count, d_out.data_ptr(), in_stride=packed_rows.shape[1])
    got = d_out.cpu().numpy()
    assert (got[count * circuit.m:] == FILL).all()
    return got[:count * circuit.m].view(np.uint64).reshape(count, circuit.m, 4)


@pytest.fixture(scope="module")
def widths():
    """the ~300-gate circuit with packs of every width, its inputs and the host witnesses of the most instances any test asks for"""
    c = pm.lib_circuit(pm.all_widths)
    assert c.boolean and c.packed_wires == 11 and c.n == 311
    rows = random_bits(171, max(COUNTS), c.n_in)
    return c, rows, host_witnesses(c, rows)


# ---- parity ---------------------------------------------------------------------------------------------------------
def test_the_three_witness_paths_agree(ctx, widths):
    c, rows, want = widths
    # the packed wires are where they are meant to be and hold what the model says
    assert [c.wire_index(w) for w in (2 + 40 + 300 + 4, 2 + 40 + 300 + 10)] == [1, c.m - 1]
    assert limbs_to_ints(want[1, 3:4]) == [(1 << 40) - 1]                              # the pack over the 40 inputs, all ones
    assert np.array_equal(tape_witnesses(ctx, c, rows), want)                          # zk_witgen_run == zk_circuit_weights
    bg = Boolgen(ctx, c)
    for count in COUNTS:
        got = run_prefilled(ctx, bg, c, bc.pack_rows(rows[:count]))
        assert np.array_equal(got, want[:count]), count                                 # zk_boolgen_run == both, word for word
    bg.close()


@pytest.mark.parametrize("m", [63, 64, 65])
def test_witness_index_alignment(ctx, m):
    c = pm.lib_circuit(pm.sized_with_pack(m))
    assert c.m == m and c.boolean and c.packed_wires == 1
    rows = random_bits(180 + m, 65, c.n_in)
    want = host_witnesses(c, rows)
    for expand_form in (0, 1):
        bg = Boolgen(ctx, c, expand_form=expand_form)
        for count in (1, 65):
            assert np.array_equal(run_prefilled(ctx, bg, c, bc.pack_rows(rows[:count])), want[:count]), (expand_form, count)
        bg.close()


def test_many_packs(ctx):
    c = pm.lib_circuit(pm.many_packs(300))
    assert c.packed_wires == 300 and c.boolean
    rows = random_bits(190, 65, c.n_in)
    want = host_witnesses(c, rows)
    bg = Boolgen(ctx, c)
    assert np.array_equal(run_prefilled(ctx, bg, c, bc.pack_rows(rows)), want)
    got = bg.eval_fields_numpy(bc.pack_rows(rows), range(c.m))                         # every wire, packed or not, as a field element
    assert np.array_equal(got, want)
    bg.close()


# ---- chunking ---------------------------------------------------------------------------------------------------------
def test_chunks_give_identical_bytes(ctx, widths):
    c, rows, want = widths
    need = (c.m + 1) * 8                                          # bytes of packed state per word of 64 instances
    kib = -(-need // 1024)
    assert kib * 1024 // need == 1                                # one word per chunk: 129 instances are three chunks
    packed = bc.pack_rows(rows[:129])
    whole = Boolgen(ctx, c)
    reference = run_prefilled(ctx, whole, c, packed)
    assert np.array_equal(reference, want[:129])
    wires = [1, 3, c.m - 1, 2, 0, 77]
    fields = whole.eval_fields_numpy(packed, wires)
    whole.close()
    for expand_form, group_words in ((0, None), (1, 1), (1, 8)):
        bg = Boolgen(ctx, c, scratch_kib=kib, expand_form=expand_form, group_words=group_words)
        got = run_prefilled(ctx, bg, c, packed)
        assert got.tobytes() == reference.tobytes(), (expand_form, group_words)
        assert np.array_equal(bg.eval_fields_numpy(packed, wires), fields), (expand_form, group_words)
        bg.close()
    for expand_form, group_words in ((1, 1), (1, 8)):             # the same forms unchunked
        bg = Boolgen(ctx, c, expand_form=expand_form, group_words=group_words)
        assert run_prefilled(ctx, bg, c, packed).tobytes() == reference.tobytes(), (expand_form, group_words)
        bg.close()


# ---- eval_fields ----------------------------------------------------------------------------------------------------------
def test_eval_fields_returns_columns_of_the_witnesses(ctx, widths):
    c, rows, want = widths
    packed_at = sorted(c.wire_index(2 + 40 + 300 + k) for k in range(11))
    wires = [1, 5, packed_at[3], 0, c.m - 1, 2, packed_at[8], 3, 41, 1, packed_at[0]]  # bits, packed wires, the constant, a repeat
    bg = Boolgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    guard = 2
    for count in (1, 64, 65):
        d_in = torch.from_numpy(bc.pack_rows(rows[:count])).to(dev)
        d_out = torch.full((count * len(wires) + guard, 4), FILL, dtype=torch.int64, device=dev)
        bg.eval_fields(d_in.data_ptr(), count, wires, d_out.data_ptr())
        got = d_out.cpu().numpy()
        assert (got[count * len(wires):] == FILL).all()                                # nothing behind the rows is written
        got = got[:count * len(wires)].view(np.uint64).reshape(count, len(wires), 4)
        assert np.array_equal(got, want[:count][:, wires, :]), count
    # the bits-out call refuses a packed wire and is unchanged on bit wires
    d_in = torch.from_numpy(bc.pack_rows(rows[:65])).to(dev)
    d_bits = torch.zeros((65, 1), dtype=torch.uint8, device=dev)
    for bad in (packed_at[0], c.m - 1, 1):
        with pytest.raises(ZkError) as e:
            bg.eval(d_in.data_ptr(), 65, [2, bad], d_bits.data_ptr())
        assert e.value.status == _lib.ZK_ERR_ARG and "packed wire" in str(e.value)
    assert not d_bits.cpu().numpy().any()                                              # a refused call wrote nothing
    bit_wires = [w for w in range(c.m) if w not in packed_at][:19]
    got = bg.eval_numpy(bc.pack_rows(rows[:65]), bit_wires)
    for j in range(65):
        assert bytes(got[j]) == bm.bits_to_bytes([int(want[j, w, 0]) for w in bit_wires] + [0] * 5), j
    # refusals of the new call: as zk_boolgen_eval's
    d_out = torch.zeros((65, 2, 4), dtype=torch.int64, device=dev)
    for call in (lambda: bg.eval_fields(d_in.data_ptr(), 65, [c.m], d_out.data_ptr()),
                 lambda: bg.eval_fields(d_in.data_ptr(), 65, [1, 2], d_out.data_ptr(), in_stride=4),
                 lambda: bg.eval_fields(0, 65, [1, 2], d_out.data_ptr()),
                 lambda: bg.eval_fields(d_in.data_ptr(), 65, [1, 2], 0)):
        with pytest.raises(ZkError) as e:
            call()
        assert e.value.status == _lib.ZK_ERR_ARG
    bg.eval_fields(0, 0, [1], 0)                                                       # count == 0: ZK_OK, nothing touched
    bg.eval_fields(d_in.data_ptr(), 65, [], 0)
    assert ctx.lib.zk_boolgen_eval_fields(None, None, 0, 0, None, 0, None) == _lib.ZK_ERR_ARG
    bg.close()


def test_a_packed_wire_that_is_read_is_refused_by_boolgen(ctx):
    lib = pm.PackLib()
    xs = lib.new_bits(4)
    p = lib.pack(xs[:3])
    lib.gate("and", p, xs[3])
    c = lib.finish([p])
    assert not c.boolean and c.packed_wires == 1
    with pytest.raises(ZkError) as e:
        Boolgen(ctx, c)
    assert e.value.status == _lib.ZK_ERR_UNSUPPORTED and "not boolean" in str(e.value)
    rows = random_bits(195, 5, 4)
    assert np.array_equal(tape_witnesses(ctx, c, rows), host_witnesses(c, rows))       # the tape takes it


# ---- SHA3-256 ---------------------------------------------------------------------------------------------------------------
def messages(seed, count, n_bytes=64):
    rng = SplitMix64(seed)
    return np.array([[rng.next() & 0xFF for _ in range(n_bytes)] for _ in range(count)], np.uint8)


def test_sha3_256_digest_as_two_field_elements(ctx):
    c = pm.lib_circuit(pm.digest_packed(64, 24))
    assert c.n == 8 * 64 + 16 + 9664 * 24 + 2 and c.input == 2 and c.boolean and c.packed_wires == 2
    msgs = messages(201, 65)
    bg = Boolgen(ctx, c)
    got = bg.eval_fields_numpy(msgs, [1, 2])                      # a Keccak message is simply its bytes
    for j in range(65):
        digest = hashlib.sha3_256(bytes(msgs[j])).digest()
        assert limbs_to_ints(got[j]) == [int.from_bytes(digest[16 * k:16 * k + 16], "little") for k in range(2)], j
    bg.close()


# ---- end to end at 2 rounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["qap_sparse", "qap_sparse_unity"])
def test_prove_and_verify_over_two_packed_inputs(ctx, form):
    c = pm.lib_circuit(pm.digest_packed(64, 2))
    assert c.n == 8 * 64 + 16 + 9664 * 2 + 2 and c.input == 2 and c.boolean
    count = 3
    msgs = messages(210, count)
    bg = Boolgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(msgs).to(dev)
    d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device=dev)
    bg.run(d_in.data_ptr(), count, d_w.data_ptr())
    public = bg.eval_fields_numpy(msgs, [1, 2])                   # (count, 2, 4): the `inputs` array of zk_verify_batch as it is
    for j in range(count):
        digest = bm.sponge(bytes(msgs[j]), 136, 0x06, 2, 32)
        assert limbs_to_ints(public[j]) == [int.from_bytes(digest[:16], "little"), int.from_bytes(digest[16:], "little")]

    qap = getattr(c, form)(ctx)
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert [int(x) for x in res["bad_gates"]] == [0] * count and (res["first_bad"] == _lib.QAP_CHECK_NONE).all() and not res["flags"].any()
    rng = SplitMix64(211)
    crs = ctx.setup(qap, zk.ints_to_limbs([rng.fr() for _ in range(5)]))
    n, m, l = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert ctx.lib.zk_crs_dims(crs.ptr, C.byref(n), C.byref(m), C.byref(l)) == 0
    assert (m.value, l.value) == (c.m, 2)
    assert ctx.crs_download(crs)["sum_gamma_g1"].shape[0] == 3    # 3 sum_gamma points where the bit form carries 257
    ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(count)]
    ticket = ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * count, [rng.fr() for _ in range(count)], [rng.fr() for _ in range(count)])
    proofs = ctx.prove_batch_wait(ticket, count)
    assert ctx.verify_batch(crs, public, proofs).all()
    assert all(ctx.verify(crs, public[j], proofs[j]) for j in range(count))
    off_by_one = public.copy()
    off_by_one[1, 0, 0] ^= np.uint64(1)                           # the low element of proof 1, +-1
    assert list(ctx.verify_batch(crs, off_by_one, proofs)) == [True, False, True]
    high = public.copy()
    assert high[2, 1, 2] == 0
    high[2, 1, 2] = 1                                             # the high element of proof 2, + 2^128: still below r
    assert list(ctx.verify_batch(crs, high, proofs)) == [True, True, False]
    swapped = public[:, ::-1, :].copy()
    assert not ctx.verify_batch(crs, swapped, proofs).any()
    d_w[0, 2 + 512 + 4000, 0] ^= 1                                # one internal wire of witness 0 (behind the inputs)
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert int(res["bad_gates"][0]) > 0 and [int(x) for x in res["bad_gates"][1:]] == [0] * (count - 1)
    forged = ctx.prove_dev(crs, qap, ptrs[0], c.m, rng.fr(), rng.fr())
    assert not ctx.verify(crs, public[0], forged)
    crs.close()
    qap.close()
    bg.close()
