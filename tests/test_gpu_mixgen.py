"""Mixed circuits on the bit-sliced witness path (csrc/mixgen.hip: the kernels of boolgen_kernels.cuh on the boolean core, k_mix_tail
on the field tail, k_mix_fields): zk_mixgen_run against zk_witgen_run on the same circuit and inputs and against the host runner
(zk_circuit_weights_mixed), word for word, into a buffer that held a byte pattern; every lane, word, group and chunk edge; the tail
shapes that steer the number of waves; refusals of field inputs; zk_mixgen_eval_fields; proofs over a digest and a tail wire.

The generated circuits are tests/generated_circuits.py's as they are drawn (150 to 500 sub-circuits, `wide` about 1200)."""
import hashlib

import numpy as np
import pytest
import torch

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ZkError, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuit import Boolgen, Mixgen, Witgen

import builder_model as bm
import builder_pack_model as pm
import generated_circuits as gc
import mixed_model as mm

pytestmark = pytest.mark.gpu

R = bm.R
COUNTS = (1, 63, 64, 65, 129)
FILL = 0xA5                                                 # the byte an output buffer holds before a call


def build(case):
    lib, model = pm.PackLib(), mm.SplitModel()
    v_lib, v_model = case(lib), case(model)
    assert list(v_lib) == list(v_model)
    return lib.finish(v_lib), model


class Inputs:
    """rows of inputs in creation order -> what each path takes"""

    def __init__(self, model, rows):
        kinds = [k for k in model.kind if k in ("bit", "field")]
        self.count, self.rows = len(rows), rows
        self.tape = np.stack([ints_to_limbs(list(r)) for r in rows]) if kinds else np.zeros((len(rows), 0, 4), np.uint64)
        split = [mm.split_inputs(model, r) for r in rows]
        self.n_bit_bytes = len(split[0][0])
        self.bits = np.zeros((len(rows), max(self.n_bit_bytes, 1)), np.uint8)
        for j, (b, _) in enumerate(split):
            self.bits[j, :len(b)] = np.frombuffer(b, np.uint8)
        self.n_field = len(split[0][1])
        self.fields = (np.stack([ints_to_limbs(f) for _, f in split]) if self.n_field else np.zeros((len(rows), 0, 4), np.uint64))

    def first(self, count):
        other = object.__new__(Inputs)
        other.count, other.rows, other.n_field, other.n_bit_bytes = count, self.rows[:count], self.n_field, self.n_bit_bytes
        other.tape, other.bits, other.fields = self.tape[:count], self.bits[:count], self.fields[:count]
        return other


def host_witnesses(c, ins):
    """the host runner per instance; the first three also through zk_circuit_weights"""
    out = np.zeros((ins.count, c.m, 4), np.uint64)
    for j in range(ins.count):
        out[j] = c.weights_mixed(ins.bits[j][:ins.n_bit_bytes], ins.fields[j])
        if j < 3:
            assert np.array_equal(out[j], c.weights(ins.tape[j]))
    return out


def reference(ctx, c, ins):
    """zk_witgen_run on the same circuit and inputs, equal to the host runner word for word"""
    assert ins.n_bit_bytes == (c.mixed_dims()["n_bit_inputs"] + 7) // 8
    wg = Witgen(ctx, c)
    try:
        tape = wg.run_numpy(ins.tape)
    finally:
        wg.close()
    assert np.array_equal(tape, host_witnesses(c, ins))
    return tape


def run(mg, ins, count=None):
    part = ins if count is None else ins.first(count)
    return mg.run_numpy(part.bits, part.fields, fill=FILL)


def drawn(ctx, shape, seed, count):
    c, model = build(gc.built_case(shape, seed))
    ins = Inputs(model, gc.built_inputs(model, 900 + seed, count))
    return c, model, ins, reference(ctx, c, ins)


# ---- generated circuits -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field_case(ctx):
    """the `field` shape (field inputs, general sub-circuits, packs that are read) with 513 input sets and their witnesses"""
    c, model, ins, want = drawn(ctx, "field", 3, 513)
    d = c.mixed_dims()
    assert not c.boolean and d["core_ops"] > 0 and d["tail_ops"] > 0 and "cpack" in model.cat
    return c, model, ins, want


@pytest.mark.parametrize("shape", ["field", "mixed", "packs", "chain", "wide"])
def test_generated_circuits_at_every_lane_edge(ctx, shape, field_case):
    c, model, ins, want = field_case if shape == "field" else drawn(ctx, shape, 2, max(COUNTS))
    mg = Mixgen(ctx, c)
    for count in COUNTS:
        assert np.array_equal(run(mg, ins, count), want[:count]), count
    mg.close()
    if c.boolean:                                           # a pure boolean circuit: the bytes of zk_boolgen_run
        bg = Boolgen(ctx, c)
        assert bg.run_numpy(ins.bits[:129]).tobytes() == want[:129].tobytes()
        bg.close()


@pytest.mark.parametrize("group_words", [1, 2, 4, 8])
def test_group_words(ctx, field_case, group_words):
    c, model, ins, want = field_case
    for expand_form in (0, 1):
        mg = Mixgen(ctx, c, group_words=group_words, expand_form=expand_form)
        for count in (511, 512, 513) if expand_form == 0 else (513,):
            assert np.array_equal(run(mg, ins, count), want[:count]), (expand_form, count)
        mg.close()


def test_chunks_of_one_and_two_words(ctx, field_case):
    c, model, ins, want = field_case
    need = (c.m + 1) * 8 + c.mixed_dims()["tail_slots"] * 64 * 32
    for words in (1, 2):
        kib = -(-words * need // 1024)
        assert kib * 1024 // need == words
        mg = Mixgen(ctx, c, scratch_kib=kib)
        assert np.array_equal(run(mg, ins, 193), want[:193]), words      # 4 words: 4 chunks, or 2
        assert np.array_equal(mg.eval_fields_numpy(ins.bits[:193], ins.fields[:193], [c.m - 1, 1, 2]), want[:193][:, [c.m - 1, 1, 2], :])
        mg.close()
    with pytest.raises(ZkError) as e:
        Mixgen(ctx, c, scratch_kib=need // 1024 - 1)
    assert e.value.status == _lib.ZK_ERR_SIZE and "boolgen_scratch_kib" in str(e.value)


# ---- tail shapes that steer the W rule ------------------------------------------------------------------------------------------------
def chain_tail(n):
    """n dependent general sub-circuits: every tail level one operation wide -> one wave, no barrier, a register hand-over per step"""
    def case(b):
        x = b.new_bits(9)
        f = b.new_field()
        g = b.gate("xor", x[0], x[1])
        t = b.sub_circuit([(1, f)], [(1, f), (1, g)])
        for i in range(n - 1):
            t = b.sub_circuit([(1, t)], [(1, t), (1, x[i % 9])])
        return [t]
    return case


def level_tail(n):
    """n independent general sub-circuits of one operation each: one tail level n wide -> four waves"""
    def case(b):
        x = b.new_bits(9)
        f, h = b.new_field(), b.new_field()
        g = b.gate("and", x[0], x[1])
        outs = [b.sub_circuit([(1, (f, h, g)[i % 3])], [(1, (h, x[i % 9], f)[i % 3])]) for i in range(n)]
        return [outs[-1], outs[0]]
    return case


def two_op_tail(b):
    x = b.new_bits(2)
    f = b.new_field()
    return [b.sub_circuit([(1, f), (1, x[0])], [(1, f)])]


@pytest.mark.parametrize("name, case, ops, levels", [
    ("chain", chain_tail(300), 600, 600), ("level", level_tail(300), 300, 1), ("level", level_tail(301), 301, 1),
    ("level", level_tail(302), 302, 1), ("level", level_tail(303), 303, 1), ("two", two_op_tail, 2, 2)])
def test_tail_shapes(ctx, name, case, ops, levels):
    """a level of 300 divides evenly over the four waves; 301, 302 and 303 leave every remainder"""
    c, model = build(case)
    d = c.mixed_dims()
    assert (d["tail_ops"], d["tail_levels"]) == (ops, levels)   # mean width 1 -> W = 1; 300 and more -> W = 4
    ins = Inputs(model, gc.built_inputs(model, 31, 129))
    want = reference(ctx, c, ins)
    mg = Mixgen(ctx, c)
    for count in (1, 65, 129):
        assert np.array_equal(run(mg, ins, count), want[:count]), count
    mg.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_field_input_refusals(ctx, field_case):
    c, model, ins, want = field_case
    part = ins.first(70)                                    # the last live lane of a partial word is instance 69
    fields = part.fields.copy()
    mg = Mixgen(ctx, c)
    fields[69, part.n_field - 1] = ints_to_limbs([R - 1])[0]
    got = mg.run_numpy(part.bits, fields, fill=FILL)        # r - 1 is accepted
    assert np.array_equal(got[:69], want[:69])
    fields[69, part.n_field - 1] = [(R >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    with pytest.raises(ZkError) as e:
        mg.run_numpy(part.bits, fields)
    assert e.value.status == _lib.ZK_ERR_RANGE and str(e.value).endswith("instance 69")
    fields[5, 0] = [2 ** 64 - 1] * 4
    for call in (lambda: mg.run_numpy(part.bits, fields), lambda: mg.eval_fields_numpy(part.bits, fields, [1])):
        with pytest.raises(ZkError) as e:
            call()
        assert e.value.status == _lib.ZK_ERR_RANGE and str(e.value).endswith("instance 5")    # the lowest one
    assert np.array_equal(run(mg, part), want[:70])         # the generator is usable afterwards
    dev = "cuda:%d" % ctx.device
    d_out = torch.zeros((2, c.m, 4), dtype=torch.int64, device=dev)
    d_in = torch.from_numpy(part.bits[:2]).to(dev)
    d_f = torch.from_numpy(part.fields[:2].view(np.int64)).to(dev)
    for call in (lambda: mg.run(d_in.data_ptr(), d_f.data_ptr(), 2, d_out.data_ptr(), m=c.m + 1),
                 lambda: mg.run(d_in.data_ptr(), d_f.data_ptr(), 2, d_out.data_ptr(), in_stride=0),
                 lambda: mg.run(d_in.data_ptr(), None, 2, d_out.data_ptr()),
                 lambda: mg.run(d_in.data_ptr(), d_f.data_ptr(), 2, None),
                 lambda: mg.eval_fields(d_in.data_ptr(), d_f.data_ptr(), 2, [c.m], d_out.data_ptr())):
        with pytest.raises(ZkError) as e:
            call()
        assert e.value.status == _lib.ZK_ERR_ARG
    mg.run(None, None, 0, None)                             # count == 0: ZK_OK, nothing touched
    mg.close()
    parsed = zk.circuit.Circuit("(in a b) (out c) (verify c) (program (= c (* a b)))")
    with pytest.raises(ZkError) as e:
        p = zk.circuit.C.c_void_p()
        ctx._check(ctx.lib.zk_mixgen_create(ctx.ptr, parsed.ptr, zk.circuit.C.byref(p)))
    assert e.value.status == _lib.ZK_ERR_UNSUPPORTED


# ---- eval_fields --------------------------------------------------------------------------------------------------------------------
def test_eval_fields_names_wires_of_every_class(ctx, field_case):
    c, model, ins, want = field_case
    fin = model.finish([])                                  # (only the classes are read: the witness order is the library's)
    by_class = {"bit": [], "pack": [], "tail": [], "field_in": []}
    lib_index = lambda w: c.wire_index(w)                   # noqa: E731
    for w in range(2, len(model.kind)):
        if model.kind[w] == "field":
            by_class["field_in"].append(lib_index(w))
        elif model.bitc[w]:
            by_class["bit"].append(lib_index(w))
    for (_, _, out), cat in zip(model.subs, model.cat):
        if cat == "cpack":
            by_class["pack"].append(lib_index(out))
        elif cat == "tail":
            by_class["tail"].append(lib_index(out))
    assert all(by_class.values()) and fin.m == c.m
    wires = [by_class["tail"][-1], by_class["bit"][0], by_class["pack"][0], 0, by_class["tail"][0], by_class["field_in"][-1], by_class["bit"][-1],
             by_class["pack"][-1], by_class["tail"][len(by_class["tail"]) // 2], by_class["bit"][0], c.m - 1, 1]
    mg = Mixgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    for count in (1, 64, 65, 129):
        d_in = torch.from_numpy(ins.bits[:count]).to(dev)
        d_f = torch.from_numpy(ins.fields[:count].view(np.int64)).to(dev)
        d_out = torch.empty((count * len(wires) + 2, 4), dtype=torch.int64, device=dev)
        d_out.view(torch.uint8).fill_(FILL)
        mg.eval_fields(d_in.data_ptr(), d_f.data_ptr(), count, wires, d_out.data_ptr(), in_stride=ins.bits.shape[1])
        got = d_out.cpu().numpy()
        assert (got[count * len(wires):].view(np.uint8) == FILL).all()     # nothing behind the rows is written
        assert np.array_equal(got[:count * len(wires)].view(np.uint64).reshape(count, len(wires), 4), want[:count][:, wires, :]), count
    mg.close()


# ---- SHA3-256 at 2 rounds with a 16-operation tail, end to end ----------------------------------------------------------------------------
def sha3_with_tail(rounds, k):
    """digest of a 64-byte message packed into two wires of 128 bits, one field input c, and a chain of k general sub-circuits
    t0 = (lo + c) hi, t' = t (t + lo); public: the last tail wire and the two packs"""
    def case(b):
        msg = b.new_bits(8 * 64)
        c_in = b.new_field()
        d = b.keccak(msg, 136, 0x06, rounds, 32)
        lo, hi = b.pack(d[:128]), b.pack(d[128:])
        t = b.sub_circuit([(1, lo), (1, c_in)], [(1, hi)])
        for _ in range(k - 1):
            t = b.sub_circuit([(1, t)], [(1, t), (1, lo)])
        return [t, lo, hi]
    return case


def test_prove_and_verify_a_digest_with_a_tail(ctx):
    count, k = 65, 16
    lib = pm.PackLib()
    c = lib.finish(sha3_with_tail(2, k)(lib))
    d = c.mixed_dims()
    assert (d["n_bit_inputs"], d["n_field_inputs"], c.input) == (512, 1, 3) and d["core_ops"] == c.n - k - 2 and not c.boolean
    rng = SplitMix64(77)
    msgs = np.array([[rng.next() & 0xFF for _ in range(64)] for _ in range(count)], np.uint8)
    c_vals = [0, 1, R - 1] + [rng.fr() for _ in range(count - 3)]
    fields = ints_to_limbs(c_vals).reshape(count, 1, 4)
    mg = Mixgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(msgs).to(dev)
    d_f = torch.from_numpy(fields.view(np.int64)).to(dev)
    d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device=dev)
    d_w.view(torch.uint8).fill_(FILL)
    qap = c.qap_sparse_unity(ctx)
    res = mg.run_checked(qap, d_in.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr())
    assert [int(x) for x in res["bad_gates"]] == [0] * count and (res["first_bad"] == _lib.QAP_CHECK_NONE).all() and not res["flags"].any()
    public = mg.eval_fields_numpy(msgs, fields, [1, 2, 3])
    assert np.array_equal(public, d_w.cpu().numpy().view(np.uint64)[:, 1:4, :])
    for j in range(count):
        digest = bm.sponge(bytes(msgs[j]), 136, 0x06, 2, 32)
        lo, hi = int.from_bytes(digest[:16], "little"), int.from_bytes(digest[16:], "little")
        t = (lo + c_vals[j]) * hi % R
        for _ in range(k - 1):
            t = t * (t + lo) % R
        assert limbs_to_ints(public[j]) == [t, lo, hi], j
    assert np.array_equal(d_w[0].cpu().numpy().view(np.uint64), c.weights_mixed(bytes(msgs[0]), fields[0]))
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(count)]
    proofs = []
    for first in range(0, count, 64):                       # a batch holds at most ZK_MAX_BATCH = 64 proofs
        n = min(64, count - first)
        ticket = ctx.prove_batch_submit(crs, qap, ptrs[first:first + n], [c.m] * n, [rng.fr() for _ in range(n)], [rng.fr() for _ in range(n)])
        proofs += ctx.prove_batch_wait(ticket, n)
    assert ctx.verify_batch(crs, public, proofs).all()
    flipped = public.copy()
    flipped[7, 1, 0] ^= np.uint64(1 << 5)                    # one digest bit of instance 7
    assert [j for j, ok in enumerate(ctx.verify_batch(crs, flipped, proofs)) if not ok] == [7]
    tail_wire = c.wire_index(2 + 512 + 1 + (c.n - k - 2) + 2 + 5)       # the sixth tail sub-circuit's output
    assert tail_wire > 3
    d_w[9, tail_wire, 0] ^= 1
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert int(res["bad_gates"][9]) > 0 and sum(int(x) for x in res["bad_gates"]) == int(res["bad_gates"][9])
    forged = ctx.prove_dev(crs, qap, ptrs[9], c.m, rng.fr(), rng.fr())
    assert not ctx.verify(crs, public[9], forged)
    crs.close()
    qap.close()
    mg.close()


def test_sha3_256_digest_beside_a_field_relation(ctx):
    """24 rounds: the digest out of the core equals hashlib's, the tail wire the relation over it"""
    lib = pm.PackLib()
    c = lib.finish(sha3_with_tail(24, 1)(lib))
    rng = SplitMix64(78)
    msgs = np.array([[rng.next() & 0xFF for _ in range(64)] for _ in range(65)], np.uint8)
    c_vals = [rng.fr() for _ in range(65)]
    mg = Mixgen(ctx, c)
    got = mg.eval_fields_numpy(msgs, ints_to_limbs(c_vals).reshape(65, 1, 4), [1, 2, 3])
    for j in range(65):
        digest = hashlib.sha3_256(bytes(msgs[j])).digest()
        lo, hi = int.from_bytes(digest[:16], "little"), int.from_bytes(digest[16:], "little")
        assert limbs_to_ints(got[j]) == [(lo + c_vals[j]) * hi % R, lo, hi], j
    mg.close()
