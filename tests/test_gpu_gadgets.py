"""The curve and hash gadgets on the device witness paths: every case of tests/gadget_cases.py through zk_witgen_run (k_witgen) and
zk_mixgen_run (the bit-sliced core and k_mix_tail) against the witness tests/babyjub_model.py computes in Python integers, word for
word on every instance, among them a chain of the gadgets' gate sides, the one tape here that runs with one wave a group and hands
results on in registers; chunking on the deep variable-base tape; zk_qap_check_dev naming the failing gate; and the statement
[S] Base8 = R + [h] A at 251 bits fed device to device from zk_babyjub_mul_batch, its digests against zk_poseidon_hash_batch, through
the prover to proofs that verify.  The model's witnesses are computed once per case and shared (gadget_cases.Case)."""
import numpy as np
import pytest
import torch

from zksnark_rs_amd import SplitMix64, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd import babyjub
from zksnark_rs_amd.circuit import Mixgen, Witgen

import babyjub_model as bm
import gadget_cases as gc

pytestmark = pytest.mark.gpu

R = bm.R
FILL = 0xA5                                                 # the byte an output buffer holds before a call
SPARE = 3                                                   # rows behind the last witness that a call must leave alone
COUNTS = (1, 63, 64, 65, 129)                               # one lane, a wave less one, a wave, a wave and one, two waves and one
SWEPT = ("add_affine", "mul_var_7", "poseidon_4")
CASES = gc.all_cases()


def to_dev(ctx, a):
    a = np.array(a)                                         # a copy: the cases' arrays are shared and read-only
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:%d" % ctx.device)


def filled(ctx, count, m):
    d_out = torch.empty((count + SPARE, m, 4), dtype=torch.int64, device="cuda:%d" % ctx.device)
    d_out.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    return d_out


def split_output(d_out, count):
    out = d_out.cpu().numpy().view(np.uint64)
    return out[:count], out[count:]


def run_witgen(ctx, case, count, d_in=None, scratch_kib=None):
    """-> (witnesses (count, m, 4), the spare rows, the device buffer)"""
    wg = Witgen(ctx, case.c, scratch_kib=scratch_kib)
    d_in = to_dev(ctx, case.tape_inputs()[:count]) if d_in is None else d_in
    d_out = filled(ctx, count, case.c.m)
    wg.run(d_in.data_ptr(), count, d_out.data_ptr())
    wg.close()
    return split_output(d_out, count) + (d_out,)


def run_mixgen(ctx, case, count):
    bits, fields = case.mixed_inputs()
    mg = Mixgen(ctx, case.c)
    d_bits = to_dev(ctx, bits[:count])
    d_fields = to_dev(ctx, fields[:count]) if fields.shape[1] else None
    d_out = filled(ctx, count, case.c.m)
    mg.run(d_bits.data_ptr(), None if d_fields is None else d_fields.data_ptr(), count, d_out.data_ptr(), in_stride=bits.shape[1])
    mg.close()
    return split_output(d_out, count) + (d_out,)


def first_difference(got, want):
    """(instance, witness index) of the first word that differs, for the assertion's message"""
    bad = np.argwhere((got != want).any(axis=2))
    return None if not len(bad) else (int(bad[0][0]), int(bad[0][1]))


# ---- a. every case through both device paths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_witgen_and_mixgen_against_the_model(ctx, name):
    case = CASES[name]()
    want = case.want_words()
    full = len(case.rows)
    for count in (COUNTS if name in SWEPT else (full,)):    # prefixes of one input array
        assert count <= full
        for run in (run_witgen, run_mixgen):
            got, spare, _ = run(ctx, case, count)
            assert np.array_equal(got, want[:count]), (run.__name__, count, first_difference(got, want[:count]))
            assert (spare.view(np.uint8) == FILL).all(), (run.__name__, count)


# ---- b. chunking on a deep tape -------------------------------------------------------------------------------------------------
def test_a_deep_tape_in_chunks_of_one_group(ctx):
    case = gc.mul_var_case(7)
    count = 129                                             # three chunks, the last of one instance
    group_kib = case.c.tape_dims()["slots"] * 2             # slots x 64 lanes x 32 bytes
    whole, _, _ = run_witgen(ctx, case, count)
    got, spare, _ = run_witgen(ctx, case, count, scratch_kib=group_kib + 1)
    assert np.array_equal(got, whole) and np.array_equal(got, case.want_words()[:count])
    assert (spare.view(np.uint8) == FILL).all()


# ---- c. the device QAP check names the gate -------------------------------------------------------------------------------------
def test_qap_check_tells_points_on_the_curve_from_points_off_it_within_a_wave(ctx):
    case = gc.on_curve_case()
    count = len(case.rows)
    qap = case.c.qap_sparse_unity(ctx)
    for run in (run_witgen, run_mixgen):
        _, _, d_w = run(ctx, case, count)
        res = ctx.qap_check_dev(qap, d_w.data_ptr(), case.c.m, count)
        on, off = slice(0, count, 2), slice(1, count, 2)
        assert (res["bad_gates"][on] == 0).all() and (res["first_bad"][on] == _lib.QAP_CHECK_NONE).all(), run.__name__
        assert (res["bad_gates"][off] == 1).all() and (res["first_bad"][off] == 3).all(), run.__name__
    qap.close()


@pytest.mark.parametrize("q_affine", [True, False])
def test_qap_check_names_the_assertion_a_wrong_coordinate_breaks(ctx, q_affine):
    case = gc.add_case(q_affine)
    count, n, at = 65, case.c.n, case.info["x_input"]
    qap = case.c.qap_sparse_unity(ctx)
    x_off, y_off = (0, 63, 64), (2, 62)                     # the instances whose supplied x, or y, is pushed off by one
    ins = case.tape_inputs()[:count]
    for j, k in [(j, at) for j in x_off] + [(j, at + 1) for j in y_off]:   # one more is still below r and carries into no second word
        assert case.rows[j][k] + 1 < R and ins[j, k, 0] != np.uint64(2 ** 64 - 1)
    d_in = to_dev(ctx, ins)
    for j in x_off:
        d_in[j, at, 0] += 1
    for j in y_off:
        d_in[j, at + 1, 0] += 1
    torch.cuda.synchronize()
    _, _, d_w = run_witgen(ctx, case, count, d_in=d_in)
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), case.c.m, count)
    want_first = {j: n - 3 for j in x_off}                  # the gates test_babyjub.py names on the host
    want_first.update({j: n - 1 for j in y_off})
    assert [int(x) for x in res["first_bad"]] == [want_first.get(j, _lib.QAP_CHECK_NONE) for j in range(count)]
    assert [int(x) for x in res["bad_gates"]] == [int(j in want_first) for j in range(count)]
    qap.close()


# ---- d, e. the kernels meet the gadgets ---------------------------------------------------------------------------------------------
N_S = N_H = 251
ROW_WORDS = 4 * gc.STATEMENT_FIELDS                         # a row of field inputs: Ax, Ay, Rx, Ry, M, Ox, Oy
AT_A, AT_R, AT_M, AT_O = 0, 2, 4, 5


def words_of(values):
    return babyjub.scalars_to_words(list(values))


def packed_bits(s, h):
    """the bit inputs of one instance: S, then h"""
    return np.frombuffer((s | (h << N_S)).to_bytes((N_S + N_H + 7) // 8, "little"), np.uint8)


def fill_rows(ctx, scalars, messages):
    """S, h, A, M -> the field rows (count, 7, 4) on the device.  O = [S] Base8 comes from the fixed-base kernel, written into the
    rows with the row as its stride; [h] A from the variable-base kernel; R = O - [h] A is completed on the host from the kernels'
    output through the model's add and neg, and uploaded.  Nothing but R visits the host."""
    count = len(scalars)
    d_s = to_dev(ctx, words_of(s for s, _, _ in scalars))
    d_h = to_dev(ctx, words_of(h for _, h, _ in scalars))
    d_a = to_dev(ctx, np.stack([ints_to_limbs(list(a)) for _, _, a in scalars]).reshape(count, 8))
    d_rows = torch.zeros((count, gc.STATEMENT_FIELDS, 4), dtype=torch.int64, device=d_s.device)
    d_ha = torch.zeros((count, 8), dtype=torch.int64, device=d_s.device)
    torch.cuda.synchronize()
    ctx.babyjub_mul_batch(d_s.data_ptr(), None, count, d_rows.data_ptr() + AT_O * 32, ROW_WORDS)
    ctx.babyjub_mul_batch(d_h.data_ptr(), d_a.data_ptr(), count, d_ha.data_ptr(), 8)
    d_rows[:, AT_A:AT_A + 2] = d_a.view(count, 2, 4)
    d_rows[:, AT_M] = to_dev(ctx, ints_to_limbs(list(messages)))
    o = d_rows[:, AT_O:AT_O + 2].cpu().numpy().view(np.uint64)
    ha = d_ha.cpu().numpy().view(np.uint64).reshape(count, 2, 4)
    r = [bm.add(tuple(limbs_to_ints(o[j])), bm.neg(tuple(limbs_to_ints(ha[j])))) for j in range(count)]
    d_rows[:, AT_R:AT_R + 2] = to_dev(ctx, np.stack([ints_to_limbs(list(p)) for p in r]))
    torch.cuda.synchronize()
    return d_rows


def run_statement(ctx, case, mg, scalars, messages, flip=None):
    """-> (device witnesses with spare rows, device field rows); flip = (instance, bit of S) changes that bit after O is written"""
    count = len(scalars)
    d_rows = fill_rows(ctx, scalars, messages)
    d_bits = to_dev(ctx, np.stack([packed_bits(s, h) for s, h, _ in scalars]))
    if flip:
        d_bits[flip[0], flip[1] // 8] ^= 1 << (flip[1] % 8)
    d_w = filled(ctx, count, case.c.m)
    mg.run(d_bits.data_ptr(), d_rows.data_ptr(), count, d_w.data_ptr(), in_stride=d_bits.shape[1])
    return d_w, d_rows


@pytest.fixture(scope="module")
def statement(ctx):
    case = gc.statement_case(N_S, N_H)
    assert case.c.mixed_dims()["n_bit_inputs"] == N_S + N_H and case.c.mixed_dims()["n_field_inputs"] == gc.STATEMENT_FIELDS
    qap = case.c.qap_sparse_unity(ctx)
    rng = SplitMix64(2400)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    mg = Mixgen(ctx, case.c)
    messages = [row[AT_M] for row in case.rows]
    d_w, d_rows = run_statement(ctx, case, mg, case.info["scalars"], messages)
    yield case, qap, crs, mg, d_w, d_rows, rng
    mg.close()
    crs.close()
    qap.close()


def test_statement_witnesses_from_the_kernels(ctx, statement):
    case, qap, crs, mg, d_w, d_rows, _ = statement
    count = len(case.rows)
    assert count == 65
    got, spare = split_output(d_w, count)
    rows = d_rows.cpu().numpy().view(np.uint64)
    want_rows = case.mixed_inputs()[1]
    assert np.array_equal(rows, want_rows), first_difference(rows, want_rows)   # O, [h] A from the kernels = the model's
    assert np.array_equal(got, case.want_words()), first_difference(got, case.want_words())
    assert (spare.view(np.uint8) == FILL).all()
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), case.c.m, count)
    assert (res["bad_gates"] == 0).all() and (res["first_bad"] == _lib.QAP_CHECK_NONE).all()
    # the digests: public wires 1 and 2 against the hash kernels over the rows as they lie on the device
    d_ra = d_rows[:, [AT_R, AT_R + 1, AT_A, AT_A + 1]].contiguous()
    d_m = d_rows[:, AT_M].contiguous()
    d_h4 = torch.zeros((count, 4), dtype=torch.int64, device=d_rows.device)
    d_h1 = torch.zeros((count, 4), dtype=torch.int64, device=d_rows.device)
    torch.cuda.synchronize()
    ctx.poseidon_hash_batch(d_ra.data_ptr(), 4, count, d_h4.data_ptr())
    ctx.poseidon_hash_batch(d_m.data_ptr(), 1, count, d_h1.data_ptr())
    assert torch.equal(d_w[:count, 1], d_h4) and torch.equal(d_w[:count, 2], d_h1)


def prove_all(ctx, crs, qap, d_w, m, count, rs, ss):
    ptrs = [d_w.data_ptr() + j * m * 32 for j in range(count)]
    proofs = []
    for first in range(0, count, 64):                       # a batch holds at most ZK_MAX_BATCH = 64 proofs
        n = min(64, count - first)
        ticket = ctx.prove_batch_submit(crs, qap, ptrs[first:first + n], [m] * n, rs[first:first + n], ss[first:first + n])
        proofs += ctx.prove_batch_wait(ticket, n)
    return proofs


def test_statement_proofs_verify_and_equal_the_proofs_of_the_model_witness(ctx, statement):
    case, qap, crs, mg, d_w, d_rows, rng = statement
    count, m = len(case.rows), case.c.m
    rs, ss = [rng.fr() for _ in range(count)], [rng.fr() for _ in range(count)]
    proofs = prove_all(ctx, crs, qap, d_w, m, count, rs, ss)
    public = np.array(case.want_words()[:, 1:3])
    assert ctx.verify_batch(crs, public, proofs).all()
    for j in (0, 63, 64):
        assert proofs[j] == ctx.prove(crs, qap, np.array(case.want_words()[j]), rs[j], ss[j]), j


def test_a_flipped_bit_of_s_breaks_the_first_affine_assertion(ctx, statement):
    case, qap, crs, mg, _, _, _ = statement
    count = len(case.rows)
    messages = [row[AT_M] for row in case.rows]
    d_w, _ = run_statement(ctx, case, mg, case.info["scalars"], messages, flip=(64, 5))
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), case.c.m, count)
    assert [j for j in range(count) if int(res["bad_gates"][j])] == [64]
    affine_x = bm.fixed_gates(N_S) + bm.var_gates(N_H) + 4 + 10 + 1   # behind mul_fixed, mul, assert_on_curve and add: t = Ox Z, then the assertion
    assert affine_x == case.info["affine_x"] and int(res["first_bad"][64]) == affine_x
    assert (res["first_bad"][:64] == _lib.QAP_CHECK_NONE).all()


def test_a_witness_of_another_message_proves_its_own_digest_only(ctx, statement):
    case, qap, crs, mg, d_w, _, rng = statement
    lanes = [0, 63, 64]
    scalars = [case.info["scalars"][j] for j in lanes]
    other = [(case.rows[j][AT_M] + 1) % R for j in lanes]
    d_o, d_rows = run_statement(ctx, case, mg, scalars, other)
    res = ctx.qap_check_dev(qap, d_o.data_ptr(), case.c.m, len(lanes))
    assert (res["bad_gates"] == 0).all()
    rs, ss = [rng.fr() for _ in lanes], [rng.fr() for _ in lanes]
    proofs = prove_all(ctx, crs, qap, d_o, case.c.m, len(lanes), rs, ss)
    own = d_o[:len(lanes), 1:3].cpu().numpy().view(np.uint64)
    original = case.want_words()[lanes, 1:3]
    assert np.array_equal(own[:, 0], original[:, 0]) and not (own[:, 1] == original[:, 1]).all(axis=1).any()   # the same R and A, another M
    assert limbs_to_ints(own[:, 1]) == [case.f.evaluate(case.rows[j][:AT_M] + [mm] + case.rows[j][AT_M + 1:])[2] for j, mm in zip(lanes, other)]
    assert ctx.verify_batch(crs, own, proofs).all()
    assert not ctx.verify_batch(crs, original, proofs).any()
