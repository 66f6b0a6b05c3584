"""Generated structure on the device (tests/generated_circuits.py): every drawn boolean circuit through zk_boolgen_run and
zk_witgen_run against tests/builder_model.py word for word, the drawn field circuits and .zk programs through zk_witgen_run against
the model and the oracle, drawn wire lists through zk_boolgen_eval / _eval_fields, and the device witnesses against the circuits'
own rows (zk_qap_check_dev), before and after one wire of one instance is altered.  The CPU side of the same draws, and the census
that says what they reach, is tests/test_generated_circuits.py."""
import functools

import numpy as np
import pytest
import torch

from zksnark_rs_amd import ZkError, _lib
from zksnark_rs_amd.circuit import Boolgen, Circuit, Witgen, qap_download_dense

import builder_cases as bc
import builder_model as bm
import builder_pack_model as pm
import generated_circuits as gc
from test_gpu_boolgen_pack import random_bits, run_prefilled

pytestmark = pytest.mark.gpu

COUNTS = (1, 64, 65, 130)
BUILT_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
PROGRAM_SEEDS = (1, 2, 3, 4, 5, 6)
TWO = (1, 2)                                                # an even and an odd seed: the two chain patterns
BOOLEAN_SHAPES = ("chain", "wide", "mixed", "packs")
SIZED = [(gc.sized(m), m) for m in gc.SIZED]
BOOLEAN = [(shape, seed) for shape in BOOLEAN_SHAPES for seed in BUILT_SEEDS] + SIZED
BOOLEAN_TWO = [(shape, seed) for shape in BOOLEAN_SHAPES for seed in TWO] + SIZED
PROGRAMS = [(shape, seed) for shape in gc.PROGRAM_SHAPES for seed in PROGRAM_SEEDS]
LIST_LENGTHS = (1, 7, 8, 9, 64, 65)
NONE = _lib.QAP_CHECK_NONE


@functools.lru_cache(maxsize=None)
def built(shape, seed):
    """-> (library Circuit, model Finished, PackModel, inputs of max(COUNTS) instances, the model's witnesses (count, m, 4)): computed
    once per draw, shared by the tests, never written to"""
    c, fin, model = pm.build_both(gc.built_case(shape, seed))
    count = max(COUNTS)
    rows = random_bits(300 + seed, count, c.n_in) if c.boolean else gc.built_inputs(model, 300 + seed, count)
    want = np.stack([bc.words(fin.evaluate(r)) for r in rows])
    want.setflags(write=False)
    return c, fin, model, rows, want


def field_inputs(rows):
    return np.stack([bc.words(r) for r in rows])


def compare_runs(ctx, shape, seed, configs):
    c, fin, model, rows, want = built(shape, seed)
    assert c.boolean
    ins = field_inputs(rows)
    for group_words, expand_form in configs:
        bg = Boolgen(ctx, c, group_words=group_words, expand_form=expand_form)
        for count in COUNTS:
            got = run_prefilled(ctx, bg, c, bc.pack_rows(rows[:count]))              # (the words behind the last witness are checked there)
            assert np.array_equal(got, want[:count]), (group_words, expand_form, count)
        bg.close()
    wg = Witgen(ctx, c)
    for count in COUNTS:
        assert np.array_equal(wg.run_numpy(ins[:count]), want[:count]), count        # the tape kernel: the same array
    wg.close()


# ---- boolean shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", BOOLEAN)
def test_bit_sliced_and_tape_witnesses_equal_the_model(ctx, shape, seed):
    compare_runs(ctx, shape, seed, [(None, None)])


@pytest.mark.parametrize("shape,seed", BOOLEAN_TWO)
def test_group_words_and_the_pair_expansion(ctx, shape, seed):
    compare_runs(ctx, shape, seed, [(1, 0), (8, 0), (1, 1), (8, 1)])


def wire_lists(seed, candidates, must=()):
    """per length a drawn list over `candidates` (witness indices): index 0 is in it, one index is in it twice, and so is one of
    `must` where there is room"""
    d = gc.Draw(seed)
    lists = []
    for n in LIST_LENGTHS:
        wires = [d.pick(candidates) for _ in range(n)]
        zero_at = d.below(n)
        wires[zero_at] = 0
        if n > 1:
            dst = (zero_at + 1 + d.below(n - 1)) % n        # not where the 0 is
            src = (dst + 1 + d.below(n - 1)) % n            # not dst: the list repeats wires[src]
            wires[dst] = wires[src]
            free = [i for i in range(n) if i not in (zero_at, dst, src)]
            if must and free:
                wires[d.pick(free)] = d.pick(list(must))
        assert 0 in wires and (n == 1 or len(set(wires)) < n)
        lists.append(wires)
    return lists


@pytest.mark.parametrize("shape,seed", BOOLEAN_TWO)
def test_named_wires_as_bits_and_as_field_elements(ctx, shape, seed):
    c, fin, model, rows, want = built(shape, seed)
    packed_at = sorted(c.wire_index(w) for w in model.packed)
    bits_at = [i for i in range(c.m) if i not in packed_at]
    bg = Boolgen(ctx, c)
    for wires in wire_lists(400 + seed, bits_at):
        pad = [0] * (-len(wires) % 8)
        for count in COUNTS:
            got = bg.eval_numpy(bc.pack_rows(rows[:count]), wires)
            assert got.shape == (count, (len(wires) + 7) // 8)
            for j in range(count):
                assert bytes(got[j]) == bm.bits_to_bytes([int(want[j, w, 0]) for w in wires] + pad), (len(wires), count, j)
    for wires in wire_lists(500 + seed, list(range(c.m)), packed_at):   # packed wires among them, where the circuit has any
        assert len(wires) == 1 or not packed_at or set(wires) & set(packed_at)
        for count in COUNTS:
            got = bg.eval_fields_numpy(bc.pack_rows(rows[:count]), wires)
            assert np.array_equal(got, want[:count][:, wires, :]), (len(wires), count)
    if packed_at:                                            # refused before any launch
        with pytest.raises(ZkError) as e:
            bg.eval_numpy(bc.pack_rows(rows[:65]), [0, 1, packed_at[-1], 1])
        assert e.value.status == _lib.ZK_ERR_ARG and "packed wire" in str(e.value)
    bg.close()


# ---- the field shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", BUILT_SEEDS)
def test_field_circuits_on_the_tape(ctx, seed):
    c, fin, model, rows, want = built("field", seed)
    assert not c.boolean
    with pytest.raises(ZkError) as e:
        Boolgen(ctx, c)
    assert e.value.status == _lib.ZK_ERR_UNSUPPORTED
    ins = field_inputs(rows)
    wg = Witgen(ctx, c)
    for count in COUNTS:
        assert np.array_equal(wg.run_numpy(ins[:count]), want[:count]), count
    wg.close()


# ---- programs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def parsed(shape, seed):
    code, ast = gc.program(shape, seed)
    rows = gc.program_inputs(ast, 600 + seed, max(COUNTS))
    return code, ast, Circuit(code), rows


@pytest.mark.parametrize("shape,seed", PROGRAMS)
def test_programs_against_the_oracle(ctx, orc, shape, seed):
    code, ast, c, rows = parsed(shape, seed)
    ins = field_inputs(rows)
    want = np.stack([orc.zk_weights(code, ins[j], c.m) for j in range(len(rows))])
    assert np.array_equal(want[3], bc.words(gc.eval_ast(ast, rows[3])))
    wg = Witgen(ctx, c)
    for count in COUNTS:
        assert np.array_equal(wg.run_numpy(ins[:count]), want[:count]), count
    wg.close()
    if c.n <= 40:
        ref = orc.zk_qap_dense(code)
        qap = c.qap(ctx)
        u, v, w, t = qap_download_dense(ctx, qap)
        assert np.array_equal(u, ref["u"]) and np.array_equal(v, ref["v"]) and np.array_equal(w, ref["w"]) and np.array_equal(t, ref["t"])
        qap.close()


# ---- the witnesses against the rows ---------------------------------------------------------------------------------------------
def check_on_device(ctx, c, d_w, count):
    qap = c.qap_sparse(ctx)
    try:
        return ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    finally:
        qap.close()


def alter(d_w, j, index, value):
    """witness j, element `index` := value, on the device"""
    d_w[j, index] = torch.from_numpy(bc.words([value]).view(np.int64)[0]).to(d_w.device)
    torch.cuda.synchronize(d_w.device)


@pytest.mark.parametrize("shape,seed", [(shape, seed) for shape in gc.BUILT_SHAPES for seed in TWO] + SIZED[2:4])
def test_device_witnesses_satisfy_the_rows_until_one_wire_is_altered(ctx, shape, seed):
    c, fin, model, rows, want = built(shape, seed)
    count = 65
    dev = "cuda:%d" % ctx.device
    d_w = torch.zeros((count, c.m, 4), dtype=torch.int64, device=dev)
    if c.boolean:
        d_in = torch.from_numpy(bc.pack_rows(rows[:count])).to(dev)
        gen = Boolgen(ctx, c)
        gen.run(d_in.data_ptr(), count, d_w.data_ptr())
    else:
        d_in = torch.from_numpy(field_inputs(rows[:count]).view(np.int64)).to(dev)
        gen = Witgen(ctx, c)
        gen.run(d_in.data_ptr(), count, d_w.data_ptr())
    res = check_on_device(ctx, c, d_w, count)
    assert not res["bad_gates"].any() and (res["first_bad"] == NONE).all() and not res["flags"].any()
    d = gc.Draw(700 + seed)
    inputs_at = {fin.wit[w] for w in fin.inputs}
    j, index = d.below(count), d.pick([i for i in range(1, c.m) if i not in inputs_at])
    a = fin.evaluate(rows[j])
    a[index] = (a[index] + 1) % bm.R
    alter(d_w, j, index, a[index])
    bad = fin.failing_gates(a)
    assert bad
    res = check_on_device(ctx, c, d_w, count)
    assert (int(res["bad_gates"][j]), int(res["first_bad"][j])) == (len(bad), min(bad))
    others = np.arange(count) != j
    assert not res["bad_gates"][others].any() and (res["first_bad"][others] == NONE).all() and not res["flags"].any()
    gen.close()


def open_gates(ast, values):
    """the gates a program's rows find failing on `values` (a witness, altered or not), from the AST alone: a `*` gate holds where
    the product of its two sides is the target's value; a right-hand side that is no `*` puts nothing on u or v, so its gate reads
    0 * 0 = v and holds only where v is 0 (the reference accepts such a program without a word).  On the program's own witness
    every `*` gate holds and only gates of the second kind are open."""
    env = dict(zip(gc.variable_order(ast), values[1:]))

    def ev(e):
        if e[0] == "lit":
            return e[1] % bm.R
        if e[0] == "var":
            return env[e[1]]
        return ev(e[1]) * ev(e[2]) % bm.R if e[0] == "mul" else sum(ev(k) for k in e[1]) % bm.R

    return [k for k, (v, e) in enumerate(ast["program"]) if (ev(e) if e[0] == "mul" else 0) != env[v]]


@pytest.mark.parametrize("shape,seed", [(shape, seed) for shape in gc.PROGRAM_SHAPES for seed in TWO])
def test_program_witnesses_against_the_rows(ctx, shape, seed):
    code, ast, c, rows = parsed(shape, seed)
    count = 65
    dev = "cuda:%d" % ctx.device
    d_in = torch.from_numpy(field_inputs(rows[:count]).view(np.int64)).to(dev)
    d_w = torch.zeros((count, c.m, 4), dtype=torch.int64, device=dev)
    wg = Witgen(ctx, c)
    wg.run(d_in.data_ptr(), count, d_w.data_ptr())
    res = check_on_device(ctx, c, d_w, count)
    assert not res["flags"].any()
    values = [gc.eval_ast(ast, rows[j]) for j in range(count)]
    for j in range(count):
        bad = open_gates(ast, values[j])
        assert all(ast["program"][k][1][0] != "mul" for k in bad)
        assert (int(res["bad_gates"][j]), int(res["first_bad"][j])) == (len(bad), min(bad) if bad else NONE), j
    # one gate output of one instance, off by one: its own gate and every gate that reads it fail as well
    d = gc.Draw(800 + seed)
    order = gc.variable_order(ast)
    gates = [k for k, (v, e) in enumerate(ast["program"]) if e[0] == "mul"]
    j, k = d.below(count), d.pick(gates)
    index = 1 + order.index(ast["program"][k][0])
    altered = list(values[j])
    altered[index] = (altered[index] + 1) % bm.R
    alter(d_w, j, index, altered[index])
    bad = open_gates(ast, altered)
    assert k in bad and len(bad) > len(open_gates(ast, values[j]))
    res = check_on_device(ctx, c, d_w, count)
    assert (int(res["bad_gates"][j]), int(res["first_bad"][j])) == (len(bad), min(bad))
    others = np.arange(count) != j
    for i in np.flatnonzero(others):
        was = open_gates(ast, values[i])
        assert (int(res["bad_gates"][i]), int(res["first_bad"][i])) == (len(was), min(was) if was else NONE), i
    assert not res["flags"].any()
    wg.close()
