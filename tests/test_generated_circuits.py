"""Generated structure on the host (tests/generated_circuits.py): every drawn built circuit through the library's Builder and through
tests/builder_model.py, every drawn .zk program through the parser, the oracle's restatement (oracle/zkparse.hpp) and eval_ast; both
host evaluators and both tape compilers' counts against them; and a census, which asserts that the draws reach what the fixed cases
of builder_cases.py / witgen_cases.py do not.  Equality of integers and of 64-bit words throughout."""
import ctypes as C
import functools

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd.circuit import Circuit, ParseErr

import builder_cases as bc
import builder_model as bm
import builder_pack_model as pm
import generated_circuits as gc
import witgen_cases as wc

BUILT_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
PROGRAM_SEEDS = (1, 2, 3, 4, 5, 6)
BUILT = [(shape, seed) for shape in gc.BUILT_SHAPES for seed in BUILT_SEEDS] + [(gc.sized(m), m) for m in gc.SIZED]
PROGRAMS = [(shape, seed) for shape in gc.PROGRAM_SHAPES for seed in PROGRAM_SEEDS]


@functools.lru_cache(maxsize=None)
def built(shape, seed):
    """-> (case, library Circuit, model Finished, the PackModel); build_both asserts that the two builders number wires alike"""
    case = gc.built_case(shape, seed)
    circuit, fin, model = pm.build_both(case)
    return case, circuit, fin, model


@functools.lru_cache(maxsize=None)
def parsed(shape, seed):
    code, ast = gc.program(shape, seed)
    return code, ast, Circuit(code)


def test_draws_depend_on_shape_and_seed_alone():
    assert gc.built_case("mixed", 3).plan == gc.built_case("mixed", 3).plan != gc.built_case("mixed", 4).plan
    assert gc.built_case("mixed", 3).verify == gc.built_case("mixed", 3).verify
    assert gc.program("mixed", 3)[0] == gc.program("mixed", 3)[0] != gc.program("mixed", 4)[0]


# ---- built circuits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", BUILT)
def test_built_circuit_against_the_model(shape, seed):
    case, c, fin, model = built(shape, seed)
    bc.same_shape(c, fin)
    assert c.boolean == model.boolean() == (shape != "field")
    assert c.packed_wires == len(model.packed)
    for ins in gc.built_inputs(model, 100 + seed, 3):
        want = fin.evaluate(ins)
        assert fin.failing_gates(want) == []
        words = bc.words(want)
        assert np.array_equal(c.weights(ins), words)
        assert np.array_equal(c.weights_tape(ins), words)
    ops, slots, consts = gc.built_tape_shape(fin)[:3]
    d = c.tape_dims()
    assert (d["ops"], d["slots"], d["consts"]) == (ops, slots, consts)        # the compiler's temporaries and its constant pool


# ---- programs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", PROGRAMS)
def test_program_against_the_oracle_and_eval_ast(orc, shape, seed):
    code, ast, c = parsed(shape, seed)
    dims = [C.c_size_t() for _ in range(4)]
    assert orc.lib.orc_zk_dims(code.encode(), *[C.byref(x) for x in dims]) == 0
    assert (c.m, c.n, c.input, c.n_in) == tuple(x.value for x in dims)
    assert (c.n, c.n_in, c.input) == (len(ast["program"]), len(ast["ins"]), len(ast["verify"]))
    assert 40 <= c.n <= 300
    for ins in gc.program_inputs(ast, 200 + seed, 3 + 3):
        a = zk.ints_to_limbs(ins)
        want = bc.words(gc.eval_ast(ast, ins))
        assert want.shape == (c.m, 4)
        assert np.array_equal(orc.zk_weights(code, a, c.m), want)
        assert np.array_equal(c.weights(a), want)
        assert np.array_equal(c.weights_tape(a), want)
    ops, slots, consts = gc.program_tape_shape(ast)[:3]
    d = c.tape_dims()
    assert (d["ops"], d["slots"], d["consts"]) == (ops, slots, consts)
    assert (d["depth"], d["width"]) == wc.assignment_shape(code)[1:]


def test_an_empty_sum_cannot_be_written(orc):
    """`(+)` is one word to the tokenizer, which refuses an operator inside a word: the generator cannot draw it"""
    code = "(in a) (out b c) (verify b) (program (= c (+)) (= b (* a a)))"
    with pytest.raises(ParseErr) as e:
        Circuit(code)
    assert "SyntaxErr(1, unexpected operator)" in str(e.value)
    assert orc.lib.orc_zk_dims(code.encode(), *[C.byref(C.c_size_t()) for _ in range(4)]) != 0


# ---- the census -------------------------------------------------------------------------------------------------------------
def gate_classes():
    """kind -> the union of operand classes over every gate of every generated built circuit"""
    seen = {k: set() for k in bm.GATE_KINDS}
    for shape, seed in BUILT:
        for kind, classes in built(shape, seed)[0].census["gates"]:
            seen[kind] |= classes
    return seen


def test_census_gates():
    seen = gate_classes()
    for kind in bm.GATE_KINDS:
        if kind in bm.UNARY:
            # One operand: "two inputs" and x == y do not exist, and the gate sits exactly one level above its operand, so an
            # operand 8 levels older cannot exist either.  What is left of the list: an input, either constant, an output.
            assert {"input", "zero", "one", "output"} <= seen[kind] and "old" not in seen[kind], kind
        else:
            assert {"two_inputs", "zero", "one", "same", "old"} <= seen[kind], kind
    compares = [x for shape, seed in BUILT for x in built(shape, seed)[0].census["compare"]]
    for kind in bm.CMP_KINDS:
        bits = {n for k, n in compares if k == kind}
        assert 1 in bits and max(bits) >= 5, kind
    fan_in = {n for shape, seed in BUILT for n in built(shape, seed)[0].census["fan_in"]}
    assert 1 in fan_in and max(fan_in) >= 5


def test_census_sides():
    subs = [s for shape, seed in BUILT for s in built(shape, seed)[2].subs]
    assert any(l == [] or r == [] for l, r, _ in subs)                          # empty once the zero wire is dropped
    assert any(side and all(i == 0 for _, i in side) for l, r, _ in subs for side in (l, r))      # constants only
    assert any(l == r and len(l) == 2 and {c for c, _ in l} == {1, bm.R - 1} for l, r, _ in subs)  # an XOR: the sides repeat
    general = [s for seed in BUILT_SEEDS for s in built("field", seed)[2].subs]
    weights = {c for l, r, _ in general for c, _ in l + r}
    assert {1, bm.R - 1, (bm.R - 1) // 2, 0} <= weights and len(weights) > 20
    assert any(l == [] for l, _, _ in general) and any(r == [] for _, r, _ in general)
    for seed in BUILT_SEEDS:
        assert {1, 63, 64, 65, 128, 253} <= set(built("packs", seed)[0].census["packs"])


def test_census_shapes():
    for seed in BUILT_SEEDS:
        case, c, fin, model = built("wide", seed)
        assert case.census["wide"] > 1024 and case.census["wide"] % 64
        assert 200 <= built("chain", seed)[0].census["subs"] <= 400
        for shape, lo, hi in (("mixed", 300, 600), ("packs", 300, 600), ("field", 150, 300)):
            assert lo <= built(shape, seed)[0].census["subs"] <= hi, (shape, seed)
        for shape in ("mixed", "packs", "field"):
            census = built(shape, seed)[0].census
            assert 10 * census["old_operands"] >= census["operands"], (shape, seed)
    chains = [built("chain", seed)[1].tape_dims() for seed in BUILT_SEEDS]
    assert 2 * sum(d["width"] == 1 for d in chains) >= len(chains)
    assert all(d["depth"] >= 128 for d in chains)              # (assertions and the (older, older) pattern add no level)
    for m in gc.SIZED:
        assert built(gc.sized(m), m)[1].m == m
    for seed in PROGRAM_SEEDS:
        d = parsed("wide", seed)[2].tape_dims()
        assert d["depth"] == 1 and d["width"] >= 300
    assert sum(parsed(shape, seed)[2].n <= 40 for shape, seed in PROGRAMS) >= 2   # what the dense QAP comparison on the device takes


def test_census_tapes():
    """ops / levels is the mean that picks the tape kernel's wave count: W = 1 at <= 1, 2 in (1, 2], 4 above.  The level count is
    the restatement's (generated_circuits.*_tape_shape): the library exposes operations, slots and constants, which the two tests
    above compare on every draw, but neither its tape levels nor W."""
    means = [(lambda s: s[0] / s[3])(gc.built_tape_shape(built(shape, seed)[2])) for shape, seed in BUILT]
    means += [(lambda s: s[0] / s[3])(gc.program_tape_shape(parsed(shape, seed)[1])) for shape, seed in PROGRAMS]
    assert any(x <= 1 for x in means) and any(1 < x <= 2 for x in means) and any(x > 2 for x in means)
    for shape, seed in PROGRAMS:
        code, ast, c = parsed(shape, seed)
        lits = gc.literals(ast)
        assert c.tape_dims()["consts"] == len(set(lits)) < len(lits)                # the pool de-duplicates
        assert {0, 1, bm.R - 1, gc.BIG_LITERAL % bm.R} & set(lits)
        assert "unread" in ast["ins"] and "unread" not in code[code.index("(verify"):]
        if "late" in ast["ins"]:                             # first read where no wire is made, a wire all the same
            first = next(i for i, (v, e) in enumerate(ast["program"]) if "late" in gc.variables(e))
            assert ast["program"][first][1][0] == "add" and ast["program"][first + 1][0] == "pub"
    lits = {x for shape, seed in PROGRAMS for x in gc.literals(parsed(shape, seed)[1])}
    assert {0, 1, bm.R - 1, gc.BIG_LITERAL % bm.R} <= lits
