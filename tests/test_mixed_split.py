"""The split of a built circuit into a boolean core and a field tail (zk_circuit_mixed_dims) and its host runner
(zk_circuit_weights_mixed): host code, no GPU.  The dimensions are held against a classification restated in Python
(tests/mixed_model.py), the witnesses against zk_circuit_weights and the integer model word for word."""
import numpy as np
import pytest

import builder_model as bm
import builder_pack_model as pm
import generated_circuits as gc
import mixed_model as mm
from zksnark_rs_amd import _lib, ints_to_limbs
from zksnark_rs_amd.circuit import ParseErr, Circuit

R = bm.R
SEEDS = (0, 1, 2, 3, 4)


def build(case):
    """-> (library Circuit, model Finished, the SplitModel)"""
    lib, model = pm.PackLib(), mm.SplitModel()
    v_lib, v_model = case(lib), case(model)
    assert list(v_lib) == list(v_model)
    return lib.finish(v_lib), model.finish(v_model), model


def check_rows(c, fin, model, rows):
    for row in rows:
        bits, fields = mm.split_inputs(model, row)
        got = c.weights_mixed(bits, fields)
        want = c.weights(row)
        assert np.array_equal(got, want)
        assert np.array_equal(got, ints_to_limbs(fin.evaluate(row)))


@pytest.mark.parametrize("shape", gc.BUILT_SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_generated_circuits_split_and_run(shape, seed):
    case = gc.built_case(shape, seed)
    c, fin, model = build(case)
    dims = c.mixed_dims()
    assert dims == mm.mixed_shape(model, fin)
    assert dims["n_bit_inputs"] + dims["n_field_inputs"] == c.n_in
    if c.boolean:
        with_out = sum(1 for _, _, o in model.subs if o is not None) - len(model.packed)
        assert dims["tail_ops"] == 0 and dims["tail_slots"] == 0 and dims["tail_levels"] == 0
        assert dims["core_ops"] == with_out                  # one boolean operation per sub-circuit: the tape of zk_boolgen_*
        assert dims["core_levels"] == max(model.level)
    else:
        assert dims["tail_ops"] > 0
    if shape == "field":
        assert dims["n_field_inputs"] >= 2 and "tail" in model.cat
    check_rows(c, fin, model, gc.built_inputs(model, 77 + seed, 6))


def test_boolean_shapes_are_boolean_and_field_is_not():
    assert all(build(gc.built_case(s, 1))[0].boolean for s in ("chain", "wide", "mixed", "packs"))
    assert not build(gc.built_case("field", 1))[0].boolean


def test_no_boolean_operation_at_all():
    def case(b):
        x, y = b.new_field(), b.new_field()
        t = b.sub_circuit([(3, x), (R - 1, y)], [(1, y), (5, bm.ONE)])
        u = b.sub_circuit([(1, t)], [(1, t)])
        return [u]
    c, fin, model = build(case)
    d = c.mixed_dims()
    assert (d["n_bit_inputs"], d["core_ops"], d["core_levels"]) == (0, 0, 0) and d["tail_ops"] > 0 and d == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[0, 0], [1, 1], [R - 1, R - 1], [12345, R - 2]])


def test_tail_over_bit_wires_only():
    """a general sub-circuit whose operands are all bit-class, weights 0, 1, r - 1 and (r - 1) / 2"""
    def case(b):
        x = b.new_bits(5)
        g = b.gate("xor", x[0], x[1])
        n = b.gate("nand", x[2], g)
        t = b.sub_circuit([(0, x[0]), (1, g), (R - 1, n), ((R - 1) // 2, x[3])], [(1, x[4]), ((R - 1) // 2, bm.ONE), (1, bm.ZERO)])
        return [t, g]
    c, fin, model = build(case)
    d = c.mixed_dims()
    assert d["n_field_inputs"] == 0 and d["core_ops"] == 3 and d["tail_slots"] >= 1 and d == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[(k >> i) & 1 for i in range(5)] for k in range(32)])


@pytest.mark.parametrize("width", (1, 63, 64, 65, 128, 253))
def test_pack_read_by_the_tail(width):
    def case(b):
        x = b.new_bits(width)
        f = b.new_field()
        p = b.pack(x)
        t = b.sub_circuit([(1, p), (7, f)], [(1, p)])
        u = b.sub_circuit([(2, p)], [(1, t)])               # a second reader: the pack is copied once
        return [u, p]
    c, fin, model = build(case)
    d = c.mixed_dims()
    assert model.cat == ["cpack", "tail", "tail"] and d == mm.mixed_shape(model, fin)
    rows = [[0] * width + [0], [1] * width + [R - 1], [i % 2 for i in range(width)] + [3], [0] * (width - 1) + [1, 9]]
    check_rows(c, fin, model, rows)


def test_pack_with_one_field_class_operand_is_a_tail_operation():
    def case(b):
        x = b.new_bits(4)
        f = b.new_field()
        g = b.gate("and", x[0], f)                          # field-class: it reads a field input
        p = b.pack([x[1], g, x[2], bm.ONE, bm.ZERO, x[3]])
        q = b.pack([x[1], x[2]])
        return [p, q]
    c, fin, model = build(case)
    assert model.cat == ["tail", "tail", "cpack"]
    d = c.mixed_dims()
    assert d["core_ops"] == 0 and d == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[1, 1, 0, 1, 1], [1, 0, 1, 1, 0], [0, 1, 1, 0, R - 1], [1, 1, 1, 1, 5]])


@pytest.mark.parametrize("kind", bm.GATE_KINDS)
def test_boolean_gate_with_a_field_operand(kind):
    """compiled from the sub-circuit's terms, not from its boolean kind: on a field operand XOR is (x - y)(x - y)"""
    def case(b):
        x = b.new_bits(2)
        f = b.new_field()
        outs = [b.gate(kind, f, None if kind in bm.UNARY else x[0])]
        if kind not in bm.UNARY:
            outs += [b.gate(kind, x[1], f), b.gate(kind, f, f)]
        outs.append(b.gate(kind, x[0], None if kind in bm.UNARY else x[1]))   # and one that stays in the core
        return outs[:1]
    c, fin, model = build(case)
    d = c.mixed_dims()
    assert d["core_ops"] == len(bm.GATES[kind]) and d == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[a, b, f] for a in (0, 1) for b in (0, 1) for f in (0, 1, 2, R - 1, (R - 1) // 2)])


def test_bit_check_and_assert_bit_on_a_field_wire():
    def case(b):
        x = b.new_bits(1)
        f = b.new_field()
        t = b.sub_circuit([(1, f)], [(1, x[0]), (1, bm.ONE)])
        chk = b.gate("bit_checker", t)
        b.assert_bit(t)
        b.assert_bit(f)
        return [chk]
    c, fin, model = build(case)
    assert model.cat == ["tail", "tail", "assert", "assert"] and c.mixed_dims() == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[0, 0], [1, 1], [0, 1], [1, 7], [1, R - 1]])   # assertions compute nothing, on any value


def test_field_input_that_nothing_reads_and_r_minus_one():
    def case(b):
        x = b.new_bits(3)
        f, unread = b.new_field(), b.new_field()
        g = b.gate("or", x[0], x[1])
        t = b.sub_circuit([(1, f), (1, g)], [(1, f), (1, x[2])])
        return [t, unread]
    c, fin, model = build(case)
    d = c.mixed_dims()
    assert d["n_field_inputs"] == 2 and d == mm.mixed_shape(model, fin)
    check_rows(c, fin, model, [[1, 0, 1, R - 1, R - 1], [0, 0, 0, 0, 5], [1, 1, 1, 2, 0]])
    bits, _ = mm.split_inputs(model, [1, 0, 1, 0, 0])
    for bad in ([R, 1], [1, R], [1, (1 << 256) - 1]):
        f = np.array([[(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)] for v in bad], np.uint64)
        with pytest.raises(ParseErr, match="input value >= r"):
            c.weights_mixed(bits, f)
        out = np.zeros((c.m, 4), np.uint64)
        rc = c.lib.zk_circuit_weights_mixed(c.ptr, bits, len(bits), f.ctypes.data_as(_lib.u64p), 2, out.ctypes.data_as(_lib.u64p), c.m)
        assert rc == _lib.ZK_ERR_RANGE


def test_wrong_counts_and_parsed_circuits():
    c, fin, model = build(gc.built_case("field", 3))
    row = gc.built_inputs(model, 1, 3)[2]
    bits, fields = mm.split_inputs(model, row)
    f = ints_to_limbs(fields)
    out = np.zeros((c.m + 1, 4), np.uint64)

    def call(bits, n_fields, m):
        rc = c.lib.zk_circuit_weights_mixed(c.ptr, bits, len(bits), f.ctypes.data_as(_lib.u64p), n_fields, out.ctypes.data_as(_lib.u64p), m)
        return rc, c.lib.zk_circuit_last_error(c.ptr).decode()

    assert call(bits, len(fields), c.m) == (0, "")
    assert call(bits + b"\0", len(fields), c.m) == (_lib.ZK_ERR_ARG, "StructureErr(None, Wrong number of values supplied)")
    assert call(bits[:-1], len(fields), c.m) == (_lib.ZK_ERR_ARG, "StructureErr(None, Wrong number of values supplied)")
    assert call(bits, len(fields) - 1, c.m) == (_lib.ZK_ERR_ARG, "StructureErr(None, Wrong number of values supplied)")
    assert call(bits, len(fields), c.m + 1) == (_lib.ZK_ERR_ARG, "StructureErr(None, weights buffer size mismatch)")
    parsed = Circuit("(in a b) (out c) (verify c) (program (= c (* a b)))")
    assert parsed.lib.zk_circuit_mixed_dims(parsed.ptr, *[None] * 7) == _lib.ZK_ERR_UNSUPPORTED
    with pytest.raises(ParseErr):
        parsed.mixed_dims()
    o = np.zeros((parsed.m, 4), np.uint64)
    two = ints_to_limbs([2, 3])
    assert parsed.lib.zk_circuit_weights_mixed(parsed.ptr, None, 0, two.ctypes.data_as(_lib.u64p), 2, o.ctypes.data_as(_lib.u64p),
                                               parsed.m) == _lib.ZK_ERR_UNSUPPORTED
