"""-m "not gpu": zk_builder_pack (host code, no context) against the Python-integer model of tests/builder_pack_model.py: rows (U
entries 2^i, V the constant 1, W the output), dimensions and witness order, both host evaluators word for word, which circuits stay
bit-sliceable, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import builder_cases as bc
import builder_model as bm
import builder_pack_model as pm
from zksnark_rs_amd import SplitMix64, _lib, limbs_to_ints
from zksnark_rs_amd.circuit import BuildErr, Builder, Circuit

R = bm.R


def agree(circuit, model, inputs, failing=()):
    """both evaluators == the model, word for word; the witness satisfies every gate in Python integers (but `failing`)"""
    a = limbs_to_ints(circuit.weights(bc.words(inputs)))
    b = limbs_to_ints(circuit.weights_tape(bc.words(inputs)))
    assert a == b, "the two host evaluators differ"
    assert a == model.evaluate(inputs)
    assert model.failing_gates(a) == list(failing)
    return a


def input_sets(n_in, seed, extra=3):
    rng = SplitMix64(seed)
    return [[0] * n_in, [1] * n_in] + [[rng.next() & 1 for _ in range(n_in)] for _ in range(extra)]


# ---- rows, dimensions, witness order, values -----------------------------------------------------------
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("width", pm.WIDTHS)
def test_one_pack_rows_and_values(width, verify):
    circuit, model, full = pm.build_both(pm.one_pack(width, verify))
    bc.same_shape(circuit, model)
    assert (circuit.n, circuit.m, circuit.n_in, circuit.input) == (1, width + 2, width, 1)
    assert circuit.boolean and full.boolean() and circuit.packed_wires == 1
    packed = width + 2                                     # the wire made after the two constants and `width` inputs
    at = circuit.wire_index(packed)
    assert at == (1 if verify else width + 1)              # first witness index as a verify wire, last otherwise
    # the rows spelled out: U of operand i has the one entry (gate 0, 2^i), V is the constant alone, W the output alone
    ptr, gate, val = bc.lib_rows(circuit, 0)
    assert gate == [0] * width
    assert sorted(val) == [1 << i for i in range(width)]
    for i in range(width):
        row = circuit.wire_index(2 + i)
        assert val[ptr[row]:ptr[row + 1]] == [1 << i]
    assert bc.lib_rows(circuit, 1) == ([0] + [1] * (width + 2), [0], [1])
    ptr, gate, val = bc.lib_rows(circuit, 2)
    assert (gate, val) == ([0], [1]) and ptr[at] == 0 and ptr[at + 1] == 1
    for bits in input_sets(width, 300 + width):
        w = agree(circuit, model, bits)
        assert w[at] == pm.pack_value(bits)
    assert agree(circuit, model, [1] * width)[at] == (1 << width) - 1      # 2^253 - 1 at the cap: below r, nothing reduced
    assert (1 << pm.PACK_MAX_BITS) - 1 < R


def test_mixed_operands_constants_and_repeats():
    circuit, model, full = pm.build_both(pm.mixed_operands)
    bc.same_shape(circuit, model)
    assert circuit.boolean and full.boolean() and circuit.packed_wires == 3 and circuit.input == 4
    # the zero wire's entries are gone: the 11-operand pack has 9 U entries, the pack of the zero wire alone has none
    _, gate_u, _ = bc.lib_rows(circuit, 0)
    n = circuit.n
    assert gate_u.count(n - 3) == 9 and gate_u.count(n - 2) == 0 and gate_u.count(n - 1) == 2
    for v in range(64):
        x = bm.bits_of(v, 6)
        w = agree(circuit, model, x)
        assert w[1] == pm.mixed_value(x) and w[3] == 0 and w[4] == 3


def test_all_widths_circuit():
    circuit, model, full = pm.build_both(pm.all_widths)
    bc.same_shape(circuit, model)
    assert circuit.boolean and full.boolean() and circuit.packed_wires == 11
    assert circuit.n == 300 + 11 and circuit.m == 1 + 40 + 300 + 11
    for bits in input_sets(40, 310):
        w = agree(circuit, model, bits)
        assert w[3] == pm.pack_value(bits)                 # the pack directly over the inputs
        assert w[-1] & 2                                   # the last wire is the last pack: its bit 1 is the constant 1


def test_digest_as_two_field_elements():
    circuit, model, full = pm.build_both(pm.digest_packed(7, 1))
    bc.same_shape(circuit, model)
    assert circuit.input == 2 and circuit.boolean and circuit.packed_wires == 2
    assert circuit.n == 8 * 7 + 16 + 9664 + 2
    msg = b"\x00\xffkecca"
    w = agree(circuit, model, bm.bytes_to_bits(msg))
    digest = bm.sponge(msg, 136, 0x06, 1, 32)
    assert w[1:3] == [int.from_bytes(digest[:16], "little"), int.from_bytes(digest[16:], "little")]


def test_pack_bytes_facade():
    b = Builder()
    msg = b.new_word8_vec(3)
    digest = b.keccak(msg, 136, 0x06, 1, 32)
    two = b.pack_bytes(digest)
    four = b.pack_bytes(digest, bytes_per_element=8)
    assert len(two) == 2 and len(four) == 4
    with pytest.raises(BuildErr):
        b.pack_bytes(digest[0][:7])
    with pytest.raises(BuildErr, match="n_bits"):
        b.pack_bytes(digest, bytes_per_element=32)         # 256 bits do not fit one element
    circuit = b.finish(two + four)
    assert circuit.input == 6 and circuit.packed_wires == 6 and circuit.boolean
    inputs = np.zeros((24, 4), np.uint64)
    inputs[:, 0] = bm.bytes_to_bits(b"abc")
    w = limbs_to_ints(circuit.weights(inputs))
    d = bm.sponge(b"abc", 136, 0x06, 1, 32)
    assert w[1:3] == [int.from_bytes(d[16 * k:16 * k + 16], "little") for k in range(2)]
    assert w[3:7] == [int.from_bytes(d[8 * k:8 * k + 8], "little") for k in range(4)]


# ---- classification ---------------------------------------------------------------------------------------
def packed_into(consumer):
    def case(b):
        xs = b.new_bits(4)
        p = b.pack(xs[:3])
        consumer(b, p, xs)
        return [p]
    return case


CONSUMERS = {
    "and": lambda b, p, xs: b.gate("and", p, xs[3]),
    "not": lambda b, p, xs: b.gate("not", p),
    "pack": lambda b, p, xs: b.pack([xs[3], p]),
    "assert_bit": lambda b, p, xs: b.assert_bit(p),
    "compare": lambda b, p, xs: b.compare("is_equal", [xs[0], p], [xs[1], xs[2]]),
    "keccak": lambda b, p, xs: b.keccak([p] + xs + xs[:3], 136, 0x06, 1, 1),
    "sub_circuit": lambda b, p, xs: b.sub_circuit([(1, p)], [(1, xs[0])]),
}


@pytest.mark.parametrize("name", list(CONSUMERS))
def test_a_packed_wire_that_is_read_sends_the_circuit_to_the_tape(name):
    circuit, model, full = pm.build_both(packed_into(CONSUMERS[name]))
    bc.same_shape(circuit, model)                          # legal: rows and evaluators as for any general sub-circuit
    assert not circuit.boolean and (name == "sub_circuit" or not full.boolean())
    assert circuit.packed_wires == (2 if name == "pack" else 1)
    for v in range(16):
        # the assertion on a packed wire is a real constraint: gate 1 fails exactly where the packed value is no bit
        agree(circuit, model, bm.bits_of(v, 4), failing=[1] if name == "assert_bit" and v & 7 > 1 else [])


def test_pack_over_a_field_input_or_a_general_sub_circuit_is_not_boolean():
    def over_field(b):
        x = b.new_field()
        y = b.new_bits(1)[0]
        return [b.pack([y, x])]
    circuit, model, full = pm.build_both(over_field)
    bc.same_shape(circuit, model)
    assert not circuit.boolean and not full.boolean() and circuit.packed_wires == 1
    assert agree(circuit, model, [12345, 1])[1] == 1 + 2 * 12345

    def over_general(b):
        x, y = b.new_bits(2)
        t = b.sub_circuit([(3, x)], [(1, y)])
        return [b.pack([t, y])]
    circuit, model, _ = pm.build_both(over_general)
    bc.same_shape(circuit, model)
    assert not circuit.boolean and circuit.packed_wires == 1
    assert agree(circuit, model, [1, 1])[1] == 3 + 2


def test_existing_circuits_have_no_packed_wires_and_classify_as_before():
    for case, boolean in ((bc.all_gates, True), (bc.comparator("less_than_eq", 8), True), (bc.keccak_case(3, 136, 0x06, 1), True),
                          (bc.odd_inputs, True), (bc.sized(64), True), (bc.not_chain(5), True), (bc.wide_level(9), True)):
        circuit, _ = bc.build_both(case)
        assert circuit.packed_wires == 0 and circuit.boolean == boolean
    parsed = Circuit("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n")
    assert parsed.packed_wires == 0 and not parsed.boolean
    lib = bc.Lib()
    x, y = lib.new_bits(2)
    general = lib.finish([lib.sub_circuit([(1, x), (2, y)], [(1, bm.ONE)])])      # the pack's shape by hand stays on the tape
    assert general.packed_wires == 0 and not general.boolean


# ---- refusals -------------------------------------------------------------------------------------------------
def refusal(fn, text):
    with pytest.raises(BuildErr, match=text) as e:
        fn()
    assert e.value.status == _lib.ZK_ERR_ARG


def test_refusals():
    b = Builder()
    xs = b.new_bits(254)
    refusal(lambda: b.pack([]), r"n_bits must be in 1\.\.253, got 0")
    refusal(lambda: b.pack(xs), r"n_bits must be in 1\.\.253, got 254")
    refusal(lambda: b.pack([xs[0], 999]), "unknown wire id 999")
    assert b.dims() == (256, 0)                            # nothing was added by a refused call
    p = b.pack(xs[:253])
    assert p == 256 and b.dims() == (257, 1)
    circuit = b.finish([p])
    refusal(lambda: b.pack(xs[:2]), "finished")
    assert circuit.packed_wires == 1 and circuit.boolean
    lib = _lib.load()
    out = C.c_uint32()
    one = np.array([2], np.uint32)
    assert lib.zk_builder_pack(None, one.ctypes.data_as(_lib.u32p), 1, C.byref(out)) == _lib.ZK_ERR_ARG
    b2 = Builder()
    b2.new_bits(1)
    assert lib.zk_builder_pack(b2.ptr, one.ctypes.data_as(_lib.u32p), 1, None) == _lib.ZK_ERR_ARG
    assert lib.zk_builder_pack(b2.ptr, None, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_circuit_packed_wires(None, C.byref(C.c_size_t())) == _lib.ZK_ERR_ARG
    assert lib.zk_circuit_packed_wires(circuit.ptr, None) == _lib.ZK_ERR_ARG
