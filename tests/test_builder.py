"""-m "not gpu": the gate-level circuit builder (zk_builder_*, host code, no context) against the Python-integer model of
tests/builder_model.py: rows and dimensions, both host evaluators word for word, every witness against its rows, Keccak digests read
off the witness against hashlib and known vectors, the witness order and every refusal."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import builder_cases as bc
import builder_model as bm
from zksnark_rs_amd import SplitMix64, _lib, limbs_to_ints
from zksnark_rs_amd.circuit import BuildErr, Builder, Circuit, ParseErr

R = bm.R
DOC_INPUT = bytes([150, 234, 20, 196, 120, 146, 1, 48, 157, 10, 170, 174, 183, 246, 34, 204, 110, 184, 31, 155, 70, 130, 115, 205, 179, 165, 27,
                   165, 104, 31, 7, 16, 157, 242, 34, 232, 56, 161, 8, 150, 228, 129, 153, 41, 144, 186, 190, 41, 16, 59, 242, 109, 102, 75, 12, 246])
DOC_DIGEST = bytes([65, 231, 91, 68, 62, 80, 71, 123, 164, 102, 65, 50, 133, 1, 30, 28, 212, 25, 134, 124, 67, 29, 5, 47, 16, 36, 248, 235, 214,
                    168, 145, 209])          # builder/mod.rs:1405-1425


def both_evaluators(circuit, inputs):
    a = limbs_to_ints(circuit.weights(bc.words(inputs)))
    b = limbs_to_ints(circuit.weights_tape(bc.words(inputs)))
    assert a == b, "the two host evaluators differ"
    return a


def agree(circuit, model, inputs):
    """both evaluators == the model, word for word; the witness satisfies every gate in Python integers"""
    got = both_evaluators(circuit, inputs)
    assert got == model.evaluate(inputs)
    assert model.failing_gates(got) == []
    return got


# ---- rows and dimensions -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bm.GATE_KINDS)
def test_each_gate_rows_and_truth_table(kind):
    circuit, model = bc.build_both(bc.one_gate(kind))
    bc.same_shape(circuit, model)
    assert circuit.n == len(bm.GATES[kind]) and circuit.boolean
    for x in (0, 1):
        for y in (0, 1):
            w = agree(circuit, model, [x, y])
            assert w[1] == bm.TRUTH[kind](x, y), (kind, x, y)


def test_all_gates_circuit():
    circuit, model = bc.build_both(bc.all_gates)
    bc.same_shape(circuit, model)
    assert circuit.boolean and circuit.input == 3 and circuit.n_in == 4
    for v in range(16):
        agree(circuit, model, bm.bits_of(v, 4))


@pytest.mark.parametrize("bits", [1, 3, 8, 64])
@pytest.mark.parametrize("kind", bm.CMP_KINDS)
def test_comparator_rows(kind, bits):
    circuit, model = bc.build_both(bc.comparator(kind, bits))
    bc.same_shape(circuit, model)
    assert circuit.boolean


@pytest.mark.parametrize("kind", bm.CMP_KINDS)
def test_comparator_three_bits_exhaustive(kind):
    circuit, model = bc.build_both(bc.comparator(kind, 3))
    one_sided = kind == "is_equal_zero"
    for l in range(8):
        for r in ([0] if one_sided else range(8)):
            w = agree(circuit, model, bm.bits_of(l, 3) + ([] if one_sided else bm.bits_of(r, 3)))
            assert w[1] == int(bm.CMP_TRUTH[kind](l, r)), (kind, l, r)


@pytest.mark.parametrize("kind", bm.CMP_KINDS)
def test_comparator_sixty_four_bits_at_the_edges(kind):
    circuit, model = bc.build_both(bc.comparator(kind, 64))
    one_sided = kind == "is_equal_zero"
    top, full = 1 << 63, (1 << 64) - 1
    edge = [0, 1, top, full]
    pairs = [(a, b) for a in edge for b in edge] + [(0x0123456789abcdef, 0x0123456789abcdef), (top | 5, 5), (5, top | 5), (6, 7), (7, 6),
                                                    (full, full - 1), (full - 1, full), (full ^ top, full)]
    for l, r in pairs:
        w = agree(circuit, model, bm.bits_of(l, 64) + ([] if one_sided else bm.bits_of(r, 64)))
        assert w[1] == int(bm.CMP_TRUTH[kind](l, r)), (kind, hex(l), hex(r))


def test_one_bit_comparators():
    for kind in bm.CMP_KINDS:
        circuit, model = bc.build_both(bc.comparator(kind, 1))
        for l in (0, 1):
            for r in ([0] if kind == "is_equal_zero" else (0, 1)):
                w = agree(circuit, model, [l] + ([] if kind == "is_equal_zero" else [r]))
                assert w[1] == int(bm.CMP_TRUTH[kind](l, r))


# ---- assertions ------------------------------------------------------------------------------------------
def test_assert_bit_gate_catches_a_flipped_input():
    def case(b):
        x, y = b.new_bits(2)
        b.assert_bit(x)
        out = b.gate("and", x, y)
        b.assert_bit(y)
        return [out]
    circuit, model = bc.build_both(case)
    bc.same_shape(circuit, model)
    assert circuit.n == 3 and circuit.m == 4
    ptr, gate, _ = bc.lib_rows(circuit, 2)
    assert gate == [1] and ptr == [0, 0, 1, 1, 1]          # W has one entry: the assertions have no output wire
    w = agree(circuit, model, [1, 1])
    assert w == [1, 1, 1, 1]
    flipped = list(w)
    flipped[2] = 2                                         # input x is no bit any more
    flipped[1] = 2                                         # ... and the AND gate is kept satisfied
    assert model.failing_gates(flipped) == [0]             # only the assertion on x objects
    with pytest.raises(ParseErr, match="bit wire 2.*not 0 or 1"):
        circuit.weights(bc.words([2, 1]))
    with pytest.raises(ParseErr, match=r"input 1 \(bit wire 3\) of instance 0 is not 0 or 1"):
        circuit.weights_tape(bc.words([1, R - 1]))
    with pytest.raises(ParseErr, match=">= r"):
        circuit.weights_tape(np.array([[1, 0, 0, 0], [0xFFFFFFFFFFFFFFFF] * 4], np.uint64))


# ---- Keccak ------------------------------------------------------------------------------------------------
def bit_witness(circuit, bits):
    """both evaluators on 0/1 inputs -> the witness as a numpy array of 0 / 1 (every element checked to be one of the two)"""
    inputs = np.zeros((len(bits), 4), np.uint64)
    inputs[:, 0] = bits
    a, b = circuit.weights(inputs), circuit.weights_tape(inputs)
    assert np.array_equal(a, b), "the two host evaluators differ"
    assert not a[:, 1:].any() and a[:, 0].max() <= 1
    return a[:, 0]


def digest_of(circuit, message, out_bytes=32):
    w = bit_witness(circuit, bm.bytes_to_bits(message))
    return bm.bits_to_bytes([int(x) for x in w[1:1 + 8 * out_bytes]])


@pytest.mark.parametrize("rounds", [1, 2])
def test_keccak_reduced_rounds_rows_and_digest(rounds):
    circuit, model = bc.build_both(bc.keccak_case(7, 136, 0x06, rounds))
    bc.same_shape(circuit, model)
    assert circuit.n == 8 * 7 + 16 + 9664 * rounds and circuit.input == 256 and circuit.n_in == 56 and circuit.boolean
    msg = b"\x00\xffkecca"
    w = agree(circuit, model, bm.bytes_to_bits(msg))
    assert bm.bits_to_bytes(w[1:257]) == bm.sponge(msg, 136, 0x06, rounds, 32)


@pytest.fixture(scope="module")
def keccak256_of_56():
    return _lib_only(bc.keccak_case(56))


def _lib_only(case):
    lib = bc.Lib()
    return lib.finish(case(lib))


def test_keccak256_doc_vector_and_gate_count(keccak256_of_56):
    circuit = keccak256_of_56
    assert circuit.n == 232400                             # 8 * 56 + 16 + 9664 * 24
    assert bm.sponge(DOC_INPUT) == DOC_DIGEST              # the model's plain Keccak reproduces the reference's doc vector
    assert digest_of(circuit, DOC_INPUT) == DOC_DIGEST
    # 448 inputs + 256 digest wires among 232400 outputs + the constant 1: nothing was folded away, the zero wire is no witness wire
    assert circuit.m == 1 + 448 + 232400 and circuit.input == 256


def test_keccak256_rows_equal_the_model(keccak256_of_56):
    model = bm.Model()
    finished = model.finish(bc.keccak_case(56)(model))
    bc.same_shape(keccak256_of_56, finished)


def test_keccak256_of_the_empty_message():
    circuit = _lib_only(bc.keccak_case(0))
    assert circuit.n_in == 0 and circuit.n == 16 + 9664 * 24
    assert digest_of(circuit, b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"


@pytest.mark.parametrize("n_bytes", [0, 1, 135, 136, 137, 272])
def test_sha3_256_against_hashlib(n_bytes):
    circuit = _lib_only(bc.keccak_case(n_bytes, 136, 0x06, 24))
    blocks = n_bytes // 136 + 1
    assert circuit.n == 8 * n_bytes + 16 + 9664 * 24 * blocks
    rng = SplitMix64(5000 + n_bytes)
    msg = bytes(rng.next() & 0xFF for _ in range(n_bytes))
    assert digest_of(circuit, msg) == hashlib.sha3_256(msg).digest()


def test_shake128_sixty_four_bytes_against_hashlib():
    circuit = _lib_only(bc.keccak_case(9, 168, 0x1F, 24, 64))
    assert digest_of(circuit, b"shake 128", 64) == hashlib.shake_128(b"shake 128").digest(64)


def test_squeeze_past_the_rate_reduced():
    """an output longer than the rate permutes between the blocks (and once more when it ends on the boundary, as the reference does)"""
    for out_bytes in (20, 41):
        circuit, model = bc.build_both(bc.keccak_case(3, 20, 0x1F, 1, out_bytes))
        bc.same_shape(circuit, model)
        assert circuit.n == 24 + 16 + 9664 * (1 + out_bytes // 20)
        assert digest_of(circuit, b"abc", out_bytes) == bm.sponge(b"abc", 20, 0x1F, 1, out_bytes)


def test_facade_names_and_validate_order():
    b = Builder()
    x, y, lo, hi, c = (b.new_word64() for _ in range(5))
    assert b.const_word8(0x4F) == [1, 1, 1, 1, 0, 0, 1, 0] and b.const_word64(1 << 63)[63] == 1
    vo = b.validate_order(x, (lo, hi), y, c)
    digest = [w for word in vo["hash_x_y"] for w in word]
    circuit = b.finish([vo["is_x_within_range"], vo["is_y_greater_than_c"]] + digest)
    assert circuit.input == 258 and circuit.n_in == 320 and circuit.boolean

    def run(xv, yv, lov, hiv, cv):
        bits = sum((bm.bits_of(v, 64) for v in (xv, yv, lov, hiv, cv)), [])
        w = [int(x) for x in bit_witness(circuit, bits)[:259]]
        return w[1], w[2], bm.bits_to_bytes(w[3:259])
    msg = (26).to_bytes(8, "little") + (9).to_bytes(8, "little")
    assert run(26, 9, 20, 30, 9) == (1, 1, bm.sponge(msg))
    assert run(26, 9, 27, 30, 10)[:2] == (0, 0)
    assert run(26, 9, 20, 26, 8)[:2] == (1, 1)
    # the reference's other spellings
    b2 = Builder()
    w8 = b2.new_word8()
    assert b2.u8_bitwise_op(w8, b2.const_word8(0xFF), b2.new_xor) == list(range(10, 18))
    assert b2.fan_in(w8, b2.new_and) == 24
    assert b2.keccak256_stream([w8])[0][0] > 24
    with pytest.raises(BuildErr):
        b2.u64_bitwise_op(w8, w8, "xor")


# ---- witness order, the zero wire, refusals ------------------------------------------------------------------
def test_witness_order_and_the_dropped_zero_wire():
    b = Builder()
    i0, i1, i2 = b.new_bits(3)
    g0 = b.new_and(i0, Builder.ZERO)                       # wire 5: its V entry sits on the zero wire and is dropped
    g1 = b.new_xor(g0, i1)                                 # wire 6
    g2 = b.new_or(i2, Builder.ONE)                         # wires 7 (the AND) and 8
    assert (g0, g1, g2) == (5, 6, 8) and b.dims() == (9, 4)
    circuit = b.finish([g2, i1])
    # [1], verify wires as given, remaining inputs in creation order, remaining wires by id
    assert [circuit.wire_index(w) for w in (1, g2, i1, i0, i2, g0, g1, 7)] == list(range(8))
    assert circuit.m == 8 and circuit.input == 2 and circuit.n_in == 3 and circuit.n == 4
    with pytest.raises(ValueError):
        circuit.wire_index(0)
    with pytest.raises(ValueError):
        circuit.wire_index(9)
    _, gate_v, _ = bc.lib_rows(circuit, 1)
    assert 0 not in gate_v                                 # gate 0's right side was the zero wire alone: V has nothing at gate 0
    w = both_evaluators(circuit, [1, 1, 0])
    assert w == [1, 1, 1, 1, 0, 0, 1, 0]


def refusal(fn, text):
    with pytest.raises(BuildErr, match=text) as e:
        fn()
    assert e.value.status == _lib.ZK_ERR_ARG


def test_refusals():
    b = Builder()
    x, y = b.new_bits(2)
    refusal(lambda: b.new_and(x, 4), "unknown wire id 4")
    refusal(lambda: b.new_not(99), "unknown wire id 99")
    refusal(lambda: b.assert_bit(4), "unknown wire id")
    refusal(lambda: b.fan_in([x, 7], "and"), "unknown wire id 7")
    refusal(lambda: b.fan_in([], "and"), "at least one")
    refusal(lambda: b.fan_in([x, y], "not"), "two-input")
    refusal(lambda: b.is_equal([x], [17]), "unknown wire id 17")
    refusal(lambda: b.is_equal([], []), "at least one")
    refusal(lambda: b.keccak([x] * 8, rate=0), "rate_bytes")
    refusal(lambda: b.keccak([x] * 8, rate=201), "rate_bytes")
    refusal(lambda: b.keccak([x] * 8, rounds=0), "rounds")
    refusal(lambda: b.keccak([x] * 8, rounds=25), "rounds")
    refusal(lambda: b.keccak([x] * 7 + [50]), "unknown wire id 50")
    refusal(lambda: b.new_sub_circuit([(1, x)], [(1, 44)]), "unknown wire id 44")
    assert b.dims() == (4, 0)                              # nothing was added by a refused call
    out = b.new_and(x, y)
    refusal(lambda: b.finish([out, out]), "named twice")
    refusal(lambda: b.finish([Builder.ONE]), "is a constant")
    refusal(lambda: b.finish([Builder.ZERO]), "is a constant")
    refusal(lambda: b.finish([9]), "unknown wire id 9")
    circuit = b.finish([out])
    assert circuit.n == 1
    for call in (lambda: b.new_bits(1), lambda: b.new_and(x, y), lambda: b.assert_bit(x), lambda: b.finish([out]), lambda: b.dims(),
                 lambda: b.keccak([x] * 8), lambda: b.is_equal([x], [y]), lambda: b.new_sub_circuit([(1, x)], [(1, y)])):
        refusal(call, "finished")
    b.close()
    assert limbs_to_ints(circuit.weights(bc.words([1, 1]))) == [1, 1, 1, 1]      # the circuit outlives its builder
    lib = _lib.load()
    assert lib.zk_builder_create(None) == _lib.ZK_ERR_ARG
    assert lib.zk_builder_gate(None, 2, 0, 0, None) == _lib.ZK_ERR_ARG
    assert lib.zk_builder_finish(None, None, 0, C.byref(C.c_void_p())) == _lib.ZK_ERR_ARG
    lib.zk_builder_free(None)


def test_weight_out_of_range_is_refused():
    lib = _lib.load()
    b = Builder()
    x = b.new_wire()
    big = np.array([0xFFFFFFFFFFFFFFFF] * 4, np.uint64)
    one = np.array([1, 0, 0, 0], np.uint64)
    wires = np.array([x], np.uint32)
    out = C.c_uint32()
    rc = lib.zk_builder_sub_circuit(b.ptr, big.ctypes.data_as(_lib.u64p), wires.ctypes.data_as(_lib.u32p), 1, one.ctypes.data_as(_lib.u64p),
                                    wires.ctypes.data_as(_lib.u32p), 1, C.byref(out))
    assert rc == _lib.ZK_ERR_RANGE and b.dims() == (3, 0)


# ---- boolean or not ----------------------------------------------------------------------------------------------
def test_general_sub_circuits_field_inputs_and_parsed_programs_are_not_boolean():
    def general(b):
        x, y = b.new_bits(2)
        t = b.sub_circuit([(3, x), (R - 2, y), (5, bm.ONE)], [(1, x), (7, bm.ZERO), (1, bm.ONE)])
        return [b.gate("and", t, y)]
    circuit, model = bc.build_both(general)
    bc.same_shape(circuit, model)
    assert not circuit.boolean
    for x in (0, 1):
        for y in (0, 1):
            w = agree(circuit, model, [x, y])
            assert w[4] == (3 * x - 2 * y + 5) * (x + 1) % R   # the entry on the zero wire contributes nothing

    def field_input(b):
        x = b.new_field()
        y = b.new_bits(1)[0]
        return [b.gate("xor", x, y)]
    circuit, model = bc.build_both(field_input)
    bc.same_shape(circuit, model)
    assert not circuit.boolean
    w = agree(circuit, model, [12345, 1])                  # a field input takes any element; (x - y)^2
    assert w[1] == 12344 ** 2
    with pytest.raises(ParseErr, match="not 0 or 1"):
        circuit.weights(bc.words([12345, 2]))

    parsed = Circuit("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n")
    assert not parsed.boolean
    with pytest.raises(ValueError):
        parsed.wire_index(2)
    assert limbs_to_ints(parsed.weights_tape(bc.words([3, 5]))) == [1, 15, 3, 5]      # parsed programs are untouched


def test_tape_dims_of_a_built_circuit():
    circuit, _ = bc.build_both(bc.not_chain(1025))
    d = circuit.tape_dims()
    assert d["depth"] == 1025 and d["width"] == 1
    circuit, _ = bc.build_both(bc.wide_level(5000))
    d = circuit.tape_dims()
    assert d["depth"] == 1 and d["width"] == 5000 and d["ops"] == 5000
