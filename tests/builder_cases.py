"""Circuits built twice from one description -- once through the library's Builder, once through tests/builder_model.py -- for
tests/test_builder.py and tests/test_gpu_boolgen.py.  A case is a function of a builder-like object `b` (new_bits, gate, compare,
keccak, fan_in, bitwise, assert_bit) returning the verify wires; Lib adapts circuit.Builder to that interface."""
import numpy as np

import builder_model as bm
from zksnark_rs_amd import ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuit import Builder


class Lib:
    """circuit.Builder behind the model's method names"""

    def __init__(self):
        self.b = Builder()

    def new_bits(self, n):
        return self.b.new_bits(n)

    def new_field(self):
        return self.b.new_wire()

    def sub_circuit(self, left, right):
        return self.b.new_sub_circuit(left, right)

    def gate(self, kind, x, y=None):
        return getattr(self.b, "new_" + kind)(*([x] if kind in bm.UNARY else [x, y]))

    def assert_bit(self, w):
        self.b.assert_bit(w)

    def fan_in(self, kind, wires):
        return self.b.fan_in(wires, kind)

    def bitwise(self, kind, xs, ys=None):
        return self.b.bitwise_op(xs, ys, kind)

    def compare(self, kind, l, r=None):
        return getattr(self.b, kind)(*([l] if r is None else [l, r]))

    def keccak(self, in_wires, rate=136, delim=0x01, rounds=24, out_bytes=32):
        return [w for word in self.b.keccak(in_wires, rate, delim, rounds, out_bytes) for w in word]

    def finish(self, verify=()):
        return self.b.finish(verify)


def build_both(case):
    """-> (library Circuit, model Finished)"""
    lib, model = Lib(), bm.Model()
    v_lib, v_model = case(lib), case(model)
    assert list(v_lib) == list(v_model), "the two builders number their wires differently"
    return lib.finish(v_lib), model.finish(v_model)


# ---- the cases ---------------------------------------------------------------------------------------
def one_gate(kind):
    def case(b):
        x, y = b.new_bits(2)
        return [b.gate(kind, x, y)]
    return case


def all_gates(b):
    """every gate kind on inputs, on both constants and on other gates' outputs; every vector form; assertions on the inputs"""
    a, c, d, e = b.new_bits(4)
    outs = []
    for kind in bm.GATE_KINDS:
        outs.append(b.gate(kind, a, c))
        outs.append(b.gate(kind, d, bm.ZERO))
        outs.append(b.gate(kind, bm.ONE, e))
    for i, kind in enumerate(bm.GATE_KINDS):
        outs.append(b.gate(kind, outs[3 * i], outs[(3 * i + 7) % len(outs)]))
    outs.append(b.fan_in("xor", [a, c, d, e, outs[5]]))
    outs.append(b.fan_in("nor", [a]))                       # a single element: no gate
    outs += b.bitwise("nand", [a, c, d], [e, outs[2], bm.ONE])
    outs += b.bitwise("not", [a, outs[9]])
    for w in (a, c, d, e):
        b.assert_bit(w)
    b.assert_bit(bm.ZERO)
    b.assert_bit(bm.ONE)
    return [outs[-1], outs[4], e]


def comparator(kind, bits):
    def case(b):
        l = b.new_bits(bits)
        r = None if kind == "is_equal_zero" else b.new_bits(bits)
        return [b.compare(kind, l, r)]
    return case


def keccak_case(n_bytes, rate=136, delim=0x01, rounds=24, out_bytes=32):
    def case(b):
        return b.keccak(b.new_bits(8 * n_bytes), rate, delim, rounds, out_bytes)
    return case


def not_chain(length):
    def case(b):
        w = b.new_bits(1)[0]
        for _ in range(length):
            w = b.gate("not", w)
        return [w]
    return case


def wide_level(width):
    def case(b):
        xs = b.new_bits(2 * width)
        outs = b.bitwise("and", xs[:width], xs[width:])
        return [outs[0], outs[-1]]
    return case


def sized(m):
    """a circuit of exactly m witness wires: n_in = 5 bit inputs, then XORs"""
    def case(b):
        xs = b.new_bits(5)
        w = xs[0]
        for i in range(m - 6):
            w = b.gate("xor", w, xs[1 + i % 4])
        return [w]
    return case


def odd_inputs(b):
    """13 inputs: the last byte of a packed row has three unused bits"""
    xs = b.new_bits(13)
    return [b.fan_in("xor", xs), b.fan_in("and", xs[8:]), b.fan_in("or", xs[:3])]


# ---- comparing -----------------------------------------------------------------------------------------
def lib_rows(circuit, which):
    ptr, gate, val = circuit.rows(which)
    return [int(x) for x in ptr], [int(x) for x in gate], limbs_to_ints(val) if len(gate) else []


def same_shape(circuit, model):
    assert (circuit.m, circuit.n, circuit.input, circuit.n_in) == (model.m, model.n, model.input, model.n_in)
    for which in range(3):
        ptr, gate, val = circuit.rows(which)
        want_ptr, want_gate, want_val = model.csr(which)
        assert np.array_equal(ptr, np.array(want_ptr, np.uint64)) and np.array_equal(gate, np.array(want_gate, np.uint32)), "rows %d" % which
        distinct = sorted(set(want_val))                    # few distinct weights: convert each once
        table, at = words(distinct), {v: i for i, v in enumerate(distinct)}
        assert np.array_equal(val, table[[at[v] for v in want_val]].reshape(-1, 4)), "row values %d" % which


def words(values):
    """integers -> (len, 4) uint64, empty-safe"""
    return ints_to_limbs(list(values)) if len(values) else np.zeros((0, 4), np.uint64)


def pack_rows(bit_rows, stride=None, fill=0):
    """list of per-instance bit lists -> (count, stride) uint8 packed the way zk_boolgen_run reads; unused bits = `fill`'s bits"""
    n = len(bit_rows[0])
    nb = (n + 7) // 8
    out = np.full((len(bit_rows), stride or max(nb, 1)), fill, np.uint8)
    for j, bits in enumerate(bit_rows):
        for k in range(nb):
            v = fill
            for i in range(8):
                if 8 * k + i < n:
                    v = (v & ~(1 << i)) | (bits[8 * k + i] << i)
            out[j, k] = v
    return out
