"""zk_builder_pack restated in Python integers on top of tests/builder_model.py: out = sum 2^i bits[i] as ONE sub-circuit
(sum 2^i bits[i]) * (1) = out, and the classification rule (a circuit stays bit-sliceable iff every pack operand is bit-valued and no
packed wire is read by anything).  Nothing here calls the library.

    PackModel    builder_model.Model plus pack(); `packed` lists the packed wires, boolean() is the rule
    PackLib      builder_cases.Lib plus pack()
    the cases    functions of a builder-like object returning the verify wires, as in builder_cases
"""
import builder_cases as bc
import builder_model as bm

PACK_MAX_BITS = 253
WIDTHS = (1, 2, 63, 64, 65, 128, 253)


class PackModel(bm.Model):
    def __init__(self):
        super().__init__()
        self.packed = []

    def pack(self, bits):
        assert 1 <= len(bits) <= PACK_MAX_BITS
        out = self.sub_circuit([(1 << i, w) for i, w in enumerate(bits)], [(1, bm.ONE)])
        self.kind[out] = "packed"
        self.packed.append(out)
        return out

    def boolean(self):
        """every input a bit, every sub-circuit a gate (weights +-1 by construction here) or a pack, no packed wire read"""
        if "field" in self.kind:
            return False
        return not any(self.kind[w] == "packed" for left, right, _ in self.subs for _, w in left + right)


class PackLib(bc.Lib):
    def pack(self, bits):
        return self.b.pack(bits)


def build_both(case):
    """-> (library Circuit, model Finished, the PackModel)"""
    lib, model = PackLib(), PackModel()
    v_lib, v_model = case(lib), case(model)
    assert list(v_lib) == list(v_model), "the two builders number their wires differently"
    return lib.finish(v_lib), model.finish(v_model), model


def lib_circuit(case):
    lib = PackLib()
    return lib.finish(case(lib))


def pack_value(bits):
    return sum(b << i for i, b in enumerate(bits))


# ---- the cases ---------------------------------------------------------------------------------------
def one_pack(width, verify=True):
    """a pack directly over `width` bit inputs; the packed wire is the first witness index (verify) or the last (not)"""
    def case(b):
        xs = b.new_bits(width)
        p = b.pack(xs)
        return [p] if verify else [xs[0]]
    return case


def mixed_operands(b):
    """operands that are bit inputs, gate outputs of different levels, both constants, and one wire at two positions"""
    x = b.new_bits(6)
    g1 = b.gate("xor", x[0], x[1])                          # level 1
    g2 = b.gate("and", g1, x[2])                            # level 2
    g3 = b.gate("or", g2, x[3])                             # level 4 (OR is two sub-circuits)
    chk = b.gate("bit_checker", x[4])                       # the bit checker's output: always 0 on bits
    p = b.pack([x[5], g3, bm.ONE, bm.ZERO, g1, x[5], g2, bm.ZERO, bm.ONE, chk, g3])
    q = b.pack([bm.ZERO])                                   # every operand dropped: the value is 0
    r = b.pack([bm.ONE, bm.ONE])                            # 3
    return [p, g3, q, r]


def mixed_value(x):
    g1 = x[0] ^ x[1]
    g2 = g1 & x[2]
    g3 = g2 | x[3]
    return pack_value([x[5], g3, 1, 0, g1, x[5], g2, 0, 1, 0, g3])


def all_widths(b):
    """~300 gates, then packs of every width at which a limb boundary or the cap is crossed, over gate outputs, inputs, constants and
    repeated wires; a packed wire first in the witness (verify) and one last (the final wire made)"""
    xs = b.new_bits(40)
    pool = list(xs)
    for i in range(300):
        kind = ("xor", "and", "xnor", "not", "less_than", "greater_than")[i % 6]
        pool.append(b.gate(kind, pool[(7 * i + 3) % len(pool)], pool[(11 * i + 5) % len(pool)]))
    outs = []
    for k, width in enumerate((1, 63, 64, 65, 128, 129, 192, 193, 253)):
        ops = [pool[(13 * k + 5 * i) % len(pool)] for i in range(width)]
        if width > 2:
            ops[1] = bm.ONE
            ops[width // 2] = bm.ZERO
            ops[-1] = ops[0]                                 # a wire at two positions, the top bit among them
        outs.append(b.pack(ops))
    direct = b.pack(xs)                                      # a pack directly over inputs
    b.pack([pool[-1], bm.ONE, pool[40]])                     # the last wire made and no verify wire: the last witness index
    return [outs[4], xs[3], direct, outs[0]]


def sized_with_pack(m):
    """exactly m witness wires: the constant, 5 inputs, XORs, and one 5-bit pack as the last index"""
    def case(b):
        xs = b.new_bits(5)
        w = xs[0]
        chain = []
        for i in range(m - 7):
            w = b.gate("xor", w, xs[1 + i % 4])
            chain.append(w)
        b.pack([w, xs[1], bm.ONE, xs[0], (chain or [xs[2]])[0]])
        return [w]
    return case


def many_packs(count=300):
    """more packs than one workgroup has lanes, widths 1..8, over a handful of gates"""
    def case(b):
        xs = b.new_bits(11)
        pool = list(xs) + [b.gate("xor", xs[i], xs[i + 1]) for i in range(10)] + [b.gate("and", xs[i], xs[i + 2]) for i in range(9)]
        packs = [b.pack([pool[(3 * k + 7 * i) % len(pool)] for i in range(1 + k % 8)]) for k in range(count)]
        return [packs[0], packs[-1], packs[count // 2]]
    return case


def digest_packed(n_bytes, rounds, delim=0x06, bytes_per_element=16):
    """the sponge's 32-byte digest as 32 / bytes_per_element packed verify wires, little-endian per element"""
    def case(b):
        d = b.keccak(b.new_bits(8 * n_bytes), 136, delim, rounds, 32)
        step = 8 * bytes_per_element
        return [b.pack(d[i:i + step]) for i in range(0, 256, step)]
    return case
