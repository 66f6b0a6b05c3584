"""The gate-level circuit builder restated in Python integers: the model tests/test_builder.py and tests/test_gpu_boolgen.py hold the
library against.  Nothing here calls the library.

    GATES        weights of every gate kind's sub-circuits, (sum left) * (sum right) = out, as circuit/builder/mod.rs:723-798, 939-950
                 writes them ('1' the unity wire, 't' the output of the sub-circuit before)
    Model        wires, sub-circuits, the comparators' composition (mod.rs:995-1241), the sponge (mod.rs:1247-1398)
    Finished     witness order, rows, evaluation in creation order, the check U_j V_j = W_j per gate
    keccak_f, sponge   a plain integer Keccak for digests (state of 25 64-bit lanes)
"""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ZERO, ONE = 0, 1

GATES = {
    "bit_checker": [([(1, "x")], [(1, "x"), (-1, "1")])],
    "not": [([(1, "1")], [(1, "1"), (-1, "x")])],
    "and": [([(1, "x")], [(1, "y")])],
    "or": [([(1, "x")], [(1, "y")]), ([(-1, "t"), (1, "x"), (1, "y")], [(1, "1")])],
    "xor": [([(1, "x"), (-1, "y")], [(1, "x"), (-1, "y")])],
    "nand": [([(1, "x")], [(1, "y")]), ([(1, "1")], [(1, "1"), (-1, "t")])],
    "nor": [([(1, "x")], [(1, "y")]), ([(1, "1"), (1, "t"), (-1, "x"), (-1, "y")], [(1, "1")])],
    "xnor": [([(1, "1"), (-1, "x"), (1, "y")], [(1, "1"), (1, "x"), (-1, "y")])],
    "less_than": [([(1, "1"), (-1, "x")], [(1, "y")])],
    "greater_than": [([(1, "1"), (-1, "y")], [(1, "x")])],
}
GATE_KINDS = list(GATES)          # in the order of ZK_GATE_*
UNARY = ("bit_checker", "not")
TRUTH = {"bit_checker": lambda x, y: 0, "not": lambda x, y: 1 - x, "and": lambda x, y: x & y, "or": lambda x, y: x | y, "xor": lambda x, y: x ^ y,
         "nand": lambda x, y: 1 - (x & y), "nor": lambda x, y: 1 - (x | y), "xnor": lambda x, y: 1 - (x ^ y),
         "less_than": lambda x, y: int(x < y), "greater_than": lambda x, y: int(x > y)}
CMP_KINDS = ["is_equal", "is_equal_zero", "less_than", "less_than_eq", "greater_than", "greater_than_eq"]   # in the order of ZK_CMP_*
CMP_TRUTH = {"is_equal": lambda a, b: a == b, "is_equal_zero": lambda a, b: a == 0, "less_than": lambda a, b: a < b,
             "less_than_eq": lambda a, b: a <= b, "greater_than": lambda a, b: a > b, "greater_than_eq": lambda a, b: a >= b}

RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808a, 0x8000000080008000, 0x000000000000808b, 0x0000000080000001,
      0x8000000080008081, 0x8000000000008009, 0x000000000000008a, 0x0000000000000088, 0x0000000080008009, 0x000000008000000a,
      0x000000008000808b, 0x800000000000008b, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
      0x000000000000800a, 0x800000008000000a, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
RHO = [1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44]
PI = [10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1]
M64 = (1 << 64) - 1


# ---- a plain integer Keccak ------------------------------------------------------------------------
def _rotl(x, r):
    r %= 64
    return ((x << r) | (x >> (64 - r))) & M64 if r else x


def keccak_f(a, rounds=24):
    """the first `rounds` rounds of Keccak-f[1600] on 25 lanes, lane x + 5 y"""
    a = list(a)
    for rnd in range(rounds):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1)
            for y in range(0, 25, 5):
                a[y + x] ^= d
        last = a[1]
        for x in range(24):
            a[PI[x]], last = _rotl(last, RHO[x]), a[PI[x]]
        for y in range(0, 25, 5):
            row = a[y:y + 5]
            for x in range(5):
                a[y + x] = row[x] ^ (~row[(x + 1) % 5] & M64 & row[(x + 2) % 5])
        a[0] ^= RC[rnd]
    return a


def sponge(message, rate=136, delim=0x01, rounds=24, out_bytes=32):
    st = bytearray(200)

    def permute():
        lanes = keccak_f([int.from_bytes(st[8 * i:8 * i + 8], "little") for i in range(25)], rounds)
        st[:] = b"".join(x.to_bytes(8, "little") for x in lanes)

    off = 0
    for byte in message:
        st[off] ^= byte
        off += 1
        if off == rate:
            permute()
            off = 0
    st[off] ^= delim
    st[rate - 1] ^= 0x80
    permute()
    out = b""
    while out_bytes - len(out) >= rate:
        out += bytes(st[:rate])
        permute()
    return out + bytes(st[:out_bytes - len(out)])


# ---- the builder ------------------------------------------------------------------------------------
class Finished:
    def __init__(self, model, verify):
        wires = len(model.kind)
        wit = {ONE: 0}
        for v in verify:
            assert v >= 2 and v not in wit
            wit[v] = len(wit)
        for w in range(2, wires):
            if model.kind[w] in ("bit", "field") and w not in wit:
                wit[w] = len(wit)
        for w in range(2, wires):
            if w not in wit:
                wit[w] = len(wit)
        self.wit, self.m, self.n, self.input = wit, len(wit), len(model.subs), len(verify)
        self.inputs = [w for w in range(2, wires) if model.kind[w] in ("bit", "field")]
        self.n_in = len(self.inputs)
        self.subs = []                                     # over witness indices, zero-wire entries dropped
        self.rows = [[[] for _ in range(self.m)] for _ in range(3)]
        for k, (left, right, out) in enumerate(model.subs):
            l = [(c % R, wit[w]) for c, w in left if w != ZERO]
            r = [(c % R, wit[w]) for c, w in right if w != ZERO]
            o = None if out is None else wit[out]
            self.subs.append((l, r, o))
            for c, i in l:
                self.rows[0][i].append((k, c))
            for c, i in r:
                self.rows[1][i].append((k, c))
            if o is not None:
                self.rows[2][o].append((k, 1))

    def csr(self, which):
        """(ptr, gate, val) of u (0), v (1) or w (2): what zk_circuit_rows returns, values as integers"""
        ptr, gate, val = [0], [], []
        for row in self.rows[which]:
            gate += [g for g, _ in row]
            val += [c for _, c in row]
            ptr.append(len(gate))
        return ptr, gate, val

    def evaluate(self, inputs):
        """inputs in creation order -> the witness as integers"""
        assert len(inputs) == self.n_in
        a = [0] * self.m
        a[0] = 1
        for w, x in zip(self.inputs, inputs):
            a[self.wit[w]] = x % R
        for l, r, o in self.subs:
            if o is not None:
                a[o] = sum(c * a[i] for c, i in l) * sum(c * a[i] for c, i in r) % R
        return a

    def failing_gates(self, a):
        bad = []
        for k, (l, r, o) in enumerate(self.subs):
            if (sum(c * a[i] for c, i in l) * sum(c * a[i] for c, i in r) - (0 if o is None else a[o])) % R:
                bad.append(k)
        return bad


class Model:
    def __init__(self):
        self.kind = ["const", "const"]
        self.subs = []                                     # (left [(weight, wire)], right, out wire or None)

    def _wire(self, kind):
        self.kind.append(kind)
        return len(self.kind) - 1

    def new_bits(self, n):
        return [self._wire("bit") for _ in range(n)]

    def new_field(self):
        return self._wire("field")

    def sub_circuit(self, left, right, with_out=True):
        out = self._wire("out") if with_out else None
        self.subs.append((list(left), list(right), out))
        return out

    def gate(self, kind, x, y=None):
        t = None
        for left, right in GATES[kind]:
            name = {"x": x, "y": y, "1": ONE, "t": t}
            t = self.sub_circuit([(c, name[s]) for c, s in left], [(c, name[s]) for c, s in right])
        return t

    def assert_bit(self, w):
        self.sub_circuit([(1, w)], [(1, w), (-1, ONE)], with_out=False)

    def fan_in(self, kind, wires):
        acc = wires[0]
        for w in wires[1:]:
            acc = self.gate(kind, acc, w)
        return acc

    def bitwise(self, kind, xs, ys=None):
        return [self.gate(kind, x, None if ys is None else ys[i]) for i, x in enumerate(xs)]

    # comparators
    def is_equal(self, l, r):
        acc = self.gate("xnor", l[0], r[0])
        for a, b in zip(l[1:], r[1:]):
            eq = self.gate("xnor", a, b)
            acc = self.gate("and", eq, acc)
        return acc

    def is_equal_zero(self, x):
        return self.is_equal(x, [ZERO] * len(x))

    def greater_than(self, l, r):
        cmp0 = self.gate("greater_than", l[0], r[0])
        if len(l) == 1:
            return cmp0
        cmp, eq = [], []
        for a, b in zip(l[1:], r[1:]):
            cmp.append(self.gate("greater_than", a, b))
            eq.append(self.gate("xnor", a, b))
        acc = cmp.pop()
        cmp.insert(0, cmp0)
        for c in cmp:
            both = self.gate("and", c, self.fan_in("and", eq))
            eq.pop(0)
            acc = self.gate("or", acc, both)
        return acc

    def compare(self, kind, l, r=None):
        if kind == "is_equal":
            return self.is_equal(l, r)
        if kind == "is_equal_zero":
            return self.is_equal_zero(l)
        if kind == "greater_than":
            return self.greater_than(l, r)
        if kind == "less_than":
            neg = self.gate("not", self.greater_than(l, r))
            neg_eq = self.gate("not", self.is_equal(l, r))
            return self.gate("and", neg, neg_eq)
        if kind == "less_than_eq":
            neg = self.gate("not", self.greater_than(l, r))
            return self.gate("or", neg, self.is_equal(l, r))
        if kind == "greater_than_eq":
            gt = self.greater_than(l, r)
            return self.gate("or", gt, self.is_equal(l, r))
        raise KeyError(kind)

    # the sponge over wires: a lane is a list of 64 wires, least significant first
    def _keccak_f(self, a, rounds):
        rot = lambda lane, by: [lane[(i - by) % 64] for i in range(64)]   # noqa: E731
        for rnd in range(rounds):
            col = [[ZERO] * 64 for _ in range(5)]
            for x in range(5):
                for y in range(0, 25, 5):
                    col[x] = self.bitwise("xor", col[x], a[x + y])
            for x in range(5):
                for y in range(0, 25, 5):
                    t = self.bitwise("xor", a[y + x], col[(x + 4) % 5])
                    a[y + x] = self.bitwise("xor", t, rot(col[(x + 1) % 5], 1))
            last = a[1]
            for x in range(24):
                a[PI[x]], last = rot(last, RHO[x]), a[PI[x]]
            for y in range(0, 25, 5):
                row = a[y:y + 5]
                for x in range(5):
                    n = self.bitwise("not", row[(x + 1) % 5])
                    c = self.bitwise("and", n, row[(x + 2) % 5])
                    a[y + x] = self.bitwise("xor", row[x], c)
            a[0] = self.bitwise("xor", a[0], [(RC[rnd] >> i) & 1 for i in range(64)])

    def keccak(self, in_wires, rate=136, delim=0x01, rounds=24, out_bytes=32):
        """in_wires: 8 per byte, flat -> 8 * out_bytes wires"""
        a = [[ZERO] * 64 for _ in range(25)]

        def xor_byte(at, src):
            lane, lo = a[at // 8], 8 * (at % 8)
            lane[lo:lo + 8] = self.bitwise("xor", lane[lo:lo + 8], src)

        off = 0
        for k in range(len(in_wires) // 8):
            xor_byte(off, in_wires[8 * k:8 * k + 8])
            off += 1
            if off == rate:
                self._keccak_f(a, rounds)
                off = 0
        xor_byte(off, [(delim >> i) & 1 for i in range(8)])
        xor_byte(rate - 1, [(0x80 >> i) & 1 for i in range(8)])
        self._keccak_f(a, rounds)
        out, left = [], out_bytes
        flat = lambda: [w for lane in a for w in lane]   # noqa: E731
        while left >= rate:
            out += flat()[:8 * rate]
            self._keccak_f(a, rounds)
            left -= rate
        return out + flat()[:8 * left]

    def finish(self, verify=()):
        return Finished(self, list(verify))


def bits_of(value, n):
    return [(value >> i) & 1 for i in range(n)]


def bytes_to_bits(data):
    return [(b >> i) & 1 for b in data for i in range(8)]


def bits_to_bytes(bits):
    return bytes(sum(bits[8 * k + i] << i for i in range(8)) for k in range(len(bits) // 8))
