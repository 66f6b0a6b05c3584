"""The curve and hash gadgets as shared test cases: tests/test_gadget_cases.py holds them against the three host evaluators and
tests/test_gpu_gadgets.py against the device witness paths, the device QAP check, the scalar-multiplication and hash kernels and the
prover.  Every case is one circuit built twice, through the library's Builder and through tests/babyjub_model.py's Gadget (Pair),
with its instances as rows of Python integers in creation order; the model's witnesses are computed once per case and shared.
Nothing here needs a device or torch.

    Pair, split_inputs, check_rows, check_witness, value, outputs     what test_babyjub.py and test_poseidon.py build and check with
    add_case(q_affine)            babyjub_add + babyjub_affine over all ordered pairs of the edge points, operands scaled by drawn Z
    on_curve_case()               babyjub_assert_on_curve alone, points on and off the curve alternating lane by lane
    mul_var_case(n_bits)          babyjub_mul + babyjub_affine, every scalar against seven points of every order
    mul_fixed_case(n_bits)        babyjub_mul_fixed + babyjub_affine, every scalar
    poseidon_case(arity)          one hash with a public digest
    statement_case(n_s, n_h)      [S] Base8 = R + [h] A with every gadget in it, the shape of a signature check
    chain_case()                  the gadgets' kinds of gate side one behind the other: the only tape here the witness kernels run with one wave
"""
import functools
import itertools

import numpy as np

from zksnark_rs_amd import SplitMix64, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuit import Builder

import babyjub_model as bm

R = bm.R
EDGE = bm.edge_points()
SPREAD = 40                                                 # instances of a case the host tests evaluate


# ---- one circuit, built twice --------------------------------------------------------------------------
class Pair:
    """one circuit built twice: through the library and through the model"""

    def __init__(self):
        self.lib, self.model = Builder(), bm.Gadget()

    def field(self):
        a, b = self.lib.new_wire(), self.model.new_field()
        assert a == b
        return a

    def bits(self, n):
        a, b = self.lib.new_bits(n), self.model.new_bits(n)
        assert a == b
        return a

    def both(self, name, *args):
        a, b = getattr(self.lib, name)(*args), getattr(self.model, name)(*args)
        assert a == b, name
        return a

    def sub(self, left, right):
        """one general gate (sum left) * (sum right) over (weight, wire) pairs"""
        a, b = self.lib.new_sub_circuit(left, right), self.model.sub_circuit([(c % R, w) for c, w in left], [(c % R, w) for c, w in right])
        assert a == b
        return a

    def finish(self, verify):
        assert self.lib.dims() == (len(self.model.kind), len(self.model.subs))
        c, f = self.lib.finish(verify), self.model.finish(verify)
        f.kinds = list(self.model.kind)
        return c, f


def split_inputs(f, row):
    kinds = [k for k in f.kinds if k in ("bit", "field")]
    bits = [x for x, k in zip(row, kinds) if k == "bit"]
    packed = bytes(sum(b << i for i, b in enumerate(bits[8 * k:8 * k + 8])) for k in range((len(bits) + 7) // 8))
    return packed, [x for x, k in zip(row, kinds) if k == "field"]


def check_rows(c, f):
    assert (c.m, c.n, c.input, c.n_in) == (f.m, f.n, f.input, f.n_in)
    for which in range(3):
        ptr, gate, val = c.rows(which)
        mptr, mgate, mval = f.csr(which)
        assert [int(x) for x in ptr] == mptr and [int(x) for x in gate] == mgate and limbs_to_ints(val) == mval, which
    assert not c.boolean


def check_witness(c, f, row, want=None, failing=()):
    """the three host evaluators agree with the model's witness, and exactly the gates `failing` do not hold (none by default)"""
    want = f.evaluate(row) if want is None else want
    assert f.failing_gates(want) == list(failing)
    w = c.weights(row)
    assert limbs_to_ints(w) == want
    assert np.array_equal(c.weights_tape(row), w)
    packed, fields = split_inputs(f, row)
    assert np.array_equal(c.weights_mixed(packed, fields), w)
    return want


def value(f, w, point):
    """the affine point behind three wires of a witness"""
    v = [1 if x == 1 else w[f.wit[x]] for x in point]
    assert v[2] != 0
    return bm.to_affine(tuple(v))


def outputs(point):
    return [x for x in point if x > 1]


# ---- a case ------------------------------------------------------------------------------------------------
class Case:
    """c, f: the circuit from the library and from the model; rows: the instances, integers in creation order; edge: the instances a
    spread always holds; failing[j]: the gates instance j leaves unsatisfied ([] for all where None); info: wires and gate indices"""

    def __init__(self, name, c, f, rows, edge, failing=None, **info):
        self.name, self.c, self.f, self.rows, self.edge, self.info = name, c, f, rows, sorted(set(edge)), info
        self.failing = failing or [[] for _ in rows]
        assert len(self.failing) == len(rows) and all(len(r) == f.n_in for r in rows) and len(self.edge) <= SPREAD
        self.kinds = [k for k in f.kinds if k in ("bit", "field")]
        self._want = {}

    def want(self, j):
        """the model's witness of instance j as integers, computed once"""
        if j not in self._want:
            self._want[j] = self.f.evaluate(self.rows[j])
        return self._want[j]

    @functools.lru_cache(maxsize=None)
    def want_words(self):
        """(count, m, 4) uint64: the model's witnesses of all instances.  Read only."""
        out = np.stack([ints_to_limbs(self.want(j)) for j in range(len(self.rows))])
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def tape_inputs(self):
        """(count, n_in, 4) uint64: every input as a field element in creation order, what Witgen.run reads"""
        out = np.stack([ints_to_limbs(row) for row in self.rows])
        out.setflags(write=False)
        return out

    @functools.lru_cache(maxsize=None)
    def mixed_inputs(self):
        """((count, max(ceil(n_bit / 8), 1)) uint8, (count, n_field, 4) uint64): what Mixgen.run reads"""
        split = [split_inputs(self.f, row) for row in self.rows]
        n_bytes, n_field = len(split[0][0]), len(split[0][1])
        bits = np.frombuffer(b"".join(p or b"\0" for p, _ in split), np.uint8).reshape(len(split), max(n_bytes, 1))   # never an empty row
        fields = np.stack([ints_to_limbs(fs) for _, fs in split]) if n_field else np.zeros((len(split), 0, 4), np.uint64)
        fields.setflags(write=False)
        return bits, fields

    def spread(self):
        """at most SPREAD instances: the edge ones and an even draw from the rest, of either parity"""
        count, room = len(self.rows), SPREAD - len(self.edge)
        step = -(-count // max(room, 1)) | 1                # odd: where two kinds of instance alternate, the draw holds both
        rest = [j for j in range(0, count, step) if j not in self.edge]
        return sorted(self.edge + rest[:room])


def bits_of(k, n):
    return [(k >> i) & 1 for i in range(n)]


def scaled(p, z):
    return [p[0] * z % R, p[1] * z % R, z]


# ---- a. babyjub_add ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def add_case(q_affine):
    p = Pair()
    pw = [p.field() for _ in range(3)]
    qw = [p.field(), p.field()] + ([p.lib.ONE] if q_affine else [p.field()])
    x, y = p.field(), p.field()
    sw = p.both("babyjub_add", pw, qw)
    p.both("babyjub_affine", sw, [x, y])
    assert p.lib.dims()[1] == (10 if q_affine else 11) + 4
    c, f = p.finish(sw)
    rng = SplitMix64(2100 + q_affine)
    rows, edge = [], []
    for (i, a), (k, b) in itertools.product(enumerate(EDGE), repeat=2):
        z1, z2 = rng.fr() or 1, 1 if q_affine else rng.fr() or 1
        if i == k or (b == bm.neg(a) and i < k):            # the doublings, and a point against its negative
            edge.append(len(rows))
        rows.append(scaled(a, z1) + scaled(b, z2)[:2 if q_affine else 3] + list(bm.add(a, b)))
    assert len(rows) == len(EDGE) ** 2 == 256               # 20 points and negatives, 16 of them distinct
    return Case("add_%s" % ("affine" if q_affine else "projective"), c, f, rows, edge, sum=sw, x_input=5 if q_affine else 6)


# ---- b. babyjub_assert_on_curve -----------------------------------------------------------------------------
OFF_CURVE = [(1, 1), (bm.BASE8[0] + 1, bm.BASE8[1]), (bm.BASE8[0], bm.BASE8[1] + 1), (0, 0)]


@functools.lru_cache(maxsize=None)
def on_curve_case():
    """even lanes on the curve, odd lanes off it: every wave holds both kinds"""
    p = Pair()
    x, y = p.field(), p.field()
    p.both("babyjub_assert_on_curve", [x, y])
    assert p.lib.dims()[1] == 4
    c, f = p.finish([])
    assert not any(bm.on_curve(q) for q in OFF_CURVE)
    rows, failing = [], []
    for j in range(130):
        on = j % 2 == 0
        rows.append(list(EDGE[(j // 2) % len(EDGE)] if on else OFF_CURVE[(j // 2) % len(OFF_CURVE)]))
        failing.append([] if on else [3])
    return Case("on_curve", c, f, rows, range(8), failing)


# ---- c. babyjub_mul -----------------------------------------------------------------------------------------
VAR_POINTS = [bm.GENERATOR, bm.IDENTITY, (0, R - 1), (bm.X4, 0), (R - bm.X4, 0), bm.mul(bm.L, bm.GENERATOR), bm.neg(bm.BASE8)]


@functools.lru_cache(maxsize=None)
def mul_var_case(n_bits):
    p = Pair()
    px, py = p.field(), p.field()
    bits = p.bits(n_bits)
    x, y = p.field(), p.field()
    out = p.both("babyjub_mul", [px, py], bits)
    p.both("babyjub_affine", out, [x, y])
    assert p.lib.dims()[1] == bm.var_gates(n_bits) + 4
    c, f = p.finish([x, y])
    rows, edge = [], []
    top = (1 << n_bits) - 1
    for pt in VAR_POINTS:
        for k in range(1 << n_bits):
            if k in (0, 1, top, 1 << (n_bits - 1)):
                edge.append(len(rows))
            rows.append(list(pt) + bits_of(k, n_bits) + list(bm.mul(k, pt)))
    assert len(rows) == 7 << n_bits
    return Case("mul_var_%d" % n_bits, c, f, rows, edge, out=out)


# ---- d. babyjub_mul_fixed -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mul_fixed_case(n_bits):
    p = Pair()
    bits = p.bits(n_bits)
    x, y = p.field(), p.field()
    out = p.both("babyjub_mul_fixed", bits)
    p.both("babyjub_affine", out, [x, y])
    assert p.lib.dims()[1] == bm.fixed_gates(n_bits) + 4
    c, f = p.finish([x, y])
    rows = [bits_of(k, n_bits) + list(bm.mul(k)) for k in range(1 << n_bits)]
    top = (1 << n_bits) - 1
    return Case("mul_fixed_%d" % n_bits, c, f, rows, [0, 1, top, 1 << (n_bits - 1), 7 & top, 8 & top], out=out)


# ---- e. poseidon ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poseidon_case(arity):
    p = Pair()
    ins = [p.field() for _ in range(arity)]
    out = p.both("poseidon", ins)
    c, f = p.finish([out])
    rng = SplitMix64(2200 + arity)
    rows = [[0] * arity, [R - 1] * arity, [(R - 1) * (1 - i % 2) for i in range(arity)]]
    rows += [[rng.fr() for _ in range(arity)] for _ in range(130 - len(rows))]
    return Case("poseidon_%d" % arity, c, f, rows, [0, 1, 2], digest=out)


# ---- f. the statement [S] Base8 = R + [h] A ----------------------------------------------------------------------
STATEMENT_SIZES = {(7, 7): (702, 21), (251, 251): (6961, 509)}
ORDER_2, ORDER_4, ORDER_8 = (0, R - 1), (bm.X4, 0), bm.mul(bm.L, bm.GENERATOR)
STATEMENT_FIELDS = 7                                        # Ax, Ay, Rx, Ry, M, Ox, Oy
STATEMENT_COUNT = 65
STATEMENT_EDGE_LANES = (0, 63, 64, 1, 31, 62)               # the first and last lane of a wave, the first of the next; then the rest


def statement_row(n_s, n_h, s, h, a, m):
    """the satisfying row of scalars s, h, key a and message m: R = [s] Base8 - [h] a, O = [s] Base8"""
    o = bm.pmul(s)
    r = bm.add(o, bm.neg(bm.pmul(h, a)))
    return list(a) + list(r) + [m] + list(o) + bits_of(s, n_s) + bits_of(h, n_h)


@functools.lru_cache(maxsize=None)
def statement_case(n_s, n_h):
    p = Pair()
    ax, ay, rx, ry, m, ox, oy = [p.field() for _ in range(STATEMENT_FIELDS)]
    s_bits = p.bits(n_s)
    h_bits = p.bits(n_h)
    sb = p.both("babyjub_mul_fixed", s_bits)
    ha = p.both("babyjub_mul", [ax, ay], h_bits)
    p.both("babyjub_assert_on_curve", [rx, ry])
    t = p.both("babyjub_add", ha, [rx, ry, p.lib.ONE])
    first_affine = p.lib.dims()[1]
    p.both("babyjub_affine", sb, [ox, oy])
    p.both("babyjub_affine", t, [ox, oy])
    digests = [p.both("poseidon", [rx, ry, ax, ay]), p.both("poseidon", [m])]
    gates, n_in = p.lib.dims()[1], STATEMENT_FIELDS + n_s + n_h
    assert first_affine == bm.fixed_gates(n_s) + bm.var_gates(n_h) + 4 + 10 and gates == first_affine + 8 + 301 + 217
    if (n_s, n_h) in STATEMENT_SIZES:
        assert (gates, n_in) == STATEMENT_SIZES[(n_s, n_h)]
    c, f = p.finish(digests)
    assert c.n_in == n_in
    top_s, top_h = (1 << n_s) - 1, (1 << n_h) - 1
    # A of order 2 under h = 2^n_h - 1 and S = 0; A of order 4 under h = 0; A of order 8; then what is left of the edge scalars and keys
    edges = [(0, top_h, ORDER_2), (top_s, 0, ORDER_4), ((bm.L - 1) & top_s, (bm.L - 1) & top_h, ORDER_8),
             (1, 1, bm.IDENTITY), (bm.L & top_s, top_h, bm.BASE8), (0, (bm.L - 1) & top_h, bm.neg(bm.BASE8))]
    rng = SplitMix64(2300 + n_s)
    draws = []
    for _ in range(STATEMENT_COUNT):
        k = rng.next() % (1 << 20)
        draws.append((((rng.fr() << 128) ^ rng.fr()) & top_s, ((rng.fr() << 128) ^ rng.fr()) & top_h, bm.pmul(k + 2, bm.GENERATOR)))
    for lane, e in zip(STATEMENT_EDGE_LANES, edges):
        draws[lane] = e
    rows = [statement_row(n_s, n_h, s, h, a, rng.fr()) for s, h, a in draws]
    return Case("statement_%d_%d" % (n_s, n_h), c, f, rows, STATEMENT_EDGE_LANES, scalars=draws, n_s=n_s, n_h=n_h,
                affine_x=first_affine + 1)                  # the assertion (Ox Z - X) * 1 = 0 of the first babyjub_affine


# ---- g. a chain ---------------------------------------------------------------------------------------------------------
CHAIN_LINKS = 12


@functools.lru_cache(maxsize=None)
def chain_case():
    """No gadget circuit is a chain: the widest has four or more operations a level, so the witness kernels give each group four
    waves and every level starts from memory.  With one operation a level they run one wave in program order and hand each result
    to the next operation in registers, as either operand.  This chain is made of the gate sides the curve gadgets emit, each link
    reading the one before: a square (both operands), a large constant times the wire against the constant wire alone (the second
    operand, then the first), the constant wire alone against the wire (the second operand)."""
    p = Pair()
    x = p.field()
    one = p.lib.ONE
    t = x
    for k in range(CHAIN_LINKS):
        t = p.sub([(1, t)], [(1, t)])
        t = p.sub([((bm.A, -bm.D, -2)[k % 3], t)], [(1, one)])
        t = p.sub([((-bm.A, bm.D, 2)[k % 3], one)], [(1, t)])
    c, f = p.finish([t])
    rng = SplitMix64(2500)
    rows = [[0], [1], [R - 1], [2]] + [[rng.fr()] for _ in range(126)]
    return Case("chain", c, f, rows, [0, 1, 2, 3, 63, 64])


def all_cases():
    """name -> a function that builds the case; nothing is built before it is asked for"""
    out = {"add_affine": lambda: add_case(True), "add_projective": lambda: add_case(False), "on_curve": on_curve_case}
    for n in (1, 2, 3, 7):
        out["mul_var_%d" % n] = functools.partial(mul_var_case, n)
    for n in (1, 2, 3, 4, 7):
        out["mul_fixed_%d" % n] = functools.partial(mul_fixed_case, n)
    for arity in (1, 2, 4):
        out["poseidon_%d" % arity] = functools.partial(poseidon_case, arity)
    out["statement_7_7"] = lambda: statement_case(7, 7)
    out["statement_251_251"] = lambda: statement_case(251, 251)
    out["chain"] = chain_case
    return out
