"""Circuits and .zk programs DRAWN from a seed, for tests/test_generated_circuits.py (host) and tests/test_gpu_generated_circuits.py
(device).  The fixed cases of builder_cases.py, builder_pack_model.py and witgen_cases.py vary the inputs; here the structure varies:
which operation reads which wire, how far back, through which constant, on which side.  No GPU, nothing but SplitMix64.

    built_case(shape, seed)   -> case(b), a function of a builder-like object as builder_pack_model.build_both takes; case.plan is
                                 the drawn description, case.census what the description reaches (filled while it is drawn, on a
                                 model of this module's own: nothing the caller's `b` returns is ever looked at)
    program(shape, seed)      -> (source text, ast) of a valid .zk program
    eval_ast(ast, inputs)     -> its witness as Python integers
    built_tape_shape, program_tape_shape   the two tape compilers' counting restated: (ops, slots, consts, levels, widest level)
"""
import builder_model as bm
import builder_pack_model as pm
from zksnark_rs_amd import SplitMix64

R = bm.R
BUILT_SHAPES = ("chain", "wide", "mixed", "packs", "field")
SIZED = (127, 128, 129, 255, 256, 257, 513)
PROGRAM_SHAPES = ("chain", "wide", "mixed")
PACK_WIDTHS = (1, 63, 64, 65, 128, 253)
WEIGHTS = (0, 1, R - 1, (R - 1) // 2)
BINARY = [k for k in bm.GATE_KINDS if k not in bm.UNARY]
BIG_LITERAL = int("8" * 80)                                 # 80 decimal digits: the tokenizer has no cap, the value wraps mod r
LITERALS = (0, 1, R - 1, BIG_LITERAL)
OLD = 8                                                     # "many levels back"


def sized(m):
    return "sized(%d)" % m


class Draw:
    def __init__(self, seed):
        self.rng = SplitMix64(seed)

    def below(self, n):
        return self.rng.next() % n

    def between(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def chance(self, num, den):
        return self.below(den) < num

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def fr(self):
        return self.rng.fr()


# ---- built circuits ---------------------------------------------------------------------------------------------------
class Tracker(pm.PackModel):
    """the model, keeping per wire the level of the boolean tape (one operation per sub-circuit, 1 + the highest level among the
    gate's operands; inputs and constants 0) and, per gate made, what its operands were"""

    def __init__(self):
        super().__init__()
        self.level = [0, 0]
        self.bit = [True, True]                             # the wire holds 0 or 1 on valid inputs
        self.gates = []                                     # (kind, set of operand classes)
        self.operands = self.old_operands = 0

    def _wire(self, kind):
        self.level.append(0)
        self.bit.append(kind == "bit")
        return super()._wire(kind)

    def _classes(self, kind, x, y, lv):
        unary = kind in bm.UNARY
        ops = [x] if unary else [x, y]
        out = set()
        for w in ops:
            if w == bm.ZERO:
                out.add("zero")
            elif w == bm.ONE:
                out.add("one")
            elif self.kind[w] == "bit":
                out.add("input")
            elif self.kind[w] == "field":
                out.add("field")
            else:
                out.add("output")
                self.operands += 1
                if lv - self.level[w] >= OLD:
                    out.add("old")
                    self.old_operands += 1
        if not unary:
            if x == y:
                out.add("same")
            elif self.kind[x] == "bit" and self.kind[y] == "bit":
                out.add("two_inputs")
        return out

    def gate(self, kind, x, y=None):
        lv = 1 + max(self.level[x], 0 if kind in bm.UNARY else self.level[y])
        self.gates.append((kind, self._classes(kind, x, y, lv)))
        first = len(self.kind)
        out = super().gate(kind, x, y)
        for w in range(first, len(self.kind)):
            self.level[w] = lv
            self.bit[w] = self.bit[x] and (kind in bm.UNARY or self.bit[y])
        if kind == "nand":
            self.level[out] = lv + 1                        # NOT of the AND
        return out

    def _linear(self, out, wires):
        self.level[out] = 1 + max([self.level[w] for w in wires] or [0])
        self.bit[out] = False

    def sub_circuit(self, left, right, with_out=True):
        """a general sub-circuit or a pack; a gate sets its own level and bit-ness over this afterwards"""
        out = super().sub_circuit(left, right, with_out)
        if with_out:
            self._linear(out, [w for _, w in list(left) + list(right)])
        return out


def apply(op, b, pool):
    """one operation of a plan on a builder-like object; operands are positions in `pool`, which takes what the operation returns"""
    what = op[0]
    at = lambda refs: None if refs is None else [pool[k] for k in refs]   # noqa: E731
    if what == "gate":
        pool.append(b.gate(op[1], pool[op[2]], None if op[3] is None else pool[op[3]]))
    elif what == "bitwise":
        pool += b.bitwise(op[1], at(op[2]), at(op[3]))
    elif what == "fan_in":
        pool.append(b.fan_in(op[1], at(op[2])))
    elif what == "compare":
        pool.append(b.compare(op[1], at(op[2]), at(op[3])))
    elif what == "assert_bit":
        b.assert_bit(pool[op[1]])
    elif what == "pack":
        pool.append(b.pack(at(op[1])))
    else:
        pool.append(b.sub_circuit([(c, pool[k]) for c, k in op[1]], [(c, pool[k]) for c, k in op[2]]))


def _replay(plan, n_bits, n_field, verify):
    def case(b):
        pool = [bm.ZERO, bm.ONE] + b.new_bits(n_bits) + [b.new_field() for _ in range(n_field)]
        for op in plan:
            apply(op, b, pool)
        return [pool[k] for k in verify]
    return case


class BuiltDraw:
    """draws a plan while replaying it on a Tracker of its own, so that levels, bit-ness and wire identity are known to the draw"""

    def __init__(self, shape, seed):
        self.d = Draw(seed * 1000003 + sum(ord(c) * 131 ** i for i, c in enumerate(shape)) % 999983)
        self.shape, self.seed = shape, seed
        self.t = Tracker()
        self.plan = []
        self.pool = [bm.ZERO, bm.ONE]                       # wire ids in the Tracker, by pool index
        self.outs = []                                      # pool indices of readable outputs
        self.wide = None

    # -- plumbing: an operation goes to the plan and to the tracker at once
    def inputs(self, n_bits, n_field=0):
        self.n_bits, self.n_field = n_bits, n_field
        self.ins = list(range(2, 2 + n_bits))
        self.fields = list(range(2 + n_bits, 2 + n_bits + n_field))
        self.pool += self.t.new_bits(n_bits) + [self.t.new_field() for _ in range(n_field)]

    def add(self, op, readable=True):
        self.plan.append(op)
        before = len(self.pool)
        apply(op, self.t, self.pool)
        made = list(range(before, len(self.pool)))
        if readable:
            self.outs += made
        return made

    # -- operands
    def operand(self, old_share=3):
        """an input, a constant or an earlier output; one output in `old_share` is drawn from all of them, the others from the last 8"""
        d = self.d
        roll = d.below(100)
        if roll < 4:
            return bm.ZERO
        if roll < 8:
            return bm.ONE
        if roll < 24 or not self.outs:
            return d.pick(self.ins + self.fields)
        if d.chance(1, old_share):
            return d.pick(self.outs)
        return d.pick(self.outs[-8:])

    def operands(self, n, repeat=True):
        got = [self.operand() for _ in range(n)]
        if repeat and n > 1 and self.d.chance(1, 3):
            got[self.d.below(n)] = got[self.d.below(n)]     # the same wire twice in one operation
        return got

    def kind(self):
        """every kind, XOR and XNOR a little more often: they keep a wire's value depending on the inputs"""
        return self.d.pick(("xor", "xnor")) if self.d.chance(1, 4) else self.d.pick(bm.GATE_KINDS)

    def one_gate(self):
        kind, x = self.kind(), self.operand()
        y = None if kind in bm.UNARY else (x if self.d.chance(1, 8) else self.operand())
        self.add(("gate", kind, x, y))

    def old_gate(self):
        """a binary gate on the newest output and one of the oldest: the operand the fixed cases never have"""
        if len(self.outs) < 40:
            return self.one_gate()
        pair = [self.outs[-1], self.d.pick(self.outs[:12])]
        if self.d.chance(1, 2):
            pair.reverse()
        self.add(("gate", self.d.pick(BINARY), pair[0], pair[1]))

    def mixed_op(self, small=False):
        d = self.d
        roll = d.below(100)
        if roll < 45:
            self.one_gate()
        elif roll < 60:
            self.old_gate()
        elif roll < 70:
            n = d.between(1, 4 if small else 9)
            kind = self.kind()
            self.add(("bitwise", kind, self.operands(n), None if kind in bm.UNARY else self.operands(n)))
        elif roll < 82:
            n = 1 if d.chance(1, 4) else d.between(2, 4 if small else 9)
            self.add(("fan_in", d.pick(BINARY), self.operands(n)))
        elif roll < 92:
            kind = d.pick(bm.CMP_KINDS)
            n = 1 if d.chance(1, 4) else d.between(2, 2 if small else 9)
            self.add(("compare", kind, self.operands(n), None if kind == "is_equal_zero" else self.operands(n)))
        else:
            bits = [k for k in [self.operand() for _ in range(4)] if self.t.bit[self.pool[k]]]
            if bits:
                self.add(("assert_bit", bits[0]))

    def subs(self):
        return len(self.t.subs)

    def m(self):
        return len(self.t.kind) - 1                         # every wire but the constant zero

    # -- the shapes
    def chain(self):
        """every sub-circuit one level above the one before; odd seeds add the (older, older) pattern, which is what makes a level two wide"""
        d = self.d
        self.inputs(d.between(5, 19))
        strict = self.seed % 2 == 0
        target = d.between(200, 380)
        prev = self.add(("gate", "xor", self.ins[0], self.ins[1]))[0]
        step = 0
        while self.subs() < target:
            older = d.pick(self.ins) if len(self.outs) < 3 or d.chance(1, 2) else d.pick(self.outs[:-1])
            pattern = step % (4 if strict else 5)
            step += 1
            roll = d.below(100)
            if roll < 8:
                self.add(("assert_bit", prev))
                continue
            if roll < 16:
                prev = self.add(("gate", d.pick(bm.UNARY) if d.chance(1, 4) else "not", prev, None))[0]
                continue
            if roll < 24:
                prev = self.add(("fan_in", d.pick(("xor", "xnor", "or", "nand")), [prev] + [d.pick(self.ins + self.outs) for _ in range(d.between(1, 4))]))[0]
                continue
            kind = d.pick(("xor", "xnor")) if d.chance(1, 2) else d.pick(BINARY)
            const = d.pick((bm.ZERO, bm.ONE))
            if strict and pattern == 3:
                pattern = 4
            x, y = ((prev, prev), (prev, older), (older, prev), (older, older), (prev, const))[pattern]
            if pattern == 4 and d.chance(1, 2):
                x, y = y, x
            made = self.add(("gate", kind, x, y))[0]
            if pattern != 3:
                prev = made

    def grow(self, lo, hi, small=False):
        target = self.d.between(lo, hi)
        while self.subs() < target:
            self.mixed_op(small)

    def mixed(self):
        self.inputs(self.d.between(9, 40))
        self.grow(300, 500)

    def wide_shape(self):
        """one level of more than 1100 boolean operations over the inputs and constants alone, then about 100 operations over its outputs"""
        d = self.d
        self.inputs(d.between(33, 70))
        src = self.ins + [bm.ZERO, bm.ONE]
        while True:
            n = d.between(20, 64)
            kind = self.kind()
            xs = [d.pick(src) for _ in range(n)]
            ys = None if kind in bm.UNARY else [d.pick(src) for _ in range(n)]
            self.add(("bitwise", kind, xs, ys))
            if self.level_one() >= 1100:
                break
        self.grow(self.subs() + 90, self.subs() + 110)
        while self.level_one() % 64 == 0:
            self.add(("gate", "and", self.ins[0], self.ins[1]))
        self.wide = self.level_one()

    def level_one(self):
        return sum(1 for w in range(2, len(self.t.kind)) if self.t.kind[w] == "out" and self.t.level[w] == 1)

    def packs(self):
        d = self.d
        self.inputs(d.between(9, 40))
        widths = list(PACK_WIDTHS) + [d.between(1, pm.PACK_MAX_BITS) for _ in range(6)]
        self.grow(120, 160)
        for width in widths:
            bits = [self.operand(old_share=2) for _ in range(width)]
            if width > 2:
                bits[d.below(width)] = bm.ZERO
                bits[d.below(width)] = bm.ONE
                bits[-1] = bits[0]                          # a wire at two positions, the top bit among them
            self.add(("pack", bits), readable=False)
            self.grow(self.subs() + 3, self.subs() + 15, small=True)
        self.grow(300, 480, small=True)

    def side(self):
        """a side of a general sub-circuit: only constants, only the zero wire, or 1..4 weighted wires"""
        d = self.d
        weight = lambda: d.pick(WEIGHTS) if d.chance(1, 2) else (d.fr() if d.chance(1, 2) else d.between(2, 9))   # noqa: E731
        roll = d.below(10)
        if roll == 0:
            return [(weight(), bm.ZERO) for _ in range(d.between(1, 2))]
        if roll == 1:
            return [(weight(), bm.ONE) for _ in range(d.between(1, 3))]
        return [(weight(), self.operand()) for _ in range(d.between(1, 4))]

    def field(self):
        d = self.d
        self.inputs(d.between(9, 24), d.between(2, 5))
        target = d.between(150, 260)
        packed = []
        while self.subs() < target:
            roll = d.below(100)
            if roll < 30:
                left = self.side()
                self.add(("sub", left, list(left) if d.chance(1, 6) else self.side()))
            elif roll < 38:
                packed += self.add(("pack", self.operands(d.pick((1, 2, 7, 64, 65, 130)))))
            elif roll < 46 and packed:
                self.add(("gate", d.pick(BINARY), d.pick(packed), self.operand()))      # a packed wire read by a gate
            elif roll < 56:
                self.old_gate()
            else:
                self.mixed_op(small=True)

    def sized(self, m):
        self.inputs(self.d.between(5, 12))
        while self.m() + 16 <= m:
            self.mixed_op(small=True)
        while self.m() < m:
            x = self.outs[-1] if self.outs else self.ins[0]
            self.add(("gate", "xor", x, self.d.pick(self.ins)))
        assert self.m() == m

    def finish(self):
        d = self.d
        by_wire = {}
        for k in range(2, len(self.pool)):                  # (fan_in of one wire returns that wire: two pool entries, one id)
            if self.pool[k] >= 2:
                by_wire.setdefault(self.pool[k], k)
        candidates = list(by_wire.values())
        verify = []
        for _ in range(d.between(1, 6)):
            verify.append(candidates.pop(d.below(len(candidates))))
        case = _replay(self.plan, self.n_bits, self.n_field, verify)
        t = self.t
        case.shape, case.seed, case.plan, case.verify = self.shape, self.seed, self.plan, verify
        case.census = dict(gates=t.gates, wide=self.wide, subs=len(t.subs), operands=t.operands, old_operands=t.old_operands,
                           fan_in=[len(op[2]) for op in self.plan if op[0] == "fan_in"],
                           compare=[(op[1], len(op[2])) for op in self.plan if op[0] == "compare"],
                           packs=[len(op[1]) for op in self.plan if op[0] == "pack"])
        return case


def built_case(shape, seed):
    g = BuiltDraw(shape, seed)
    if shape.startswith("sized("):
        g.sized(int(shape[6:-1]))
    else:
        {"chain": g.chain, "wide": g.wide_shape, "mixed": g.mixed, "packs": g.packs, "field": g.field}[shape]()
    return g.finish()


def built_inputs(model, seed, count):
    """per instance the inputs in creation order: bits for bit wires, field elements for field wires; instance 0 all zero, instance 1
    all one (as random_bits of the device tests), field inputs of instance 2 all r - 1"""
    d = Draw(seed)
    kinds = [k for k in model.kind if k in ("bit", "field")]
    rows = []
    for j in range(count):
        if j < 2:
            rows.append([j] * len(kinds))
        else:
            rows.append([d.below(2) if k == "bit" else (R - 1 if j == 2 else d.fr()) for k in kinds])
    return rows


def built_tape_shape(fin):
    """built_compile_tape's counting on a builder_model.Finished: (ops, slots, consts, levels, widest level)"""
    level, pool, per_level = {}, set(), {}
    count = dict(ops=0, slots=fin.m)

    def emit(a, b, fresh=True):
        lv = 1 + max(a, b)
        per_level[lv] = per_level.get(lv, 0) + 1
        count["ops"] += 1
        count["slots"] += fresh
        return lv

    def side(terms):
        acc = None
        for c, i in terms:
            if i == 0:
                pool.add(c)
                v = 0
            elif c == 1:
                v = level.get(i, 0)
            else:
                pool.add(c)
                v = emit(0, level.get(i, 0))
            acc = v if acc is None else emit(acc, v)
        if acc is None:
            pool.add(0)
            return 0
        return acc

    for l, r, o in fin.subs:
        if o is None:
            continue
        left = side(l)
        level[o] = emit(left, left if l == r else side(r), fresh=False)
    return count["ops"], count["slots"], len(pool), len(per_level), max(per_level.values())


# ---- .zk programs ---------------------------------------------------------------------------------------------------------
# an expression is ("lit", n) | ("var", name) | ("add", [expressions]) | ("mul", a, b); an ast is
# dict(ins=[names], outs=[names], verify=[names], program=[(name, expression)])
def render(e):
    if e[0] == "lit":
        return str(e[1])
    if e[0] == "var":
        return e[1]
    if e[0] == "add":
        return "(+ " + " ".join(render(k) for k in e[1]) + ")"
    return "(* %s %s)" % (render(e[1]), render(e[2]))


def source(ast):
    lines = ["(in %s)" % " ".join(ast["ins"]), "(out %s)" % " ".join(ast["outs"]), "(verify %s)" % " ".join(ast["verify"]), "(program"]
    lines += ["(= %s %s)" % (v, render(e)) for v, e in ast["program"]]
    return "\n".join(lines) + ")\n"


def variables(e):
    if e[0] == "var":
        return [e[1]]
    if e[0] == "lit":
        return []
    return [v for k in (e[1] if e[0] == "add" else e[1:]) for v in variables(k)]


def variable_order(ast):
    """first appearance behind `verify`: the witness order"""
    order = list(ast["verify"])
    for v, e in ast["program"]:
        for name in [v] + variables(e):
            if name not in order:
                order.append(name)
    return order


def eval_ast(ast, inputs):
    """the witness as integers: [1], then the variables in their order"""
    env = dict(zip(ast["ins"], inputs))

    def ev(e):
        if e[0] == "lit":
            return e[1] % R
        if e[0] == "var":
            return env[e[1]]
        return ev(e[1]) * ev(e[2]) % R if e[0] == "mul" else sum(ev(k) for k in e[1]) % R

    for v, e in ast["program"]:
        env[v] = ev(e)
    return [1] + [env[v] for v in variable_order(ast)]


def literals(ast):
    def walk(e):
        if e[0] == "lit":
            return [e[1] % R]
        if e[0] == "var":
            return []
        return [x for k in (e[1] if e[0] == "add" else e[1:]) for x in walk(k)]
    return [x for _, e in ast["program"] for x in walk(e)]


def program_tape_shape(ast):
    """compile_tape's counting: (ops, slots, consts, levels, widest level); inputs that are no witness wire get a slot behind the
    witness, an operation writes the assignment's slot where it is the outermost one and a fresh one otherwise"""
    order = variable_order(ast)
    level = {v: 0 for v in ast["ins"]}
    pool, per_level = set(), {}
    count = dict(ops=0, slots=len(order) + 1 + sum(1 for v in ast["ins"] if v not in order))

    def emit(a, b, fresh):
        lv = 1 + max(a, b)
        per_level[lv] = per_level.get(lv, 0) + 1
        count["ops"] += 1
        count["slots"] += fresh
        return lv

    def expr(e, top):
        """-> (level, whether an operation produced it)"""
        if e[0] == "lit":
            pool.add(e[1] % R)
            return 0, False
        if e[0] == "var":
            return level[e[1]], False
        if e[0] == "mul":
            a, b = expr(e[1], False)[0], expr(e[2], False)[0]
            return emit(a, b, not top), True
        if len(e[1]) == 1:
            return expr(e[1][0], top)
        acc = expr(e[1][0], False)[0]
        for i, k in enumerate(e[1][1:]):
            acc = emit(acc, expr(k, False)[0], not (top and i == len(e[1]) - 2))
        return acc, True

    for v, e in ast["program"]:
        lv, made = expr(e, True)
        level[v] = lv if made else emit(lv, 0, False)       # a bare variable or literal is copied
    return count["ops"], count["slots"], len(pool), len(per_level), max(per_level.values())


class ProgramDraw:
    """A gate may read any input and any earlier target: a name it meets first becomes a wire there, in the order of the text.  A
    right-hand side that emits no constraint makes no wire, so it reads only names that are wires already (`seen`) -- the witness
    order, first appearance in the text, must stay the order in which wires are made.  The one exception is drawn on purpose: the
    input `late` is first read by such a right-hand side, and the assignment behind it, to the verify variable `pub` (a wire from the
    start), names `late` first."""

    def __init__(self, shape, seed):
        self.d = Draw(seed * 7919 + 17 * PROGRAM_SHAPES.index(shape) + 5)
        self.shape, self.seed = shape, seed
        self.strict = shape == "chain" and seed % 2 == 0    # one tape operation per level
        self.ins = ["a%d" % i for i in range(self.d.between(3, 12))]
        self.wires = set()
        self.targets, self.program = [], []
        self.favourite = LITERALS[seed % len(LITERALS)]     # drawn again and again: the constant pool holds it once

    def literal(self):
        roll = self.d.below(10)
        if roll < 3:
            return ("lit", self.favourite)
        if roll < 6:
            return ("lit", self.d.pick(LITERALS))
        return ("lit", self.d.between(2, 250) if roll < 9 else self.d.fr())

    def assign(self, name, e):
        self.program.append((name, e))
        self.targets.append(name)
        self.wires.update([name] + variables(e))

    def older(self):
        if self.shape == "wide":
            return self.d.pick(self.ins)
        if self.shape == "mixed" and self.targets and self.d.chance(2, 3):
            return self.d.pick(self.targets[-6:])
        return self.d.pick(self.ins + self.targets)

    def seen(self):
        pool = [v for v in self.ins + self.targets if v in self.wires]
        if self.shape == "wide":
            pool = [v for v in pool if v in self.ins]
        if self.shape == "mixed" and self.d.chance(2, 3):
            pool = pool[-6:]
        return self.d.pick(pool or [self.targets[-1]])

    def term(self):
        roll = self.d.below(10)
        if roll < 2:
            return self.literal()
        if roll < 6:
            return ("var", self.older())
        return ("mul", self.literal(), ("var", self.older()))

    def side(self):
        roll = self.d.below(10)
        if roll < 1:
            return self.literal()
        if roll < 4:
            return ("var", self.older())
        return ("add", [self.term() for _ in range(self.d.between(1, 5))])

    def nested(self, depth):
        d = self.d
        if depth == 0 or d.chance(1, 5):
            return ("var", self.seen()) if d.chance(2, 3) else self.literal()
        if d.chance(1, 2):
            return ("mul", self.nested(depth - 1), self.nested(depth - 1))
        return ("add", [self.nested(depth - 1) for _ in range(d.between(1, 3))])

    def free(self):
        """a right-hand side that emits no constraint and is evaluated all the same: anything but a `*` at the top"""
        roll = self.d.below(8)
        if roll == 0:
            return ("var", self.seen())
        if roll == 1:
            return self.literal()
        if roll == 2:
            return ("add", [("var", self.seen())])
        if roll == 3:
            return ("add", [self.literal(), ("var", self.seen())])
        return ("add", [self.nested(5) for _ in range(self.d.between(1, 3))])    # six deep with the `+` on top

    def strict_link(self, p):
        """reads the target before it so that every tape operation does: one side may be a sum or a scaled term over p"""
        d = self.d
        lit, old = self.literal(), ("var", self.older())
        roll = d.below(10)
        if roll == 0:
            return d.pick([p, ("add", [p]), ("add", [p, lit])])
        simple = d.pick([p, old, lit])
        rich = d.pick([p, ("add", [p, lit]), ("add", [lit, p]), ("add", [old, p]), ("add", [p, old]), ("add", [("mul", lit, p)]),
                       ("add", [p, ("mul", self.literal(), p)])])
        return ("mul", rich, simple) if d.chance(1, 2) else ("mul", simple, rich)

    def loose_link(self, p, count):
        o = ("var", self.older())
        x, y = ((p, p), (p, self.side()), (self.side(), p), (o, self.side()), (p, self.literal()))[count % 5]
        return ("mul", x, y) if self.d.chance(4, 5) else self.free()

    def build(self):
        d = self.d
        n = 300 if self.shape == "wide" else (40 if self.seed % 3 == 0 else d.between(41, 300))
        special_at = None if self.strict else d.between(2, n - 3)
        self.assign("v0", ("mul", ("var", self.ins[0]), ("var", self.ins[0])))
        while len(self.program) < n:
            count = len(self.program)
            name = "v%d" % count
            if count == special_at:
                z = ("var", "late")
                self.assign(name, ("add", [z, ("mul", z, ("add", [z, ("lit", 2)]))]))
                self.assign("pub", ("mul", z, self.side()))
                continue
            if self.shape == "chain":
                p = ("var", self.targets[-1])
                e = self.strict_link(p) if self.strict else self.loose_link(p, count)
            else:
                e = ("mul", self.side(), self.side()) if d.chance(3, 4) else self.free()
            self.assign(name, e)
        named = [t for t in self.targets if t != "pub"]
        verify = [] if self.strict else ["pub"]
        for _ in range(d.between(1, 3)):
            t = d.pick(named)
            if t not in verify:
                verify.append(t)
        if self.ins[0] not in verify and d.chance(1, 2):
            verify.append(self.ins[0])                      # a public input: a wire no assignment makes
        ins = self.ins + ["unread"] + ([] if self.strict else ["late"])
        return dict(ins=ins, outs=[t for t in self.targets if t not in verify], verify=verify, program=self.program)


def program(shape, seed):
    ast = ProgramDraw(shape, seed).build()
    return source(ast), ast


def program_inputs(ast, seed, count):
    """instance 0 all zero, instance 1 all one, instance 2 all r - 1, the rest drawn"""
    d = Draw(seed)
    n = len(ast["ins"])
    return ([[0] * n, [1] * n, [R - 1] * n] + [[d.fr() for _ in range(n)] for _ in range(max(count - 3, 0))])[:count]

