"""Baby Jubjub in Python integers: the model tests/test_babyjub*.py and tests/test_gpu_babyjub.py hold the library against.  Written
from the equations, nothing here calls the library.

    the curve     a x^2 + y^2 = 1 + d x^2 y^2 over Fr, a = 168700, d = 168696, identity (0, 1); BASE8 of prime order L, GENERATOR of
                  order 8 L, BASE8 = 8 GENERATOR
    add, neg, mul             the affine law (complete: a is a square, d is not) and the scalar multiple by any integer >= 0
    padd, pdbl, to_affine     add-2008-bbjlp and dbl-2008-bbjlp for general a on (X : Y : Z)
    derive()                  the facts the constants rest on, re-derived: on-curve, orders, a square, d non-square, low-order points
    Gadget                    poseidon_model.Gadget with the five curve gadgets, emitting the rows the builder must emit
    fixed_gates, var_gates    gate counts as functions of n_bits
"""
from builder_model import ONE, R
from poseidon_model import Gadget as PoseidonGadget, form_add, form_of, form_terms

A, D = 168700, 168696
IDENTITY = (0, 1)
BASE8 = (5299619240641551281634865583518297030282874472190772894086521144482721001553,
         16950150798460657717958625567821834550301663161624707787222815936182638968203)
GENERATOR = (995203441582195749578291179787384436505546430278305826713579947235728471134,
             5472060717959818805561601436314318772137091100104008585924551046643952123905)
L = 2736030358979909402780800718157159386076813972158567259200215660948447373041
X4 = 18930368022820495955728484915491405972470733850014661777449844430438130630919   # (X4, 0) and (-X4, 0) have order 4
FIXED_WINDOW = 3                                         # the gadget's window; the kernel's is the library's babyjub.FIXED_WINDOW


def inv(x):
    return pow(x, R - 2, R)


def on_curve(p):
    x, y = p
    return (A * x * x + y * y - 1 - D * x * x * y * y) % R == 0


def add(p, q):
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * inv(1 + t) % R, (y1 * y2 - A * x1 * x2) * inv(1 - t) % R)


def neg(p):
    return ((-p[0]) % R, p[1])


def mul(k, p=BASE8):
    acc = IDENTITY
    for i in reversed(range(k.bit_length())):
        acc = add(acc, acc)
        if (k >> i) & 1:
            acc = add(acc, p)
    return acc


def padd(p, q):
    (x1, y1, z1), (x2, y2, z2) = p, q
    a = z1 * z2 % R
    b = a * a % R
    c = x1 * x2 % R
    d = y1 * y2 % R
    e = c * d % R
    h = (x1 + y1) * (x2 + y2) % R
    f, g = (b - D * e) % R, (b + D * e) % R
    return (a * f % R * (h - c - d) % R, a * g % R * (d - A * c) % R, f * g % R)


def pdbl(p):
    x, y, z = p
    b = (x + y) ** 2 % R
    c, d, h = x * x % R, y * y % R, z * z % R
    e = A * c % R
    f = (e + d) % R
    j = (f - 2 * h) % R
    return ((b - c - d) * j % R, f * (e - d) % R, f * j % R)


def to_affine(p):
    zi = inv(p[2])
    return (p[0] * zi % R, p[1] * zi % R)


def pmul(k, p=BASE8):
    """mul through the projective formulas, one inversion at the end: the reference of the large GPU cases (test_babyjub.py holds
    the formulas against the affine law)"""
    acc, q = (0, 1, 1), (p[0], p[1], 1)
    for i in reversed(range(k.bit_length())):
        acc = pdbl(acc)
        if (k >> i) & 1:
            acc = padd(acc, q)
    return to_affine(acc)


def edge_points():
    """identity, order 2, both of order 4, Base8, Generator, L * Generator, a few multiples, and the negatives"""
    pts = [IDENTITY, (0, R - 1), (X4, 0), (R - X4, 0), BASE8, GENERATOR, mul(L, GENERATOR), mul(2, BASE8), mul(3, GENERATOR), mul(L + 5, GENERATOR)]
    out = []
    for p in pts + [neg(p) for p in pts]:
        if p not in out:
            out.append(p)
    return out


EDGE_SCALARS = [0, 1, 2, 7, 8, L - 1, L, L + 1, 8 * L, R - 1, 1 << 255, (1 << 256) - 1]


def derive():
    """every fact the constants rest on; returns the low-order points found by multiplying Generator by L, 2 L and 4 L"""
    assert on_curve(BASE8) and on_curve(GENERATOR) and on_curve(IDENTITY)
    assert pow(A, (R - 1) // 2, R) == 1 and pow(D, (R - 1) // 2, R) == R - 1
    assert mul(L, BASE8) == IDENTITY and mul(8, GENERATOR) == BASE8 and mul(8 * L, GENERATOR) == IDENTITY
    assert L.bit_length() == 251 and pow(2, L - 1, L) == 1 and pow(3, L - 1, L) == 1
    low = [mul(k * L, GENERATOR) for k in (1, 2, 4)]
    assert low[2] == (0, R - 1) and low[1][1] == 0 and low[1][0] in (X4, R - X4) and (A * X4 * X4 - 1) % R == 0
    assert mul(8, low[0]) == IDENTITY and mul(4, low[0]) != IDENTITY   # L * Generator has order exactly 8
    assert mul(4, (X4, 0)) == IDENTITY and mul(2, (X4, 0)) == (0, R - 1) and mul(2, (0, R - 1)) == IDENTITY
    return low


# ---- the gadgets --------------------------------------------------------------------------------------
def const_form(c):
    return {ONE: c % R} if c % R else {}


class Gadget(PoseidonGadget):
    """poseidon_model.Gadget with the curve gadgets.  A point is three wires (X, Y, Z); an affine point is (x, y, ONE)."""

    def assert_forms(self, left, right):
        self.sub_circuit(form_terms(left), form_terms(right), with_out=False)

    def _mulf(self, left, right):
        return self.sub_circuit(form_terms(left), form_terms(right))

    def babyjub_assert_on_curve(self, xy):
        x, y = form_of(xy[0]), form_of(xy[1])
        u = self._mulf(x, x)
        v = self._mulf(y, y)
        w = self._mulf(form_of(u), form_of(v))
        eq = form_add(form_add(form_add(form_add({}, form_of(u), A), form_of(v)), const_form(-1)), form_of(w), -D)
        self.assert_forms(eq, form_of(ONE))

    def _add_forms(self, x1, y1, z1, x2, y2, z2):
        """z2 None: q is affine (Z2 = 1) and A = Z1 costs no gate"""
        a = z1 if z2 is None else form_of(self._mulf(z1, z2))
        b = self._mulf(a, a)
        c = self._mulf(x1, x2)
        d = self._mulf(y1, y2)
        e = self._mulf(form_of(c), form_of(d))
        h = self._mulf(form_add(x1, y1), form_add(x2, y2))
        f = form_add(form_of(b), form_of(e), -D)
        g = form_add(form_of(b), form_of(e), D)
        af = self._mulf(a, f)
        ag = self._mulf(a, g)
        x3 = self._mulf(form_of(af), form_add(form_add(form_of(h), form_of(c), -1), form_of(d), -1))
        y3 = self._mulf(form_of(ag), form_add(form_of(d), form_of(c), -A))
        z3 = self._mulf(f, g)
        return [x3, y3, z3]

    def _dbl_forms(self, x, y, z):
        s = form_add(x, y)
        b = self._mulf(s, s)
        c = self._mulf(x, x)
        d = self._mulf(y, y)
        h = self._mulf(z, z)
        f = form_add(form_add({}, form_of(c), A), form_of(d))
        j = form_add(f, form_of(h), -2)
        x3 = self._mulf(form_add(form_add(form_of(b), form_of(c), -1), form_of(d), -1), j)
        y3 = self._mulf(f, form_add(form_add({}, form_of(c), A), form_of(d), -1))
        z3 = self._mulf(f, j)
        return [x3, y3, z3]

    def babyjub_add(self, p, q):
        z2 = None if q[2] == ONE else form_of(q[2])
        return self._add_forms(form_of(p[0]), form_of(p[1]), form_of(p[2]), form_of(q[0]), form_of(q[1]), z2)

    def babyjub_affine(self, p, xy):
        for k in range(2):
            t = self._mulf(form_of(xy[k]), form_of(p[2]))
            self.assert_forms(form_add(form_of(t), form_of(p[k]), -1), form_of(ONE))

    def _select(self, bits, table):
        """the two forms sum_S c_S prod_{i in S} bits[i] through table[sum 2^i bits[i]], a table of 2^len(bits) affine points"""
        n = len(bits)
        prod = {0: {ONE: 1}}                                # subset mask -> form of the product of its bits
        for i in range(n):
            prod[1 << i] = form_of(bits[i])
        if n >= 2:
            prod[3] = form_of(self._mulf(form_of(bits[0]), form_of(bits[1])))
        if n == 3:
            prod[5] = form_of(self._mulf(form_of(bits[0]), form_of(bits[2])))
            prod[6] = form_of(self._mulf(form_of(bits[1]), form_of(bits[2])))
            prod[7] = form_of(self._mulf(prod[3], form_of(bits[2])))
        out = []
        for k in range(2):
            f = {}
            for mask in range(1 << n):
                c = sum((-1) ** bin(mask ^ sub).count("1") * table[sub][k] for sub in range(1 << n) if sub & ~mask == 0) % R
                f = form_add(f, prod[mask], c)
            out.append(f)
        return out

    def babyjub_mul_fixed(self, bits):
        n = len(bits)
        assert 1 <= n <= 256
        for b in bits:
            self.assert_bit(b)
        base, acc = BASE8, None
        for at in range(0, n, FIXED_WINDOW):
            window = bits[at:at + FIXED_WINDOW]
            table = [IDENTITY]
            for _ in range((1 << len(window)) - 1):
                table.append(add(table[-1], base))
            x2, y2 = self._select(window, table)
            if acc is None:
                acc = [x2, y2, form_of(ONE)]
            else:
                acc = [form_of(w) for w in self._add_forms(acc[0], acc[1], acc[2], x2, y2, None)]
            base = mul(1 << FIXED_WINDOW, base)
        if n <= FIXED_WINDOW:                               # one window: the two forms become wires
            return [self._mulf(acc[0], form_of(ONE)), self._mulf(acc[1], form_of(ONE)), ONE]
        return [next(iter(f)) for f in acc]

    def babyjub_mul(self, p_xy, bits):
        n = len(bits)
        assert 1 <= n <= 256
        self.babyjub_assert_on_curve(p_xy)
        for b in bits:
            self.assert_bit(b)
        px, py1 = form_of(p_xy[0]), form_add(form_of(p_xy[1]), const_form(-1))

        def select(bit):                                    # bit ? P : (0, 1)
            sx = self._mulf(form_of(bit), px)
            sy = self._mulf(form_of(bit), py1)
            return sx, form_add(form_of(sy), const_form(1))

        x, y = select(bits[n - 1])
        if n == 1:
            return [x, self._mulf(y, form_of(ONE)), ONE]
        acc = [form_of(x), y, form_of(ONE)]
        for i in reversed(range(n - 1)):
            dbl = [form_of(w) for w in self._dbl_forms(*acc)]
            x2, y2 = select(bits[i])
            acc = [form_of(w) for w in self._add_forms(dbl[0], dbl[1], dbl[2], form_of(x2), y2, None)]
        return [next(iter(f)) for f in acc]


def fixed_gates(n_bits):
    full, rest = divmod(n_bits, 3)
    windows = full + (1 if rest else 0)
    products = 4 * full + (1 if rest == 2 else 0)
    return n_bits + products + (10 * (windows - 1) if windows > 1 else 2)


def var_gates(n_bits):
    return 4 + n_bits + 2 + (19 * (n_bits - 1) if n_bits > 1 else 1)
