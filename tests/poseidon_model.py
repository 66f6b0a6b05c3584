"""Poseidon over the BN254 scalar field restated in Python integers: the model tests/test_poseidon.py and tests/test_gpu_poseidon.py
hold the library against.  Nothing here calls the library.

    grain_bits / grain_int   the Poseidon paper's Grain LFSR, written twice (a list of bits; one 80-bit integer): the published known
                             answers pin three widths and a handful of inputs, the two generators pin each other everywhere else
    params(t)                round constants and the Cauchy matrix M[i][j] = 1 / (x_i + y_j) from that stream
    hash, zero_hashes        state [0, inputs...], x^5, R_F = 8 full rounds around R_P partial ones; z_0 = 0, z_{k+1} = hash(z_k, z_k)
    tree_levels, path, fold  the binary tree that stores only nodes with a leaf under them, and its authentication paths
    Gadget                   the builder's Poseidon and Merkle-path gadgets over linear forms, emitting builder_model sub-circuits
"""
from builder_model import Model, ONE, ZERO

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R_F = 8
R_P = {2: 56, 3: 57, 5: 60}
TAPS = (62, 51, 38, 23, 13, 0)


def _seed_fields(t):
    return [(1, 2), (0, 4), (254, 12), (t, 12), (R_F, 10), (R_P[t], 10), ((1 << 30) - 1, 30)]


# ---- Grain, first time: a list of 80 bits, b[0] the oldest -------------------------------------------
def grain_bits(t):
    b = []
    for value, width in _seed_fields(t):
        b += [(value >> (width - 1 - i)) & 1 for i in range(width)]
    assert len(b) == 80

    def step():
        new = 0
        for k in TAPS:
            new ^= b[k]
        b.pop(0)
        b.append(new)
        return new

    for _ in range(160):
        step()
    while True:
        bit = step()
        while bit == 0:
            step()
            bit = step()
        yield step()


# ---- Grain, second time: one integer, bit 79 the oldest; the self-shrinking rule as "draw pairs, keep the second of a pair that
# starts with 1" -------------------------------------------------------------------------------------------------------------------
def grain_int(t):
    s = 0
    for value, width in _seed_fields(t):
        s = (s << width) | value
    mask = (1 << 80) - 1

    def step(s):
        new = 0
        for k in TAPS:
            new ^= (s >> (79 - k)) & 1
        return ((s << 1) & mask) | new, new

    for _ in range(160):
        s, _ = step(s)
    while True:
        s, first = step(s)
        s, second = step(s)
        if first:
            yield second


def _elements(bits):
    while True:
        x = 0
        for _ in range(254):
            x = (x << 1) | next(bits)
        yield x


_PARAMS = {}


def params(t, grain=grain_bits):
    """(round constants [(R_F + R_P) t], M [t][t]) as integers"""
    key = (t, grain.__name__)
    if key not in _PARAMS:
        draw = _elements(grain(t))
        c = []
        while len(c) < (R_F + R_P[t]) * t:
            x = next(draw)
            if x < R:
                c.append(x)
        while True:
            xy = [next(draw) % R for _ in range(2 * t)]
            xs, ys = xy[:t], xy[t:]
            if len(set(xy)) == 2 * t and all((x + y) % R for x in xs for y in ys):
                break
        m = [[pow(x + y, R - 2, R) for y in ys] for x in xs]
        _PARAMS[key] = (c, m)
    return _PARAMS[key]


def permute(state):
    t = len(state)
    c, m = params(t)
    rp = R_P[t]
    for rnd in range(R_F + rp):
        state = [(x + c[rnd * t + i]) % R for i, x in enumerate(state)]
        if rnd < 4 or rnd >= 4 + rp:
            state = [pow(x, 5, R) for x in state]
        else:
            state[0] = pow(state[0], 5, R)
        state = [sum(m[i][j] * state[j] for j in range(t)) % R for i in range(t)]
    return state


def hash(inputs):   # noqa: A001 -- the issue's name
    assert len(inputs) in (1, 2, 4) and all(0 <= x < R for x in inputs)
    return permute([0] + list(inputs))[0]


def zero_hashes(depth):
    z = [0]
    for _ in range(depth):
        z.append(hash([z[-1], z[-1]]))
    return z


def level_size(n_leaves, level):
    return n_leaves if level == 0 else max(1, (n_leaves + (1 << level) - 1) >> level)


def tree_levels(leaves, depth):
    """levels[k] = the stored nodes of level k: ceil(n / 2^k), at least one from level 1 up; a missing child of level k is z_k"""
    assert len(leaves) <= 1 << depth
    z = zero_hashes(depth)
    levels = [list(leaves)]
    for k in range(depth):
        below = levels[-1]
        get = lambda i: below[i] if i < len(below) else z[k]   # noqa: E731
        levels.append([hash([get(2 * i), get(2 * i + 1)]) for i in range(level_size(len(leaves), k + 1))])
    return levels


def tree_root(levels, depth):
    return levels[depth][0] if levels[depth] else 0       # the empty tree of depth 0


def path(levels, depth, index):
    """(leaf, siblings of levels 0 .. depth - 1, direction bits)"""
    z = zero_hashes(depth)
    sibs = []
    for k in range(depth):
        s = (index >> k) ^ 1
        sibs.append(levels[k][s] if s < len(levels[k]) else z[k])
    return levels[0][index], sibs, [(index >> k) & 1 for k in range(depth)]


def fold(leaf, sibs, dirs):
    cur = leaf
    for s, d in zip(sibs, dirs):
        cur = hash([s, cur]) if d else hash([cur, s])
    return cur


# ---- the gadgets --------------------------------------------------------------------------------------
def form_of(wire):
    """a linear form over wires: {wire: weight}, the constant carried on wire ONE; the constant-zero wire is the empty form"""
    return {} if wire == ZERO else {wire: 1}


def form_add(a, b, scale=1):
    out = dict(a)
    for w, c in b.items():
        v = (out.get(w, 0) + scale * c) % R
        if v:
            out[w] = v
        else:
            out.pop(w, None)
    return out


def form_terms(f):
    return [(c, w) for w, c in sorted(f.items())]


class Gadget(Model):
    """builder_model.Model with the Poseidon gadgets"""

    def _sbox(self, f):
        a = self.sub_circuit(form_terms(f), form_terms(f))
        c = self.sub_circuit([(1, a)], [(1, a)])
        return form_of(self.sub_circuit([(1, c)], form_terms(f)))

    def poseidon_forms(self, forms):
        t = len(forms) + 1
        c, m = params(t)
        rp = R_P[t]
        state = [{}] + [dict(f) for f in forms]
        for rnd in range(R_F + rp):
            state = [form_add(f, {ONE: c[rnd * t + i]}) for i, f in enumerate(state)]
            if rnd < 4 or rnd >= 4 + rp:
                state = [self._sbox(f) for f in state]
            else:
                state[0] = self._sbox(state[0])
            mixed = []
            for i in range(t):
                acc = {}
                for j in range(t):
                    acc = form_add(acc, state[j], m[i][j])
                mixed.append(acc)
            state = mixed
        return self.sub_circuit(form_terms(state[0]), [(1, ONE)])

    def poseidon(self, wires):
        return self.poseidon_forms([form_of(w) for w in wires])

    def merkle_root(self, leaf, siblings, dirs):
        cur = leaf
        for sib, d in zip(siblings, dirs):
            self.assert_bit(d)
            diff = form_add(form_of(sib), form_of(cur), -1)
            delta = self.sub_circuit([(1, d)], form_terms(diff))
            cur = self.poseidon_forms([form_add(form_of(cur), form_of(delta)), form_add(form_of(sib), form_of(delta), -1)])
        return cur


def gate_count(arity):
    t = arity + 1
    return 3 * (R_F * t + R_P[t]) + 1
