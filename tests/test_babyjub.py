"""-m "not gpu": Baby Jubjub on the host (csrc/babyjub.hpp, zk_babyjub_params / _on_curve / _add / _mul) and the builder's gadgets
(zk_builder_babyjub_*) against tests/babyjub_model.py: the model's own identities, host arithmetic on the edge points and scalars,
refusals, gate counts, rows word for word, the three host evaluators, and what a wrong witness breaks."""
import itertools

import numpy as np
import pytest

from zksnark_rs_amd import SplitMix64, ZkError, _lib, limbs_to_ints
from zksnark_rs_amd import babyjub
from zksnark_rs_amd.circuit import Builder, BuildErr, ParseErr

import babyjub_model as bm
from gadget_cases import Pair, check_rows, check_witness, outputs, value

R = bm.R
EDGE = bm.edge_points()
GATE_COUNTS_FIXED = {1: 3, 2: 5, 3: 9, 4: 18, 6: 24, 7: 35, 251: 1414, 256: 1446}
GATE_COUNTS_VAR = {1: 8, 2: 27, 3: 47, 4: 67, 6: 107, 7: 127, 251: 5007, 256: 5107}


# ---- the model and the host functions -------------------------------------------------------------
def test_the_model_derives_its_constants():
    low = bm.derive()
    assert low[1] in ((bm.X4, 0), (R - bm.X4, 0)) and low[2] == (0, R - 1)
    assert len(EDGE) >= 16 and all(bm.on_curve(p) for p in EDGE)
    p = babyjub.params()
    assert (p["a"], p["d"], p["order"], p["base8"], p["generator"]) == (bm.A, bm.D, bm.L, bm.BASE8, bm.GENERATOR)


def test_the_projective_formulas_are_the_affine_law_on_all_pairs():
    rng = SplitMix64(7)
    for p, q in itertools.product(EDGE, repeat=2):
        z1, z2 = rng.fr() or 1, rng.fr() or 1
        pp, qq = (p[0] * z1 % R, p[1] * z1 % R, z1), (q[0] * z2 % R, q[1] * z2 % R, z2)
        s = bm.padd(pp, qq)
        assert s[2] != 0 and bm.to_affine(s) == bm.add(p, q)
        assert bm.to_affine(bm.padd(pp, (q[0], q[1], 1))) == bm.add(p, q)
    for p in EDGE:
        z = rng.fr() or 1
        d = bm.pdbl((p[0] * z % R, p[1] * z % R, z))
        assert d[2] != 0 and bm.to_affine(d) == bm.add(p, p)


def test_host_add_on_all_pairs_of_edge_points():
    for p, q in itertools.product(EDGE, repeat=2):
        assert babyjub.add(p, q) == bm.add(p, q), (p, q)
    for p in EDGE:
        assert babyjub.add(p, bm.neg(p)) == bm.IDENTITY and babyjub.add(p, p) == bm.mul(2, p)
        assert babyjub.on_curve(p)


def test_host_mul_on_edge_points_and_scalars():
    rng = SplitMix64(11)
    scalars = bm.EDGE_SCALARS + [rng.fr() | (rng.fr() << 200) & ((1 << 256) - 1) for _ in range(3)]
    for k in scalars:
        assert babyjub.mul(k) == bm.mul(k), k
    for p in EDGE:
        for k in bm.EDGE_SCALARS:
            assert babyjub.mul(k, p) == bm.mul(k, p), (k, p)
    assert babyjub.mul(bm.L) == bm.IDENTITY and babyjub.mul(8, bm.GENERATOR) == bm.BASE8
    assert babyjub.mul(bm.L, bm.GENERATOR) != bm.IDENTITY      # the scalar is an integer, not reduced mod l


def test_refusals():
    off = (bm.BASE8[0], (bm.BASE8[1] + 1) % R)
    assert not bm.on_curve(off) and babyjub.on_curve(off) is False
    for bad in ((R, 1), (0, R), ((1 << 256) - 1, 1)):
        for call in (lambda: babyjub.on_curve(bad), lambda: babyjub.add(bad, bm.BASE8), lambda: babyjub.add(bm.BASE8, bad), lambda: babyjub.mul(3, bad)):
            with pytest.raises(ZkError) as e:
                call()
            assert e.value.status == _lib.ZK_ERR_RANGE
    for call in (lambda: babyjub.add(off, bm.BASE8), lambda: babyjub.add(bm.BASE8, off), lambda: babyjub.mul(3, off)):
        with pytest.raises(ZkError) as e:
            call()
        assert e.value.status == _lib.ZK_ERR_RANGE               # the status of an uploaded CRS point off its curve
    lib = _lib.load()
    out = np.zeros(8, np.uint64)
    assert lib.zk_babyjub_mul(None, None, out.ctypes.data_as(_lib.u64p)) == _lib.ZK_ERR_ARG
    assert lib.zk_babyjub_add(None, None, None) == _lib.ZK_ERR_ARG and lib.zk_babyjub_on_curve(None) == _lib.ZK_ERR_ARG
    b = Builder()
    x, y = b.new_wire(), b.new_wire()
    bits = b.new_bits(3)
    for call in (lambda: b.babyjub_mul_fixed([]), lambda: b.babyjub_mul_fixed([bits[0]] * 257), lambda: b.babyjub_mul([x, y], []),
                 lambda: b.babyjub_mul_fixed([bits[0], 99]), lambda: b.babyjub_mul([x, 99], bits), lambda: b.babyjub_add([x, y, 1], [x, y, 99]),
                 lambda: b.babyjub_affine([x, y, 99], [x, y]), lambda: b.babyjub_assert_on_curve([x, 99]), lambda: b.babyjub_add([x, y], [x, y, 1])):
        with pytest.raises(BuildErr) as e:
            call()
        assert e.value.status == _lib.ZK_ERR_ARG
    assert b.dims()[1] == 0                                      # a refusal emits nothing


# ---- the gadgets -----------------------------------------------------------------------------------
def test_assert_on_curve_and_affine():
    p = Pair()
    x, y = p.field(), p.field()
    p.both("babyjub_assert_on_curve", [x, y])
    assert p.lib.dims()[1] == 4
    c, f = p.finish([])
    check_rows(c, f)
    for pt in EDGE:
        check_witness(c, f, list(pt))
    for pt in ((1, 1), (bm.BASE8[0], bm.BASE8[1] + 1), (bm.BASE8[0] + 1, bm.BASE8[1])):
        w = limbs_to_ints(c.weights(list(pt)))
        assert f.failing_gates(w) == [3]                        # the library's witness for a point off the curve breaks the assertion


@pytest.mark.parametrize("q_affine", [True, False])
def test_add_gadget_over_all_pairs_of_edge_points(q_affine):
    p = Pair()
    pw = [p.field() for _ in range(3)]
    qw = [p.field(), p.field()] + ([p.lib.ONE] if q_affine else [p.field()])
    sw = p.both("babyjub_add", pw, qw)
    x, y = p.field(), p.field()
    p.both("babyjub_affine", sw, [x, y])
    assert p.lib.dims()[1] == (10 if q_affine else 11) + 4
    c, f = p.finish(sw)
    check_rows(c, f)
    rng = SplitMix64(21)
    for a, b in itertools.product(EDGE, repeat=2):
        z1, z2 = rng.fr() or 1, 1 if q_affine else rng.fr() or 1
        s = bm.add(a, b)
        row = [a[0] * z1 % R, a[1] * z1 % R, z1, b[0] * z2 % R, b[1] * z2 % R] + ([] if q_affine else [z2]) + list(s)
        w = check_witness(c, f, row)
        assert value(f, w, sw) == s == babyjub.add(a, b)
    # a supplied affine coordinate off by one in x or in y leaves an assertion unsatisfied
    a, b = bm.BASE8, bm.GENERATOR
    s = bm.add(a, b)
    base = [a[0], a[1], 1, b[0], b[1]] + ([] if q_affine else [1])
    n = c.n
    assert f.failing_gates(limbs_to_ints(c.weights(base + [(s[0] + 1) % R, s[1]]))) == [n - 3]
    assert f.failing_gates(limbs_to_ints(c.weights(base + [s[0], (s[1] + 1) % R]))) == [n - 1]


@pytest.mark.parametrize("n_bits", sorted(GATE_COUNTS_FIXED))
def test_mul_fixed_rows_counts_and_values(n_bits):
    p = Pair()
    bits = p.bits(n_bits)
    out = p.both("babyjub_mul_fixed", bits)
    assert p.lib.dims()[1] == GATE_COUNTS_FIXED[n_bits] == bm.fixed_gates(n_bits)
    x, y = p.field(), p.field()
    p.both("babyjub_affine", out, [x, y])
    c, f = p.finish([x, y])
    check_rows(c, f)
    top = (1 << n_bits) - 1
    # every window at each of its 8 values, the top bit alone, the edge scalars
    scalars = [sum(v << (3 * k) for k in range(86)) & top for v in range(8)] + [1 << (n_bits - 1)] + [k & top for k in bm.EDGE_SCALARS[:9]]
    if n_bits <= 4:
        scalars = list(range(1 << n_bits))
    for k in dict.fromkeys(scalars):
        want = bm.mul(k)
        assert babyjub.mul(k) == want
        w = check_witness(c, f, [(k >> i) & 1 for i in range(n_bits)] + list(want))
        assert value(f, w, out) == want and (w[1], w[2]) == want


@pytest.mark.parametrize("n_bits", sorted(GATE_COUNTS_VAR))
def test_mul_rows_counts_and_values(n_bits):
    p = Pair()
    px, py = p.field(), p.field()
    bits = p.bits(n_bits)
    out = p.both("babyjub_mul", [px, py], bits)
    assert p.lib.dims()[1] == GATE_COUNTS_VAR[n_bits] == bm.var_gates(n_bits)
    c, f = p.finish(outputs(out))
    check_rows(c, f)
    top = (1 << n_bits) - 1
    scalars = [sum(v << (3 * k) for k in range(86)) & top for v in range(8)] + [1 << (n_bits - 1), bm.L & top, (8 * bm.L) & top]
    if n_bits <= 4:
        scalars = list(range(1 << n_bits))
    points = [bm.GENERATOR] if n_bits > 7 else [bm.GENERATOR, bm.IDENTITY, (0, R - 1), (bm.X4, 0), bm.mul(bm.L, bm.GENERATOR), bm.neg(bm.BASE8)]
    for pt in points:
        for k in dict.fromkeys(scalars):
            w = check_witness(c, f, list(pt) + [(k >> i) & 1 for i in range(n_bits)])
            assert value(f, w, out) == bm.mul(k, pt) == babyjub.mul(k, pt)


def test_wrong_witnesses_leave_a_gate_unsatisfied():
    n_bits = 7
    p = Pair()
    px, py = p.field(), p.field()
    bits = p.bits(n_bits)
    out = p.both("babyjub_mul", [px, py], bits)
    ax, ay = p.field(), p.field()
    p.both("babyjub_affine", out, [ax, ay])
    fixed = p.both("babyjub_mul_fixed", bits)
    bx, by = p.field(), p.field()
    p.both("babyjub_affine", fixed, [bx, by])
    c, f = p.finish([ax, ay, bx, by])
    k, pt = 0b1011001, bm.GENERATOR
    good = list(pt) + [(k >> i) & 1 for i in range(n_bits)] + list(bm.mul(k, pt)) + list(bm.mul(k))
    check_witness(c, f, good)
    bad_rows = []
    for i in range(n_bits):                                     # a changed bit: the supplied results no longer fit
        bad_rows.append(good[:2 + i] + [1 - good[2 + i]] + good[3 + i:])
    for at in range(2 + n_bits, 2 + n_bits + 4):                # a supplied affine coordinate off by one, x and y, both products
        bad_rows.append(good[:at] + [(good[at] + 1) % R] + good[at + 1:])
    bad_rows.append([pt[0], (pt[1] + 1) % R] + good[2:])        # P off the curve
    for row in bad_rows:
        assert f.failing_gates(limbs_to_ints(c.weights(row))) != [], row
    # a "bit" that is no bit: the evaluators refuse the input, and the witness the gates would see breaks the bit assertion
    with pytest.raises(ParseErr):
        c.weights(good[:2] + [2] + good[3:])
    w = f.evaluate(good[:2] + [2] + good[3:])
    assert 4 in f.failing_gates(w)                              # gates 0..3 assert P on the curve, gate 4 is the first bit's assertion
