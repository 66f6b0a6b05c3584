"""-m "not gpu": Poseidon on the host (csrc/poseidon.hpp, zk_poseidon_hash / zk_poseidon_params) and the builder's gadgets
(zk_builder_poseidon, zk_builder_merkle_root) against tests/poseidon_model.py and the published circomlib values: constants, digests,
refusals, gate counts, rows, the three host evaluators, and the split of a membership circuit."""
import itertools

import numpy as np
import pytest

from zksnark_rs_amd import SplitMix64, ZkError, _lib, limbs_to_ints
from zksnark_rs_amd import poseidon
from zksnark_rs_amd.circuit import Builder, BuildErr

import poseidon_model as pm
from gadget_cases import Pair

R = pm.R

# circomlib's published values (poseidon_constants.json, the circomlibjs test vectors) and what follows from them
KAT_C = {3: 0x0ee9a592ba9a9518d05986d656f40c2114c4993c11bb29938d21d47304cd8e6e, 2: 0x09c46e9ec68e9bd4fe1faaba294cba38a71aa177534cdd1b6c7dc0dbd0abd7a7}
KAT_M3 = 0x109b7f411ba0e4c9b2b70caf5c36a7b194be7c11ad24378bfedb68592ba8118b
Z1 = 0x2098f5fb9e239eab3ceac3f27b81e481dc3124d55ffed523a839ee8446b64864
Z2 = 0x1069673dcdb12263df301a6ff584a7ec261a44cb9dc68df067a4774460b1f1e1
KAT_HASH = [
    ((1,), 0x29176100eaa962bdc1fe6c654d6a3c130e96a4d1168b33848b897dc502820133),
    ((1, 2), 0x115cc0f5e7d690413df64c6b9662e9cf2a3617f2743245519e19607a4417189a),
    ((3, 4), 0x20a3af0435914ccd84b806164531b0cd36e37d4efb93efab76913a93e1f30996),
    ((0, 0), Z1),
    ((Z1, Z1), Z2),
    ((1, 2, 3, 4), 0x299c867db6c1fdd79dcefa40e4510b9837e60ebb1ce0663dbaa525df65250465),
    ((R - 1, R - 1), 0x2c6bd813a6338781378d8706cb82fd4216ab52b752ccd41564d7b98756a6e0fb),
]
KAT_ROOT = {2: 0x0d9e989a60f1961e8fda683cfc3585608a47d513f9af9167c1287fa8cea0720e, 3: 0x05c1e52b41a571293b30efacd2afdb7173b20cfaf1f646c4ac9f96eb75848270}
GATES = {1: 217, 2: 244, 4: 301}


# ---- the function ----------------------------------------------------------------------------------
def test_known_answers_model_and_library():
    for source in (lambda a: pm.params(a + 1), lambda a: (poseidon.params(a)["c"], poseidon.params(a)["m"])):
        assert source(2)[0][0] == KAT_C[3] and source(2)[1][0][0] == KAT_M3 and source(1)[0][0] == KAT_C[2]
    for inputs, want in KAT_HASH:
        assert pm.hash(list(inputs)) == want, inputs
        assert poseidon.hash(inputs) == want, inputs
    assert pm.zero_hashes(2) == [0, Z1, Z2] and poseidon.zero_hashes(2) == [0, Z1, Z2]
    for depth, want in KAT_ROOT.items():
        assert pm.tree_root(pm.tree_levels([1, 2, 3], depth), depth) == want


def test_the_two_grain_generators_agree():
    for t in (2, 3, 5):
        assert pm.params(t, pm.grain_bits) == pm.params(t, pm.grain_int)


@pytest.mark.parametrize("arity", [1, 2, 4])
def test_all_constants_library_against_model(arity):
    p = poseidon.params(arity)
    c, m = pm.params(arity + 1)
    assert (p["t"], p["rf"], p["rp"]) == (arity + 1, 8, pm.R_P[arity + 1])
    assert len(p["c"]) == (8 + p["rp"]) * (arity + 1) and p["c"] == c
    assert p["m"] == m
    assert all(x < R for x in p["c"]) and all(x < R for row in p["m"] for x in row)
    xs = set()                                              # a Cauchy matrix: every 2 x 2 minor of 1 / M is that of x_i + y_j
    inv = [[pow(x, R - 2, R) for x in row] for row in p["m"]]
    for i, j in itertools.product(range(arity), repeat=2):
        xs.add((inv[i][j] + inv[i + 1][j + 1] - inv[i][j + 1] - inv[i + 1][j]) % R)
    assert xs == {0}


@pytest.mark.parametrize("arity", [1, 2, 4])
def test_hash_on_edge_and_drawn_inputs(arity):
    rng = SplitMix64(500 + arity)
    rows = [[0] * arity, [1] * arity, [R - 1] * arity, [0] * (arity - 1) + [R - 1], [R - 1] + [0] * (arity - 1)]
    rows += [[rng.fr() for _ in range(arity)] for _ in range(12)]
    for row in rows:
        assert poseidon.hash(row) == pm.hash(row), row


def test_refusals():
    for arity in (0, 3, 5):
        with pytest.raises(ZkError) as e:
            poseidon.hash([1] * arity)
        assert e.value.status == _lib.ZK_ERR_ARG
        with pytest.raises(ZkError) as e:
            poseidon.params(arity)
        assert e.value.status == _lib.ZK_ERR_ARG
        b = Builder()
        with pytest.raises(BuildErr) as e:
            b.poseidon([b.new_wire() for _ in range(arity)])
        assert e.value.status == _lib.ZK_ERR_ARG and "arity" in str(e.value)
    for row in ([R], [1, R], [R, 1], [1, 2, 3, R], [(1 << 256) - 1, 0]):
        with pytest.raises(ZkError) as e:
            poseidon.hash(row)
        assert e.value.status == _lib.ZK_ERR_RANGE
    b = Builder()
    with pytest.raises(BuildErr) as e:
        b.poseidon([b.new_wire(), 99])
    assert e.value.status == _lib.ZK_ERR_ARG and "unknown wire" in str(e.value)
    with pytest.raises(BuildErr):
        b.merkle_root(b.new_wire(), [99], [b.new_bit()])
    with pytest.raises(BuildErr):
        b.merkle_root(b.new_wire(), [b.new_wire()], [])


# ---- the gadgets -----------------------------------------------------------------------------------
def check_against_model(c, f, input_rows):
    """rows word for word; per input row the three host evaluators agree with the model's witness and every gate holds"""
    assert (c.m, c.n, c.input, c.n_in) == (f.m, f.n, f.input, f.n_in)
    for which in range(3):
        ptr, gate, val = c.rows(which)
        mptr, mgate, mval = f.csr(which)
        assert [int(x) for x in ptr] == mptr and [int(x) for x in gate] == mgate and limbs_to_ints(val) == mval, which
    out = []
    for row in input_rows:
        want = f.evaluate(row)
        assert f.failing_gates(want) == []
        w = c.weights(row)
        assert limbs_to_ints(w) == want
        assert np.array_equal(c.weights_tape(row), w)
        kinds = [k for k in f.kinds if k in ("bit", "field")]
        bits = [x for x, k in zip(row, kinds) if k == "bit"]
        packed = bytes(sum(b << i for i, b in enumerate(bits[8 * k:8 * k + 8])) for k in range((len(bits) + 7) // 8))
        assert np.array_equal(c.weights_mixed(packed, [x for x, k in zip(row, kinds) if k == "field"]), w)
        out.append(want)
    return out


def finish(pair, verify):
    c, f = pair.finish(verify)
    f.kinds = list(pair.model.kind)
    return c, f


@pytest.mark.parametrize("arity", [1, 2, 4])
def test_poseidon_gadget(arity):
    p = Pair()
    ins = [p.field() for _ in range(arity)]
    out = p.both("poseidon", ins)
    assert p.lib.dims()[1] == GATES[arity] == pm.gate_count(arity)
    c, f = finish(p, [out])
    assert not c.boolean
    rng = SplitMix64(40 + arity)
    rows = [[0] * arity, [R - 1] * arity, list(range(1, arity + 1))] + [[rng.fr() for _ in range(arity)] for _ in range(3)]
    for row, w in zip(rows, check_against_model(c, f, rows)):
        assert w[f.wit[out]] == pm.hash(row) == w[1]
    widest = max(len(l) for l, _, _ in f.subs)
    assert widest <= (arity + 1) + pm.R_P[arity + 1] + 1


def test_poseidon_gadget_on_constants_a_repeated_wire_and_a_bit_wire():
    p = Pair()
    x = p.field()
    bit = p.bits(1)[0]
    outs = [p.both("poseidon", [p.lib.ONE, p.lib.ZERO]), p.both("poseidon", [x, x]), p.both("poseidon", [bit, x]),
            p.both("poseidon", [p.lib.ZERO]), p.both("poseidon", [x, bit, p.lib.ONE, x])]
    assert p.lib.dims()[1] == 3 * 244 + 217 + 301
    c, f = finish(p, outs)
    rng = SplitMix64(46)
    rows = [[0, 0], [R - 1, 1], [rng.fr(), 1], [rng.fr(), 0]]
    for (xv, bv), w in zip(rows, check_against_model(c, f, rows)):
        assert w[1:6] == [pm.hash([1, 0]), pm.hash([xv, xv]), pm.hash([bv, xv]), pm.hash([0]), pm.hash([xv, bv, 1, xv])]
    d = c.mixed_dims()
    assert (d["n_bit_inputs"], d["n_field_inputs"], d["core_ops"]) == (1, 1, 0)


def test_a_digest_feeds_another_hash_and_a_gate():
    p = Pair()
    a, b = p.field(), p.field()
    h1 = p.both("poseidon", [a, b])
    h2 = p.both("poseidon", [h1, a])
    c, f = finish(p, [h2])
    rows = [[5, 6], [R - 1, 0]]
    for (av, bv), w in zip(rows, check_against_model(c, f, rows)):
        assert w[1] == pm.hash([pm.hash([av, bv]), av])


def membership(depth, p=None):
    p = p or Pair()
    leaf = p.field()
    sibs = [p.field() for _ in range(depth)]
    dirs = p.bits(depth)
    root = p.both("merkle_root", leaf, sibs, dirs)
    return p, leaf, root


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_merkle_root_over_every_direction_pattern(depth):
    p, leaf, root = membership(depth)
    assert p.lib.dims()[1] == 246 * depth
    if depth == 0:
        assert root == leaf
        return
    c, f = finish(p, [root])
    rng = SplitMix64(60 + depth)
    leaves = [rng.fr() for _ in range(5 if depth == 3 else 1 << depth)]
    levels = pm.tree_levels(leaves, depth)
    rows, roots = [], []
    for pattern in range(1 << depth):                       # every direction pattern, over drawn siblings
        sibs = [rng.fr() for _ in range(depth)]
        dirs = [(pattern >> k) & 1 for k in range(depth)]
        value = rng.fr()
        rows.append([value] + sibs + dirs)
        roots.append(pm.fold(value, sibs, dirs))
    for index in range(len(leaves)):                        # and the real paths of a tree
        value, sibs, dirs = pm.path(levels, depth, index)
        rows.append([value] + sibs + dirs)
        roots.append(pm.tree_root(levels, depth))
    for want, w in zip(roots, check_against_model(c, f, rows)):
        assert w[1] == want


def test_a_direction_that_is_no_bit_breaks_its_assertion():
    p, leaf, root = membership(1)
    c, f = finish(p, [root])
    w = f.evaluate([7, 9, 0])
    assert f.failing_gates(w) == []
    w[f.wit[4]] = 2                                         # the direction wire: wires 2, 3, 4 = leaf, sibling, direction
    assert 0 in f.failing_gates(w)


def test_mixed_dims_of_a_depth_3_membership_circuit():
    p, leaf, root = membership(3)
    c, f = finish(p, [root])
    d = c.mixed_dims()
    assert (c.n, c.input, c.n_in) == (738, 1, 7)
    assert (d["n_bit_inputs"], d["n_field_inputs"], d["core_ops"], d["core_levels"]) == (3, 4, 0, 0)
    assert d["tail_ops"] > 3 * 244 and d["tail_slots"] >= 4 + 3 * 245
    assert not c.boolean
