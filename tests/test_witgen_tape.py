"""circuit::weights through the compiled tape (zk_circuit_weights_tape, zk_circuit_tape_dims): host code, no GPU.  The tape must give
the words, statuses and texts of zk_circuit_weights, which stays the yardstick; every comparison is equality of 64-bit words."""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib
from zksnark_rs_amd.circuit import Circuit, ParseErr
from zksnark_rs_amd.circuits import chain_zk

import witgen_cases as wc


@pytest.mark.parametrize("prog", wc.GOLDEN)
def test_tape_matches_weights_and_oracle(orc, prog):
    code = wc.golden(prog)
    c = Circuit(code)
    rng = zk.SplitMix64(29)
    sets = [[rng.fr() for _ in range(c.n_in)] for _ in range(3)] + [[0] * c.n_in, [1] * c.n_in, [wc.R - 1] * c.n_in]
    for ins in sets:
        a = zk.ints_to_limbs(ins)
        got = c.weights_tape(a)
        assert np.array_equal(got, c.weights(a))
        assert np.array_equal(got, orc.zk_weights(code, a, c.m))


def test_tape_dims():
    d = Circuit(wc.golden("deg_15.zk")).tape_dims()
    assert (d["depth"], d["width"]) == (16, 1)
    d = Circuit(wc.golden("simple.zk")).tape_dims()
    assert (d["depth"], d["width"]) == (2, 1)
    code = wc.golden("8bit_comparator.zk")
    assert wc.assignment_shape(code) == (70, 20, 24)
    c = Circuit(code)
    d = c.tape_dims()
    assert (c.n, d["depth"], d["width"]) == (70, 20, 24)
    assert d["slots"] >= c.m and d["ops"] >= c.n and d["consts"] >= 2      # literals 250 and 1
    n = (1 << 10) + 1
    c = Circuit(chain_zk(n))
    d = c.tape_dims()
    assert (c.n, c.m, d["depth"], d["width"]) == (n, 2 * n + 2, n, 1)
    for prog in ("deg_15.zk", "8bit_comparator.zk"):
        code = wc.golden(prog)
        d = Circuit(code).tape_dims()
        assert (d["depth"], d["width"]) == wc.assignment_shape(code)[1:]


def test_chain_text_is_the_chain_circuit():
    """chain_zk(n) parses to the wires of circuits.chain_rows and the tape gives circuits.chain_weights."""
    from zksnark_rs_amd.circuits import chain_weights
    c = Circuit(chain_zk(16))
    assert (c.m, c.n, c.input, c.n_in) == (34, 16, 2, 17)
    rng = zk.SplitMix64(5)
    x, avals = rng.fr(), [rng.fr() for _ in range(16)]
    assert np.array_equal(c.weights_tape([x] + avals), chain_weights(4, x, avals))
    assert np.array_equal(c.weights([x] + avals), chain_weights(4, x, avals))


@pytest.mark.parametrize("code,text", wc.STATIC_ERRORS)
def test_static_errors_keep_status_and_text(code, text):
    c = Circuit(code)                                   # parses exactly as before
    ins = zk.ints_to_limbs([3])
    rc0, msg0, _ = wc.call_weights(c, "zk_circuit_weights", ins)
    rc1, msg1, _ = wc.call_weights(c, "zk_circuit_weights_tape", ins)
    assert (rc0, msg0) == (_lib.ZK_ERR_ARG, text)
    assert (rc1, msg1) == (rc0, msg0)
    with pytest.raises(ParseErr) as e:
        c.tape_dims()
    assert str(e.value) == text
    # the argument checks still come first, as in circuit_weights
    for kw in (dict(n_in=0), dict(m=c.m + 1)):
        assert wc.call_weights(c, "zk_circuit_weights_tape", ins, **kw)[:2] == wc.call_weights(c, "zk_circuit_weights", ins, **kw)[:2]
    big = zk.ints_to_limbs([wc.R])
    assert wc.call_weights(c, "zk_circuit_weights_tape", big)[:2] == wc.call_weights(c, "zk_circuit_weights", big)[:2]
    assert wc.call_weights(c, "zk_circuit_weights_tape", big)[0] == _lib.ZK_ERR_RANGE


def test_odd_valid_programs():
    c = Circuit(wc.UNUSED_INPUT)
    assert zk.limbs_to_ints(c.weights_tape([3, 4])) == [1, 9, 3] == zk.limbs_to_ints(c.weights([3, 4]))
    assert c.tape_dims()["slots"] == c.m + 1            # the unused input lives behind the witness
    c = Circuit(wc.NESTED)
    assert zk.limbs_to_ints(c.weights_tape([3])) == [1, 54, 18, 3] == zk.limbs_to_ints(c.weights([3]))
    assert c.tape_dims()["slots"] > c.m                 # temporaries of the nested right-hand side


def test_argument_and_range_errors_match_weights():
    c = Circuit(wc.golden("simple.zk"))
    good = zk.ints_to_limbs([3, 2, 4])
    cases = [dict(inputs=good[:2]), dict(inputs=good, m=c.m - 1), dict(inputs=zk.ints_to_limbs([3, wc.R, 4])),
             dict(inputs=zk.ints_to_limbs([3, 2, (1 << 256) - 1]))]
    want = [(_lib.ZK_ERR_ARG, "Wrong number of values supplied"), (_lib.ZK_ERR_ARG, "weights buffer size mismatch"),
            (_lib.ZK_ERR_RANGE, ">= r"), (_lib.ZK_ERR_RANGE, ">= r")]
    for kw, (rc, frag) in zip(cases, want):
        ref = wc.call_weights(c, "zk_circuit_weights", **kw)
        got = wc.call_weights(c, "zk_circuit_weights_tape", **kw)
        assert ref[0] == rc and frag in ref[1]
        assert got[:2] == ref[:2]
    # an unused input is range-checked too
    c = Circuit(wc.UNUSED_INPUT)
    bad = zk.ints_to_limbs([3, wc.R])
    assert wc.call_weights(c, "zk_circuit_weights_tape", bad)[:2] == wc.call_weights(c, "zk_circuit_weights", bad)[:2]
    assert wc.call_weights(c, "zk_circuit_weights_tape", bad)[0] == _lib.ZK_ERR_RANGE


def test_deep_nesting_and_long_literal():
    c = Circuit(wc.DEEP)
    assert c.m == 4
    d = c.tape_dims()
    assert d["slots"] > c.m and d["consts"] == 3        # 1, 2 and the wrapped literal
    for a in (0, 1, 3, wc.R - 1, zk.SplitMix64(7).fr()):
        got = c.weights_tape([a])
        assert zk.limbs_to_ints(got) == wc.deep_expected(a)
        assert np.array_equal(got, c.weights([a]))


def test_squares_program_shape():
    """the device tests' wide-then-narrow program: one level of 200 assignments, then 199 levels of one"""
    code = wc.squares_zk(200)
    c = Circuit(code)
    d = c.tape_dims()
    assert (d["depth"], d["width"]) == (200, 200) == wc.assignment_shape(code)[1:]
    ins = wc.random_inputs(3, 3, c.n_in)
    for j in range(3):
        assert np.array_equal(c.weights_tape(ins[j]), c.weights(ins[j]))
    assert zk.limbs_to_int(c.weights([2] * 200)[1]) == 800
