"""-m "not gpu": the shared cases of tests/gadget_cases.py on the host, before tests/test_gpu_gadgets.py takes them to the device.  Per
case: the three row sets word for word against the model, the three host evaluators (weights, weights_tape, weights_mixed) against
the model's witness on a spread of instances that always holds the edge ones, the gates that fail (none on the curve, gate 3 off
it), and the shape of the tape and of the split the device tests rely on.  Run with -s to see every circuit's dimensions."""
import pytest

import babyjub_model as bm
import gadget_cases as gc
from gadget_cases import check_rows, check_witness

CASES = gc.all_cases()
VARIABLE_BASE = [name for name in CASES if name.startswith("mul_var_") or name.startswith("statement_")]


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_host_evaluators_against_the_model(name):
    case = CASES[name]()
    check_rows(case.c, case.f)
    picked = case.spread()
    assert len(picked) <= gc.SPREAD and set(case.edge) <= set(picked)
    for j in picked:
        check_witness(case.c, case.f, case.rows[j], want=case.want(j), failing=case.failing[j])


def test_the_on_curve_case_alternates_within_every_wave():
    case = gc.on_curve_case()
    assert len(case.rows) == 130 and sorted(tuple(r) for r in case.rows[0:2 * len(gc.EDGE):2]) == sorted(gc.EDGE)
    for j, row in enumerate(case.rows):
        assert bm.on_curve(tuple(row)) == (j % 2 == 0) and case.failing[j] == ([] if j % 2 == 0 else [3])
    picked = case.spread()
    assert any(j % 2 for j in picked) and any(j % 2 == 0 for j in picked)
    assert {tuple(r) for r in case.rows[1::2]} == set(gc.OFF_CURVE)


def test_instance_counts_and_gate_counts():
    assert len(gc.add_case(True).rows) == len(gc.add_case(False).rows) == len(gc.EDGE) ** 2 == 256
    v = gc.mul_var_case(7)
    assert len(v.rows) == 896 and v.c.n == 127 + 4
    assert [len(gc.mul_fixed_case(n).rows) for n in (1, 2, 3, 4, 7)] == [2, 4, 8, 16, 128]
    for arity in (1, 2, 4):
        rows = gc.poseidon_case(arity).rows
        r1 = gc.R - 1
        assert len(rows) == 130 and rows[0] == [0] * arity and rows[1] == [r1] * arity and rows[2] == ([r1, 0] * 2)[:arity]
    for (n_s, n_h), (gates, n_in) in gc.STATEMENT_SIZES.items():
        s = gc.statement_case(n_s, n_h)
        assert (s.c.n, s.c.n_in, s.c.input, len(s.rows)) == (gates, n_in, 2, 65)


@pytest.mark.parametrize("sizes", list(gc.STATEMENT_SIZES))
def test_statement_rows_of_low_order_keys_and_edge_scalars(sizes):
    """the model alone: the statement holds for a key of order 2, 4 and 8, for S = 0 under h = 2^n - 1 and for h = 0; the 251-bit
    circuit is where test_babyjub.py's variable-base test keeps Generator only"""
    n_s, n_h = sizes
    case = gc.statement_case(n_s, n_h)
    top_s, top_h = (1 << n_s) - 1, (1 << n_h) - 1
    seen = {}
    for lane in case.edge:
        s, h, a = case.info["scalars"][lane]
        seen[a] = (s, h)
        w = case.want(lane)
        assert case.f.failing_gates(w) == [], lane
        # public wires 1 and 2 are the digests; the supplied O is [S] Base8 and R + [h] A
        row = case.rows[lane]
        assert (row[5], row[6]) == bm.pmul(s) == bm.add((row[2], row[3]), bm.pmul(h, a))
    assert seen[gc.ORDER_2] == (0, top_h) and seen[gc.ORDER_4] == (top_s, 0) and gc.ORDER_8 in seen
    assert {s for s, _, _ in case.info["scalars"]} >= {0, 1, (bm.L - 1) & top_s, bm.L & top_s, top_s}
    assert {h for _, h, _ in case.info["scalars"]} >= {0, 1, top_h, (bm.L - 1) & top_h}
    assert set(seen) == {bm.IDENTITY, gc.ORDER_2, gc.ORDER_4, gc.ORDER_8, bm.BASE8, bm.neg(bm.BASE8)}
    assert [bm.mul(k, gc.ORDER_8) == bm.IDENTITY for k in (4, 8)] == [False, True]
    assert case.edge[:1] == [0] and {63, 64} <= set(case.edge)


def test_a_changed_bit_of_the_statement_breaks_the_first_affine_assertion():
    case = gc.statement_case(7, 7)
    lane = 64
    row = list(case.rows[lane])
    row[gc.STATEMENT_FIELDS + 2] ^= 1                       # bit 2 of S, with O left alone
    assert case.f.failing_gates(case.f.evaluate(row))[0] == case.info["affine_x"]
    check_witness(case.c, case.f, row, failing=case.f.failing_gates(case.f.evaluate(row)))


# ---- the shapes the device tests rely on ----------------------------------------------------------------------------------
DEEP = ("mul_var_3", "mul_var_7", "statement_7_7", "statement_251_251")


@pytest.mark.parametrize("name", list(CASES))
def test_tape_and_split_dimensions(name):
    """What the kernels make of each circuit.  The witness kernels give a group W waves, W = the mean number of operations a level
    rounded up to a power of two, at most 4 and at most the widest level (witgen_waves): one wave, which runs the tape in program
    order and hands results on in registers, needs a tape with one operation a level."""
    case = CASES[name]()
    t, d = case.c.tape_dims(), case.c.mixed_dims()
    mean = -(-d["tail_ops"] // d["tail_levels"])
    print("\n%-18s n %5d m %5d | tape ops %5d slots %5d depth %5d width %4d | bits %3d fields %d core ops %4d levels %3d tail ops %5d levels %5d slots %5d"
          " mean ops a level %2d" % (name, case.c.n, case.c.m, t["ops"], t["slots"], t["depth"], t["width"], d["n_bit_inputs"], d["n_field_inputs"],
                                     d["core_ops"], d["core_levels"], d["tail_ops"], d["tail_levels"], d["tail_slots"], mean))
    n_bit = sum(k == "bit" for k in case.kinds)
    assert (d["n_bit_inputs"], d["n_field_inputs"]) == (n_bit, len(case.kinds) - n_bit)
    assert d["tail_ops"] > 0 and d["tail_slots"] > 0        # every case has field arithmetic: Mixgen runs k_mix_tail on all of them
    # no gadget emits a boolean gate with an output (a bit assertion computes nothing), so the core has no operation: the whole
    # circuit is the tail, whose operations are the whole-circuit tape's, and the bit inputs reach it through the bit-sliced state
    assert (d["core_ops"], d["core_levels"]) == (0, 0) and d["tail_ops"] == t["ops"]
    if name.startswith("mul_var_") or name.startswith("statement_"):
        assert n_bit > 0 and d["tail_levels"] > 2 * n_bit   # bit wires multiply field forms level after level of the tail
    if name in DEEP:
        assert t["depth"] > t["width"]                      # deeper than wide; at 1 and 2 bits the variable base is not
    if name == "chain":
        assert d["tail_ops"] == d["tail_levels"] == 4 * gc.CHAIN_LINKS and t["width"] == 1   # one operation a level: W = 1
    else:
        assert mean > 1                                     # more than one wave, a barrier a level, every operand from memory
