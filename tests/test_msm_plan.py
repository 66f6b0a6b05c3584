"""-m "not gpu": the plan of the inner products -- which window, which run length by which rule, which tail form, chained or not --
restated in Python (tests/msm_plan_model.py) and checked on the CPU:

  * the window rule equals the library's (zk_msm_auto_window is host code) around every threshold;
  * at 256 compute units the restatement gives the table of DESIGN.md section 6 for the proof sizes 2^15 .. 2^21;
  * the sizes the GPU tests run at (tests/test_gpu_size_ladder.py) together reach every run-length rule in G1 and in G2, both
    tail forms, both chaining states, every value of the automatic window and the boundaries no other test sits on;
  * a slip planted in any rule changes the plan of at least one of those sizes, so the comparison of the library's record with the
    restatement on the GPU would notice it;
  * the boundary constructions expect every counted event at least 20 times at the wanted position.

The GPU tests compare this restatement with the record the library keeps (Context.msm_plans()), product by product."""
import pytest

import msm_plan_model as M
from msm_plan_model import FILL, PLAIN, SMALL, WHOLE

CU = 256


def test_window_rule_is_the_librarys():
    from zksnark_rs_amd import _lib
    lib = _lib.load()
    edges = [1 << k for k in range(0, 25)] + [(1 << 20) - 8, (1 << 21) - 8]
    for e in edges:
        for n in range(max(e - 3, 0), e + 3):
            assert M.auto_window(n) == lib.zk_msm_auto_window(n), n
            assert M.auto_window_g2(n) == lib.zk_msm_auto_window_g2(n), n
    assert {M.auto_window(n) for n in range(0, 1 << 21, 997)} == {8, 13, 15, 16, 17, 20}


def _row(p):
    return (p["c"], p["run_branch"], p["run_len"], p["quad_tail"], p["unchained"])


def test_plan_table_at_256_compute_units():
    """the proof sizes 2^15 .. 2^21: A (= B in G2 at these sizes) and the merged product"""
    want = {15: ((15, SMALL, 8, 1, 1), (16, SMALL, 28, 1, 1)),
            16: ((16, SMALL, 16, 1, 1), (17, WHOLE, 128, 1, 1)),
            17: ((17, WHOLE, 128, 1, 1), (17, WHOLE, 256, 1, 1)),
            18: ((17, WHOLE, 128, 1, 1), (20, WHOLE, 128, 0, 0)),
            19: ((17, WHOLE, 256, 1, 1), (20, WHOLE, 128, 0, 0)),
            20: ((20, WHOLE, 128, 0, 0), (20, WHOLE, 256, 0, 0)),
            21: ((20, WHOLE, 128, 0, 0), (20, FILL, 256, 0, 0))}
    for log_n, (ab, lh) in want.items():
        n, m, l = M.chain_dims(log_n)
        a, b, merged = M.proof_plans(n, m, l, CU)
        assert (a["g2"], b["g2"], merged["g2"]) == (0, 1, 0)
        assert _row(a) == ab and _row(b) == ab and _row(merged) == lh, log_n
        assert (a["n_used"], b["n_used"], merged["n_used"]) == (n, n, 4 * n - 1)
    # merge_lh = 0: L, A, B, H -- L and H over the merged table, with its window
    n, m, l = M.chain_dims(18)
    L, a, b, h = M.proof_plans(n, m, l, CU, merge_lh=False)
    assert (L["n_used"], L["c"], h["n_used"], h["c"]) == (2 * n - 1, 20, 2 * n, 20) and a["c"] == b["c"] == 17
    # the integer roots: xi_t keeps its n - 1 points, the merged table has 4 n - 2 -- at 2^18 exactly the 2^20 - 8 clause
    assert M.table_points(n, m, l, integers=True)[2] == 4 * n - 2 == 1048574
    assert M.proof_plans(n, m, l, CU, integers=True)[2]["c"] == 20 and M.auto_window(1048574 - 7) == 17
    # a witness cut before the private wires leaves no L product to record
    assert len(M.proof_plans(n, m, l, CU, merge_lh=False, witness_len=l + 1)) == 3


def test_chosen_sizes_reach_every_branch_and_boundary():
    prods = M.chosen_products(CU)
    plans = [p for _, p in prods]
    for g2 in (0, 1):
        mine = [p for p in plans if p["g2"] == g2]
        assert {p["run_branch"] for p in mine} == {PLAIN, WHOLE, FILL, SMALL}, g2
        assert {p["quad_tail"] for p in mine} == {0, 1} and {p["unchained"] for p in mine} == {0, 1}, g2
        assert {8, 13, 15, 16, 17, 20} <= {p["c"] for p in mine}, g2
        assert {128, 256} <= {p["run_len"] for p in mine if p["run_branch"] == WHOLE}, g2
        # run_fill with 32 < T < 256 (only the band of the c = 17 window reaches it unsharded), and its cap at RUN_MAX
        fills = {p["run_len"] for p in mine if p["run_branch"] == FILL}
        assert any(32 < t < 256 for t in fills), g2
    assert 256 in {p["run_len"] for p in plans if p["run_branch"] == FILL}
    by = dict(prods)
    # 2^18: quad-tail, unchained A and B beside a one-lane, chained merged product whose table sits on the n + 8 >= 2^20 clause
    a, b, merged = (by[("ladder", 18, True, i)] for i in range(3))
    assert a["quad_tail"] == b["quad_tail"] == 1 and a["unchained"] == b["unchained"] == 1
    assert merged["quad_tail"] == 0 and merged["unchained"] == 0 and merged["c"] == 20 and M.auto_window(merged["n_used"] - 8) == 17
    # 2^17: runs cut at RUN_MAX under the four-lane tail; 2^15: c = 16 with a run length that is none of 4, 8, 16, 32
    merged = by[("ladder", 17, True, 2)]
    assert (merged["run_len"], merged["quad_tail"]) == (256, 1)
    merged = by[("ladder", 15, True, 2)]
    assert merged["c"] == 16 and merged["run_len"] not in (4, 8, 16, 32)
    # the stand-alone sizes: both sides of every change of the run-length rule in the c = 17 band and of the 2^20 - 8 clause
    for g2 in (False, True):
        sizes, (n256, nfill) = M.band_17(g2, CU)
        p = lambda n: M.msm_plan(n, g2, CU)
        assert (p(n256 - 1)["run_len"], p(n256)["run_len"]) == (128, 256)
        assert (p(nfill - 1)["run_branch"], p(nfill)["run_branch"]) == (WHOLE, FILL) and 32 < p(nfill)["run_len"] < 256
        assert (p(sizes[-2])["c"], p(sizes[-1])["c"]) == (17, 20) and sizes[-2:] == [(1 << 20) - 9, (1 << 20) - 8]
        assert p(sizes[4])["run_branch"] == FILL and nfill < sizes[4] < sizes[-2]
        assert set(sizes) <= set(M.stand_alone_sizes(CU))
    # the integer-roots proof inside the band: A and B are the only unsharded products that take run_fill below RUN_MAX
    n = M.integer_sizes(CU)[0]
    a, b = by[("integers", n, 0)], by[("integers", n, 1)]
    assert a["run_branch"] == b["run_branch"] == FILL and 32 < a["run_len"] < b["run_len"] < 256 and a["unchained"] == 0 and a["quad_tail"] == 1
    # the batches: 64 groups at c >= 10 put the level-1 counters at exactly the 64 KiB the library accepts
    for log_n, count in M.BATCHES:
        assert M.batch_fits(*M.chain_dims(log_n), count), (log_n, count)
    assert not M.batch_fits(*M.chain_dims(16), 65)
    assert by[("batch", 16, 64, 0)]["buckets"] == 64 << 15 and by[("batch", 16, 64, 0)]["n_used"] == 64 << 16
    # the boundary constructions run where they are meant to
    for kind, branch in ((128, WHOLE), (256, WHOLE), ("fill", FILL), ("plain", PLAIN)):
        for g2 in (False, True):
            T, c, n = M.boundary_setup(kind, g2, CU)
            p = by[("boundary", kind, g2, 0)]
            assert (p["run_len"], p["run_branch"], p["c"]) == (T, branch, c) and M.boundary_entries(T) <= n
            assert T == (kind if isinstance(kind, int) else T) and (kind != "fill" or 32 < T < 256) and (kind != "plain" or T == 32)


@pytest.mark.parametrize("slip", M.SLIPS)
def test_planted_slips_change_a_chosen_plan(slip):
    """each slip alters one comparison or constant of the restated rules; at least one product of the chosen sizes must come out
    with another plan -- the GPU tests compare every one of them with the library's record"""
    good, bad = M.chosen_products(CU), M.chosen_products(CU, slip=slip)
    assert [k for k, _ in good] == [k for k, _ in bad]
    changed = [k for (k, p), (_, q) in zip(good, bad) if p != q]
    assert changed, slip


def test_run_bounds_restates_the_cut():
    for T in (4, 32, 44, 64, 128, 256):
        assert M.run_bounds(T - 1, T) == [(0, T - 1)] and M.run_bounds(T, T) == [(0, T)]
        assert M.run_bounds(T + 1, T) == [(0, (T + 1) // 2), ((T + 1) // 2, T + 1)]
        assert M.run_bounds(2 * T, T) == [(0, T), (T, 2 * T)] and len(M.run_bounds(2 * T + 1, T)) == 3
        for z in range(1, 5 * T):
            b = M.run_bounds(z, T)
            assert b[0][0] == 0 and b[-1][1] == z and all(x[1] == y[0] for x, y in zip(b, b[1:]))
            assert all(0 < hi - lo <= T for lo, hi in b) and max(hi - lo for lo, hi in b) - min(hi - lo for lo, hi in b) <= 1


def test_boundary_constructions_expect_every_event_20_times():
    for kind in M.BOUNDARY_KINDS:
        for g2 in (False, True):
            T = M.boundary_setup(kind, g2, CU)[0]
            exp = M.boundary_expectations(T)
            assert len(exp) == 11 and min(exp.values()) >= M.EXPECT, (kind, g2, exp)
            # a bucket of T + 1 entries: a first run of even and a second of odd length, which no bucket of T entries has
            (a0, a1), (b0, b1) = M.run_bounds(T + 1, T)
            assert (a1 - a0) % 2 == 0 and (b1 - b0) % 2 == 1 and T % 2 == 0
            assert M.copies_multiplier("copies last-", T) == -(a1 - 1) == -M.copies_multiplier("copies last+", T)
            assert M.copies_multiplier("copies head-", T) == -(b1 - b0 - 1)
            sizes = {z for name, z, _, _ in M.boundary_classes(T) if name == "plain"}
            assert sizes == {T - 1, T, T + 1, 2 * T, 2 * T + 1}


def test_record_layout_matches_the_restatement():
    """the binding, the library's field names, the header's rule names and the restatement's dictionary agree"""
    import os
    import re
    import zksnark_rs_amd as zk
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert zk.Context.MSM_PLAN_FIELDS == M.PLAN_FIELDS == tuple(M.plan(1, False, 8, CU))
    header = open(os.path.join(root, "include", "zkgpu_measure.h")).read()
    names = dict(re.findall(r"ZK_MSM_RUN_(\w+) = (\d)", header))
    assert {k: int(v) for k, v in names.items()} == {"PLAIN": PLAIN, "WHOLE": WHOLE, "FILL": FILL, "SMALL": SMALL}
    capi = open(os.path.join(root, "zksnark_rs_amd", "csrc", "capi.hip")).read()
    body = capi[capi.index("static long msm_plan_value"):capi.index("long zk_get_option")]
    assert tuple(re.findall(r'strcmp\(f, "(\w+)"\)', body)) == M.PLAN_FIELDS
    for f in M.PLAN_FIELDS:
        assert re.search(r"\* +%s +" % f, header), f
