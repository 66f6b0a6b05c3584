"""zk_qap_check / zk_qap_check_dev (csrc/qap_check.hip): does a witness satisfy the QAP, and which gate fails first?

Every expected result comes from Python integers over the rows by gate: per gate sum(a * vals[x] for x, a in row if x < a_len) % R
for u, v and w, then su * sv % R != sw.  bad_gates, first_bad and flags are compared exactly; nothing under test computes its own
expectation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib, groth16, ints_to_limbs, limbs_to_ints, R_MODULUS as R
from zksnark_rs_amd.circuit import Circuit, Witgen
from zksnark_rs_amd.circuits import chain_rows, chain_weights, chain_zk

from test_circuit_shapes import shaped_circuit, default_m, HALF
from test_qap_check_host import build_qap_check_api

pytestmark = pytest.mark.gpu

NONE, WIRE0 = _lib.QAP_CHECK_NONE, _lib.QAP_CHECK_WIRE0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 40
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


# ---- the Python side ------------------------------------------------------------------------------------------------------------
def by_gate(rows, n):
    """(ptr, gate, val) by wire -> [[(wire, value)] per gate]"""
    ptr, gate, val = rows
    vv = limbs_to_ints(val) if len(gate) else []
    out = [[] for _ in range(n)]
    for x in range(len(ptr) - 1):
        for e in range(int(ptr[x]), int(ptr[x + 1])):
            out[int(gate[e])].append((x, vv[e]))
    return out


class Case:
    """a circuit as rows by wire (what is uploaded) and by gate (what Python sums), and a satisfying witness as ints"""

    def __init__(self, n, m, l, u, v, w, values):
        self.n, self.m, self.l, self.u, self.v, self.w, self.values = n, m, l, u, v, w, list(values)
        self.gu, self.gv, self.gw = by_gate(u, n), by_gate(v, n), by_gate(w, n)

    def bad_set(self, vals, a_len=None):
        a_len = len(vals) if a_len is None else a_len
        a_len = min(a_len, self.m)
        bad = []
        for g in range(self.n):
            su = sum(a * vals[x] for x, a in self.gu[g] if x < a_len) % R
            sv = sum(a * vals[x] for x, a in self.gv[g] if x < a_len) % R
            sw = sum(a * vals[x] for x, a in self.gw[g] if x < a_len) % R
            if su * sv % R != sw:
                bad.append(g)
        return bad

    def expect(self, vals, a_len=None):
        a_len = len(vals) if a_len is None else a_len
        bad = self.bad_set(vals, a_len)
        return len(bad), (bad[0] if bad else NONE), (0 if a_len and vals[0] == 1 else WIRE0)

    def upload(self, ctx, form, seed=1):
        if form == "unity":
            assert self.n & (self.n - 1) == 0
            return ctx.qap_sparse(self.n.bit_length() - 1, self.m, self.l, self.u, self.v, self.w)
        if form == "integers":
            return ctx.qap_sparse_integers(self.n, self.m, self.l, self.u, self.v, self.w)
        rng = zk.SplitMix64(seed)
        roots = set()
        while len(roots) < self.n:
            roots.add(rng.fr())
        return ctx.qap_sparse_roots(ints_to_limbs(sorted(roots)), self.m, self.l, self.u, self.v, self.w)


def got(ctx, qap, vals):
    """zk_qap_check through the raw result record: (bad_gates, first_bad, flags)"""
    w = np.ascontiguousarray(ints_to_limbs(list(vals)).reshape(-1, 4)) if len(vals) else np.zeros((0, 4), np.uint64)
    out = _lib.QapCheckResult(99, 99, 99)
    rc = ctx.lib.zk_qap_check(ctx.ptr, qap.ptr, w.ctypes.data_as(_lib.u64p) if len(vals) else None, len(vals), C.byref(out))
    assert rc == 0, ctx.lib.zk_last_error(ctx.ptr)
    return out.bad_gates, out.first_bad, out.flags


def _rows(entries, m):
    """[(wire, gate, value)] -> rows by wire; entries of one wire keep their order (duplicates stay)"""
    wires = np.array([e[0] for e in entries], np.int64)
    order = np.argsort(wires, kind="stable")
    ptr = np.zeros(m + 1, np.uint64)
    if len(entries):
        np.add.at(ptr, wires + 1, 1)
    ptr = np.cumsum(ptr).astype(np.uint64)
    gate = np.array([entries[i][1] for i in order], np.uint32)
    val = ints_to_limbs([entries[i][2] for i in order]).reshape(-1, 4)
    return ptr, gate, val


def chain_case(log_n, seed=3):
    n = 1 << log_n
    m, l, u, v, w = chain_rows(log_n)
    rng = zk.SplitMix64(seed)
    vals = limbs_to_ints(chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)]))
    return Case(n, m, l, u, v, w, vals)


def small_case(n, seed, one=1):
    """n gates of a few entries: wires 0 | public 1, 2 | private inputs p_g = 3 + g | outputs o_g = 3 + n + g.  Gate g:
    (c p_g + c pub) (c pub + c * 1 [+ c o_h, h < g]) = o_g, solved gate by gate with the constant wire set to `one`."""
    rng = zk.SplitMix64(seed)
    l, m = 2, 3 + 2 * n
    coef = lambda: (R - 1, HALF, rng.fr())[rng.next() % 3]
    vals = [0] * m
    vals[0] = one
    for x in range(1, 3 + n):
        vals[x] = rng.fr()
    ue, ve, we = [], [], []
    for g in range(n):
        gu = [(3 + g, coef()), (1 + g % 2, coef())]
        gv = [(1 + rng.next() % 2, coef()), (0, coef())]   # p_g is read by U of gate g alone
        if g and rng.next() % 2:
            gv.append((3 + n + rng.next() % g, coef()))
        su = sum(a * vals[x] for x, a in gu) % R
        sv = sum(a * vals[x] for x, a in gv) % R
        vals[3 + n + g] = su * sv % R
        ue += [(x, g, a) for x, a in gu]
        ve += [(x, g, a) for x, a in gv]
        we.append((3 + n + g, g, 1))
    return Case(n, m, l, _rows(ue, m), _rows(ve, m), _rows(we, m), vals)


@pytest.fixture(scope="module")
def store():
    """cases and uploaded QAPs, built once and shared (never modified)"""
    cases, qaps = {}, {}

    class Store:
        def case(self, name):
            if name not in cases:
                kind, arg = name.split(":")
                if kind == "chain":
                    cases[name] = chain_case(int(arg))
                elif kind == "small":
                    cases[name] = small_case(int(arg), 100 + int(arg))
                elif kind == "shaped":
                    n = 1 << int(arg)
                    c = shaped_circuit(n, default_m(n, L), L, 11 + int(arg))
                    cases[name] = Case(n, c["m"], L, c["u"], c["v"], c["w"], c["values"])
                    cases[name].shaped = c
            return cases[name]

        def qap(self, ctx, name, form):
            if (name, form) not in qaps:
                qaps[(name, form)] = self.case(name).upload(ctx, form)
            return qaps[(name, form)]
    return Store()


# ---- 1. satisfying witnesses, every sparse form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["unity", "integers", "roots"])
@pytest.mark.parametrize("name", ["chain:4", "chain:10", "shaped:10"])
def test_satisfying_witness_every_form(ctx, store, name, form):
    c = store.case(name)
    assert c.expect(c.values) == (0, NONE, 0)
    assert got(ctx, store.qap(ctx, name, form), c.values) == (0, NONE, 0)
    assert ctx.qap_check(store.qap(ctx, name, form), ints_to_limbs(c.values)) == (0, None, True)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_satisfying_witness_lane_and_block_edges(ctx, store, n):
    c = store.case("small:%d" % n)
    assert c.expect(c.values) == (0, NONE, 0)
    assert got(ctx, store.qap(ctx, "small:%d" % n, "integers"), c.values) == (0, NONE, 0)


# ---- 2. one wire off by one -----------------------------------------------------------------------------------------------------
def _off_by_one(ctx, qap, c, wires):
    seen = set()
    for x in wires:
        vals = list(c.values)
        vals[x] = (vals[x] + 1) % R
        want = c.expect(vals)
        assert want[0] >= 1, x                         # the change is visible to Python
        assert got(ctx, qap, vals) == want, (x, want)
        seen.add(want[1])
    return seen


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_one_wire_off_by_one_small(ctx, store, n):
    c = store.case("small:%d" % n)
    qap = store.qap(ctx, "small:%d" % n, "integers")
    gates = [g for g in (0, n - 1, 63, 64, 65) if g < n]
    wires = [3 + g for g in gates]                     # p_g: read by U of gate g
    wires += [1, 3 + n + (n - 1)]                      # a public input; the last output, which only W reads
    firsts = _off_by_one(ctx, qap, c, wires)
    assert set(gates) <= firsts                         # each of those gates is named as the first failing one by some change


def test_one_wire_off_by_one_chain(ctx, store):
    c = store.case("chain:10")
    n = c.n
    # chain wires: a_k = 2k + 2 is read by V of gate k - 1 only (k < n), a_n = 2n + 1 by gate n - 1; x = 1 by every gate but the
    # last; y = 2 by W of the last gate only
    wires = [4, 2 * n + 1, 2 * 64 + 2, 2 * 65 + 2, 2 * 66 + 2, 1, 2]
    for form in ("unity", "integers"):
        firsts = _off_by_one(ctx, store.qap(ctx, "chain:10", form), c, wires)
        assert {0, 63, 64, 65, n - 1} <= firsts


@pytest.mark.parametrize("n", [65, 1000])
def test_constant_wire_two_every_gate_holds(ctx, n):
    """the witness solved gate by gate with wire 0 = 2: every gate holds, zk_verify would still reject -- only the flag says so"""
    c = small_case(n, 7 + n, one=2)
    assert c.bad_set(c.values) == [] and c.values[0] == 2
    assert got(ctx, c.upload(ctx, "integers"), c.values) == (0, NONE, WIRE0)


# ---- 3. many failing gates and the lazy sums at their bounds ---------------------------------------------------------------------
def test_many_failing_gates_and_lazy_sum_bounds(ctx, store):
    c = store.case("shaped:10")
    m = c.m
    rng = np.random.default_rng(5)
    uniform = [x % R for x in limbs_to_ints(rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64))]
    most = 0
    for form in ("unity", "integers"):
        qap = store.qap(ctx, "shaped:10", form)
        for name, vals in (("r-1", [R - 1] * m), ("half", [HALF] * m), ("uniform", uniform)):
            want = c.expect(vals)
            most = max(most, want[0])
            assert got(ctx, qap, vals) == want, (form, name, want)
        assert c.expect([0] * m) == (0, NONE, WIRE0)
        assert got(ctx, qap, [0] * m) == (0, NONE, WIRE0)
        # witnesses cut so that the 1000-entry row keeps 63 .. 129 entries (as test_spmv_wide_rows builds them)
        g = [g for g, w in c.shaped["wide"].items() if w == 1000][0]
        wires = sorted(x for x, _ in c.shaped["gate_u"][g])
        assert len(set(wires)) == len(wires)
        for keep in (63, 64, 65, 127, 128, 129):
            a_len = wires[keep - 1] + 1
            assert sum(1 for x, _ in c.gu[g] if x < a_len) == keep
            for vals in (uniform, [R - 1] * m, c.values):
                want = c.expect(vals[:a_len])
                most = max(most, want[0])
                assert got(ctx, qap, vals[:a_len]) == want, (form, keep, want)
    assert most >= 300                                  # the count crosses waves and blocks


# ---- 4. W rows the existing circuits never have ---------------------------------------------------------------------------------
def odd_w_case():
    """200 gates over 300 wires: wires 0 | public 1, 2 | inputs 3..99 | outputs o_j = 100 + j.  W rows of 0, 1, 2 and 70 entries, a
    duplicated (wire, gate) pair, coefficients r - 1 and HALF, gates with an empty U row (they hold exactly when W_j = 0)."""
    rng = zk.SplitMix64(44)
    n, m, l = 200, 300, 2
    special = (R - 1, HALF)
    coef = lambda: special[rng.next() % 2] if rng.next() % 3 == 0 else rng.fr()
    inp = lambda: 1 + rng.next() % 99
    vals = [0] * m
    vals[0] = 1
    for x in range(1, m):
        vals[x] = rng.fr()                              # outputs of gates with an empty W row keep these
    ue, ve, we = [], [], []
    kinds = {}
    for j in range(n):
        o = 100 + j
        gu = [] if j % 10 == 3 else [(inp(), coef()), (0, coef())]
        gv = [] if j == 7 else [(inp(), coef())] + ([(100 + rng.next() % j, coef())] if j % 3 == 1 else [])
        if j % 20 == 3 or j == 7:
            gw = []                                     # 0 entries: 0 * V = 0 (empty U), U * 0 = 0 (gate 7: empty V)
        elif j == 50:
            gw = [(o, R - 1)] + [(inp() if k % 2 else 100 + rng.next() % j, special[k % 2] if k % 5 == 0 else rng.fr()) for k in range(69)]
        elif j == 60:
            gw = [(o, HALF), (5, coef()), (o, R - 1)]   # a duplicated (wire, gate) pair: the entries add up
        elif j % 2:
            gw = [(o, coef()), (inp(), coef())]         # 2 entries
        else:
            gw = [(o, coef())]                          # 1 entry
        kinds[j] = len(gw)
        if gw:                                          # solve o's value: c_o a_o + rest = U V
            c_o = sum(a for x, a in gw if x == o) % R
            rest = sum(a * vals[x] for x, a in gw if x != o) % R
            su = sum(a * vals[x] for x, a in gu) % R
            sv = sum(a * vals[x] for x, a in gv) % R
            vals[o] = (su * sv - rest) * pow(c_o, -1, R) % R
        ue += [(x, j, a) for x, a in gu]
        ve += [(x, j, a) for x, a in gv]
        we += [(x, j, a) for x, a in gw]
    assert {0, 1, 2, 3, 70} <= set(kinds.values())
    return Case(n, m, l, _rows(ue, m), _rows(ve, m), _rows(we, m), vals)


def test_w_rows_of_every_length(ctx):
    c = odd_w_case()
    assert c.expect(c.values) == (0, NONE, 0)
    assert sum(1 for g in range(c.n) if not c.gu[g] and c.gw[g]) >= 5       # empty U, W_j = 0 from a non-empty row
    for form in ("integers", "roots"):
        qap = c.upload(ctx, form, seed=9)
        assert got(ctx, qap, c.values) == (0, NONE, 0)
        for x in (150, 160, 113, 5, 100 + 13, 42):      # outputs of the 70-entry, duplicated and empty-U gates; inputs
            vals = list(c.values)
            vals[x] = (vals[x] + 1) % R
            want = c.expect(vals)
            assert want[0] >= 1
            assert got(ctx, qap, vals) == want, (form, x, want)


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------
def _batch(c, count, breaks, stride, pad_word=0xFFFFFFFFFFFFFFFF):
    """`count` instances cycling through 4 satisfying witnesses of the chain, instance j broken at wire breaks[j]; the padding
    between instances is all ones (>= r: a read of it would surface as ZK_ERR_RANGE).  -> (array (count, stride, 4), per-instance ints)"""
    log_n = c.n.bit_length() - 1
    base = []
    for k in range(4):
        rng = zk.SplitMix64(50 + k)
        base.append(limbs_to_ints(chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(c.n)])))
    arr = np.full((count, stride, 4), pad_word, dtype=np.uint64)
    base_limbs = [ints_to_limbs(b) for b in base]
    insts = []
    for j in range(count):
        vals = base[j % 4]
        arr[j, :c.m] = base_limbs[j % 4]
        if j in breaks:
            vals = list(vals)
            vals[breaks[j]] = (vals[breaks[j]] + 1) % R
            arr[j, breaks[j]] = ints_to_limbs([vals[breaks[j]]])[0]
        insts.append(vals)
    return arr, insts


def _check_batch(ctx, qap, c, arr, insts, m_in=None, host=True):
    import torch
    count, stride = arr.shape[0], arr.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()
    torch.cuda.synchronize()
    res = ctx.qap_check_dev(qap, d.data_ptr(), c.m if m_in is None else m_in, count, stride)
    cache = {}
    for j in range(count):
        key = id(insts[j])
        if key not in cache:
            cache[key] = c.expect(insts[j])
            if host:
                assert got(ctx, qap, insts[j]) == cache[key], j
        assert (int(res["bad_gates"][j]), int(res["first_bad"][j]), int(res["flags"][j])) == cache[key], (j, cache[key])
    return res


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("log_n", [4, 10])
def test_batches(ctx, store, log_n, count, pad):
    c = store.case("chain:%d" % log_n)
    qap = store.qap(ctx, "chain:%d" % log_n, "unity")
    n = c.n
    # a_k = wire 2k + 2 breaks gate k - 1; y = wire 2 breaks the last gate
    breaks = {j: w for j, w in ((0, 2 * 3 + 2), (63, 2), (64, 2 * 1 + 2), (count - 1, 2 * (n // 2) + 2)) if j < count}
    arr, insts = _batch(c, count, breaks, c.m + pad)
    res = _check_batch(ctx, qap, c, arr, insts)
    assert int((res["bad_gates"] != 0).sum()) == len(breaks)


def test_batch_crosses_the_chunk_limit_and_both_lane_mappings(ctx, store):
    c = store.case("chain:4")
    qap = store.qap(ctx, "chain:4", "unity")
    assert ctx.get_option("qap_check_chunk") == _lib.QAP_CHECK_CHUNK_LANES and ctx.get_option("qap_check_by_instance") == 0
    count = 200
    breaks = {6: 2 * 2 + 2, 7: 2, 13: 2 * 9 + 2, 14: 2 * 16 + 1, 199: 2 * 5 + 2}     # either side of the seams at 7 and 14
    arr, insts = _batch(c, count, breaks, c.m + 1)
    try:
        ctx.set_option("qap_check_chunk", 7 * c.n)      # 7 instances per launch: 29 chunks, the last one partial
        _check_batch(ctx, qap, c, arr, insts, host=False)
        ctx.set_option("qap_check_chunk", 1)            # below one instance: one instance per launch
        _check_batch(ctx, qap, c, arr[:9], insts[:9], host=False)
        ctx.set_option("qap_check_chunk", _lib.QAP_CHECK_CHUNK_LANES)
        ctx.set_option("qap_check_by_instance", 1)      # the other lane mapping gives the same results
        _check_batch(ctx, qap, c, arr, insts, host=False)
        c10 = store.case("chain:10")
        arr10, insts10 = _batch(c10, 65, {0: 8, 63: 2, 64: 4}, c10.m)
        _check_batch(ctx, store.qap(ctx, "chain:10", "unity"), c10, arr10, insts10, host=False)
        ctx.set_option("qap_check_chunk", 5 * c.n)
        _check_batch(ctx, qap, c, arr, insts, host=False)
    finally:
        ctx.set_option("qap_check_chunk", _lib.QAP_CHECK_CHUNK_LANES)
        ctx.set_option("qap_check_by_instance", 0)


# ---- 6. range -------------------------------------------------------------------------------------------------------------------
def test_range_errors_name_the_lowest_instance(ctx, store):
    import torch
    c = store.case("chain:4")
    qap = store.qap(ctx, "chain:4", "unity")
    arr, insts = _batch(c, 12, {}, c.m)
    r_limbs = ints_to_limbs([R])[0]
    bad = arr.copy()
    bad[9, 7] = r_limbs
    bad[5, c.m - 1] = r_limbs
    d = torch.from_numpy(bad.view(np.int64)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(zk.ZkError) as e:
        ctx.qap_check_dev(qap, d.data_ptr(), c.m, 12)
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 5" in str(e.value) and "9" not in str(e.value).split("instance")[1]
    with pytest.raises(zk.ZkError) as e:
        ctx.qap_check(qap, bad[9])
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 0" in str(e.value)
    # the same word behind a_len: witnesses longer than m_qap are legal and their tail is never read
    longer = np.zeros((12, c.m + 2, 4), np.uint64)
    longer[:, :c.m] = arr
    longer[:, c.m:] = r_limbs
    _check_batch(ctx, qap, c, longer, insts, m_in=c.m + 2, host=False)
    assert ctx.qap_check(qap, longer[0]) == (0, None, True)
    # the state is as good as new
    _check_batch(ctx, qap, c, arr, insts, host=False)


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, store):
    import torch
    lib = ctx.lib
    c = store.case("chain:4")
    qap = store.qap(ctx, "chain:4", "unity")
    w = np.ascontiguousarray(ints_to_limbs(c.values))
    wp = w.ctypes.data_as(_lib.u64p)
    d = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    dp = C.c_void_p(d.data_ptr())
    out = _lib.QapCheckResult(7, 8, 9)
    dense = Circuit(open(os.path.join(ROOT, "tests", "golden", "zk", "simple.zk")).read()).qap(ctx)
    w6 = np.ascontiguousarray(ints_to_limbs([1, 2, 34, 6, 3, 4]))
    assert lib.zk_qap_check(ctx.ptr, dense.ptr, w6.ctypes.data_as(_lib.u64p), 6, C.byref(out)) == _lib.ZK_ERR_UNSUPPORTED
    assert b"dense" in lib.zk_last_error(ctx.ptr)
    assert lib.zk_qap_check_dev(ctx.ptr, dense.ptr, dp, 6, 6, 1, C.byref(out)) == _lib.ZK_ERR_UNSUPPORTED
    assert lib.zk_qap_check_dev(ctx.ptr, qap.ptr, dp, c.m, c.m - 1, 1, C.byref(out)) == _lib.ZK_ERR_ARG      # stride < m
    assert lib.zk_qap_check_dev(ctx.ptr, qap.ptr, None, c.m, c.m, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(ctx.ptr, qap.ptr, dp, c.m, c.m, 1, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(ctx.ptr, None, dp, c.m, c.m, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(None, qap.ptr, dp, c.m, c.m, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(ctx.ptr, qap.ptr, None, c.m, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(ctx.ptr, qap.ptr, wp, c.m, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(ctx.ptr, None, wp, c.m, C.byref(out)) == _lib.ZK_ERR_ARG
    # count == 0: ZK_OK, the poisoned record untouched, nothing dereferenced
    assert lib.zk_qap_check_dev(ctx.ptr, qap.ptr, None, c.m, 0, 0, C.byref(out)) == _lib.ZK_OK
    assert lib.zk_qap_check_dev(ctx.ptr, qap.ptr, dp, c.m, c.m, 0, None) == _lib.ZK_OK
    assert (out.bad_gates, out.first_bad, out.flags) == (7, 8, 9)
    # a QAP of another context
    other = zk.Context(0)
    try:
        assert lib.zk_qap_check(other.ptr, qap.ptr, wp, c.m, C.byref(out)) == _lib.ZK_ERR_ARG
        assert lib.zk_qap_check_dev(other.ptr, qap.ptr, dp, c.m, c.m, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    finally:
        other.close()
    assert (out.bad_gates, out.first_bad, out.flags) == (7, 8, 9)
    # no witness at all: every row sum is 0, so every gate holds, and the constant wire is not 1
    assert got(ctx, qap, []) == (0, NONE, WIRE0)
    assert c.expect([], 0) == (0, NONE, WIRE0)
    # zk_qap_weighted_sum keeps refusing w on the sparse forms
    with pytest.raises(zk.ZkError) as e:
        ctx.qap_weighted_sum(qap, w, 2)
    assert e.value.status == _lib.ZK_ERR_UNSUPPORTED
    assert got(ctx, qap, c.values) == (0, NONE, 0)


# ---- 8. with the generator and the prover ---------------------------------------------------------------------------------------
def test_with_the_generator_and_the_prover(ctx):
    import torch
    code = chain_zk(16)
    circ = Circuit(code)
    qap = circ.qap_sparse(ctx)
    c = Case(circ.n, circ.m, circ.input, circ.rows(0), circ.rows(1), circ.rows(2), [0] * circ.m)
    count = 200
    rng = zk.SplitMix64(81)
    ins = ints_to_limbs([rng.fr() for _ in range(count * circ.n_in)]).reshape(count, circ.n_in, 4)
    d_in = torch.from_numpy(ins.view(np.int64)).cuda()
    d_out = torch.zeros((count, circ.m, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    wg = Witgen(ctx, circ)
    res = wg.run_checked(qap, d_in.data_ptr(), count, d_out.data_ptr())
    assert res.dtype == zk.Context.QAP_CHECK_DTYPE and res.shape == (count,)
    assert not res["bad_gates"].any() and (res["first_bad"] == NONE).all() and not res["flags"].any()
    # one element of instance 77 replaced on the device by another value < r: t_9 = wire 19, W of gate 8 and V of gate 9
    other = rng.fr()
    d_out[77, 19] = torch.from_numpy(ints_to_limbs([other]).view(np.int64))[0].cuda()
    torch.cuda.synchronize()
    res = ctx.qap_check_dev(qap, d_out.data_ptr(), circ.m, count)
    wits = d_out.cpu().numpy().view(np.uint64)
    vals77 = limbs_to_ints(wits[77])
    want = c.expect(vals77)
    assert want[0] == 2 and want[1] == 8
    assert np.flatnonzero(res["bad_gates"]).tolist() == [77]
    assert (int(res["bad_gates"][77]), int(res["first_bad"][77]), int(res["flags"][77])) == want
    # the prover and the verifier agree with the check in all three cases
    crs = ctx.setup(qap, [rng.fr() for _ in range(5)])
    r, s = rng.fr(), rng.fr()
    good = wits[3]
    assert c.expect(limbs_to_ints(good)) == (0, NONE, 0)
    assert ctx.verify(crs, good[1:1 + circ.input], ctx.prove(crs, qap, good, r, s)) is True
    assert ctx.verify(crs, wits[77][1:1 + circ.input], ctx.prove(crs, qap, wits[77], r, s)) is False
    # every gate holds with the constant wire at 2: y = wire 2 = 2 (t_15 + a_16) -- only the flag tells
    v = limbs_to_ints(good)
    v[0] = 2
    v[2] = 2 * v[2] % R
    assert c.expect(v) == (0, NONE, WIRE0)
    assert got(ctx, qap, v) == (0, NONE, WIRE0)
    w2 = ints_to_limbs(v)
    assert ctx.verify(crs, w2[1:1 + circ.input], ctx.prove(crs, qap, w2, r, s)) is False
    wg.close()


# ---- 9. a ticket in flight ------------------------------------------------------------------------------------------------------
def test_check_under_an_outstanding_ticket(ctx, store):
    import torch
    c = store.case("chain:10")
    qap = store.qap(ctx, "chain:10", "unity")
    rng = zk.SplitMix64(91)
    crs = ctx.setup(qap, [rng.fr() for _ in range(5)])
    r, s = rng.fr(), rng.fr()
    w = np.ascontiguousarray(ints_to_limbs(c.values))
    d = torch.from_numpy(w.view(np.int64)).cuda()
    torch.cuda.synchronize()
    sync = ctx.prove_dev(crs, qap, d.data_ptr(), c.m, r, s)
    vals = list(c.values)
    vals[2 * 500 + 2] = (vals[2 * 500 + 2] + 1) % R
    t = ctx.prove_submit(crs, qap, d.data_ptr(), c.m, r, s)
    in_flight = (got(ctx, qap, vals), ctx.qap_check_dev(qap, d.data_ptr(), c.m, 1))
    proof = ctx.prove_wait(t)
    assert proof == sync
    assert in_flight[0] == c.expect(vals) and in_flight[0][1] == 499
    assert (int(in_flight[1]["bad_gates"][0]), int(in_flight[1]["first_bad"][0]), int(in_flight[1]["flags"][0])) == (0, NONE, 0)


# ---- 10. host APIs --------------------------------------------------------------------------------------------------------------
def test_cpp_host_api_on_the_device(tmp_path):
    exe = build_qap_check_api(tmp_path)
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "zk", "simple.zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().splitlines()[-1] == "ok", res.stdout + res.stderr


def test_python_host_api(ctx):
    code = open(os.path.join(ROOT, "tests", "golden", "zk", "simple.zk")).read()
    qap = groth16.QAP.from_zk(ctx, code, sparse=True)
    w = groth16.weights(code, [3, 2, 4])
    assert limbs_to_ints(w) == [1, 2, 34, 6, 3, 4]
    assert groth16.is_satisfied(qap, w) is True and groth16.first_unsatisfied(qap, w) is None
    bad = w.copy()
    bad[2, 0] = 35                                      # the output wire: only W of the last gate reads it
    assert groth16.is_satisfied(qap, bad) is False and groth16.first_unsatisfied(qap, bad) == qap.circuit.n - 1
    one = w.copy()
    one[0, 0] = 2
    assert groth16.is_satisfied(qap, one) is False
    assert ctx.qap_check(qap.handle, one)[2] is False
    with pytest.raises(zk.ZkError) as e:
        groth16.is_satisfied(groth16.QAP.from_zk(ctx, code), w)
    assert e.value.status == _lib.ZK_ERR_UNSUPPORTED


def test_profile_sees_the_kernel(ctx, store):
    c = store.case("chain:4")
    qap = store.qap(ctx, "chain:4", "unity")
    keep = ctx.get_option("profile")
    try:
        ctx.set_option("profile", 2)
        ctx.profile_reset()
        assert got(ctx, qap, c.values) == (0, NONE, 0)
        prof = ctx.profile()
    finally:
        ctx.set_option("profile", keep)
        ctx.profile_reset()
    assert prof["qap_check"]["launches"] == 1 and prof["qap_check"]["algo_bytes"] > 0
