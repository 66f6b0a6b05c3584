"""Circuits shaped like real R1CS instances, and the CPU checks of their generator (the GPU side: tests/test_gpu_circuit_shapes.py).

The chain circuit and random_sparse_rows (tests/test_gpu_prove.py) have short gates and hardly any unused wire.  `shaped_circuit`
builds gates (sum u a)(sum v a) = a_out with
  - wide gates: U and V rows of exactly 1, 63, 64, 65, 127, 128, 129, 1000, 1500 and 4096 entries (k_spmv reduces its lazy sum every
    64 entries; the top limb of 1000 unreduced products still fits in 32 bits, that of 1500 no longer does), one gate that reads every
    public input that is read at all, repeated (wire, gate) pairs, coefficients r - 1 and (r - 1) / 2;
  - zero columns: a contiguous block of 5/16 of the wires at the end and scattered wires (the first private wire l + 1 included) appear
    in no row, so their sum_delta points are infinity; wires only in U, only in V and only in W (every gate output);
  - public inputs no gate reads (infinity sum_gamma points); the constant wire in every gate;
  - a satisfying witness with values r - 1 and (r - 1) / 2, and non-zero values (r - 1 included) on every unused wire.

This module (no GPU): the witness satisfies every gate, and the oracle's setup puts infinity exactly at the unused wires' sum_delta /
sum_gamma entries.  It also holds the model of the G1 accumulation's fast loop that the GPU module's docstrings quote.
"""
import itertools

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, limbs_to_ints, R_MODULUS as R

WIDE = (1, 63, 64, 65, 127, 128, 129, 1000, 1500, 4096)
HALF = (R - 1) // 2


def _fr(rng, count):
    """uniform values of [0, r) as Python ints"""
    out = []
    while len(out) < count:
        a = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 62) - 1)
        out += [x for x in limbs_to_ints(a) if x < R]
    return out[:count]


def _by_wire(entries, m):
    """[(wire, gate, value)] -> (ptr[m + 1], gate[nnz], val[nnz, 4]) by wire; entries of one wire keep their order (duplicates stay)"""
    wires = np.array([e[0] for e in entries], np.int64)
    order = np.argsort(wires, kind="stable")
    ptr = np.zeros(m + 1, np.uint64)
    np.add.at(ptr, wires + 1, 1)
    ptr = np.cumsum(ptr).astype(np.uint64)
    gate = np.array([entries[i][1] for i in order], np.uint32)
    val = ints_to_limbs([entries[i][2] for i in order]).reshape(-1, 4)
    return ptr, gate, val


def shaped_circuit(n, m, l, seed):
    """(n gates, m wires, l public inputs) -> dict(u, v, w (rows by wire), weights ((m, 4) limbs, satisfying), values (ints),
    unused, only_u, only_v, only_w, unread_public (sets of wires), wide (gate -> width), gate_u / gate_v ([(wire, value)] per gate))."""
    assert n >= len(WIDE) + 2 and l >= 8
    rng = np.random.default_rng(seed)
    block_start = m - (5 * m) // 16                        # wires [block_start, m): in no row (the last rank's share at world 4)
    scattered = {l + 1} | {x for x in range(l + 2, block_start) if (x - l) % 41 == 0}
    unread_public = {3, l // 2, l}
    rest = [x for x in range(l + 2, block_start) if x not in scattered]
    rest = list(rng.permutation(rest))
    outputs, free = [int(x) for x in rest[:n]], [int(x) for x in rest[n:]]
    assert len(free) >= 1100, "m too small for the wide gates"
    tenth = len(free) // 10
    u_only, v_only, both = free[:tenth], free[tenth:2 * tenth], free[2 * tenth:]
    public = [x for x in range(1, l + 1) if x not in unread_public]
    pool_u, pool_v = public + both + u_only, public + both + v_only   # every wire listed here is read somewhere (the cycles below)

    coef = iter(_fr(rng, 12 * n + 2 * m + 20000))
    special = [R - 1, HALF]

    def c():
        x = next(coef)
        return special[x & 1] if x % 7 == 0 else x

    gate_u, gate_v = [[] for _ in range(n)], [[] for _ in range(n)]
    wide = {}
    for g, width in enumerate(WIDE, start=1):              # gates 1..10: wide rows (gate 0 and the others: short ones)
        wide[g] = width
        for rows, pool in ((gate_u, pool_u), (gate_v, pool_v)):
            rows[g].append((0, c()))                       # the constant wire in every gate
            k = width - 1
            if k <= len(pool) // 2:
                picks = sorted(rng.choice(len(pool), size=k, replace=False).tolist())
                if width == 65:                            # repeated (wire, gate) pairs in one row
                    picks[-4:] = [picks[0]] * 4
            else:
                picks = rng.integers(0, len(pool), size=k).tolist()
            rows[g] += [(pool[i], c()) for i in picks]
    every = len(WIDE) + 1                                  # one gate reads every public input that is read at all
    gate_u[every] = [(0, c())] + [(x, c()) for x in public]
    gate_v[every] = [(0, c()), (public[0], R - 1)]
    cu = cv = 0
    for g in range(n):
        for rows, pool, cyc in ((gate_u, pool_u, 0), (gate_v, pool_v, 1)):
            if rows[g]:
                continue
            rows[g].append((0, c()))
            for _ in range(2):                             # cycle through the pool: every listed wire is read
                if cyc == 0:
                    rows[g].append((pool[cu % len(pool)], c())); cu += 1
                else:
                    rows[g].append((pool[cv % len(pool)], c())); cv += 1
            for _ in range(int(rng.integers(0, 3))):
                rows[g].append((pool[int(rng.integers(0, len(pool)))], c()))
    # cover what the cycles did not reach
    for x in pool_u[cu:] if cu < len(pool_u) else []:
        gate_u[len(WIDE) + 2 + (x % (n - len(WIDE) - 2))].append((x, c()))
    for x in pool_v[cv:] if cv < len(pool_v) else []:
        gate_v[len(WIDE) + 2 + (x % (n - len(WIDE) - 2))].append((x, c()))

    # witness: inputs first, then every gate's output (gates read inputs only)
    vals = [0] * m
    outs = set(outputs)
    inputs = [x for x in range(1, m) if x not in outs]
    draw = _fr(rng, len(inputs))
    for x, y in zip(inputs, draw):
        vals[x] = y or 1
    vals[0] = 1
    for k, x in enumerate(inputs):
        if k % 13 == 0:
            vals[x] = R - 1
        elif k % 13 == 1:
            vals[x] = HALF
    vals[l + 1] = vals[m - 1] = R - 1                       # unused wires multiply infinity points by non-zero digits
    for g in range(n):
        su = sum(a * vals[x] for x, a in gate_u[g]) % R
        sv = sum(a * vals[x] for x, a in gate_v[g]) % R
        vals[outputs[g]] = su * sv % R
    ue = [(x, g, a) for g in range(n) for x, a in gate_u[g]]
    ve = [(x, g, a) for g in range(n) for x, a in gate_v[g]]
    we = [(outputs[g], g, 1) for g in range(n)]
    in_u, in_v, in_w = {e[0] for e in ue}, {e[0] for e in ve}, {e[0] for e in we}
    used = in_u | in_v | in_w
    return dict(n=n, m=m, l=l, u=_by_wire(ue, m), v=_by_wire(ve, m), w=_by_wire(we, m), values=vals, weights=ints_to_limbs(vals),
                gate_u=gate_u, gate_v=gate_v, outputs=outputs, wide=wide, block_start=block_start,
                unused={x for x in range(m) if x not in used}, only_u=in_u - in_v - in_w, only_v=in_v - in_u - in_w,
                only_w=in_w - in_u - in_v, unread_public={x for x in range(1, l + 1) if x not in used})


def default_m(n, l=40):
    return 4 * n + l + 2000


# ---- the G1 accumulation's fast loop (csrc/msm_impl.hpp), as a model over the order of one run's entries ----------------------
def lane_events(seq, ev_at):
    """seq: 'F' (finite) / 'I' (infinity) per position of a run (1-based positions); ev_at: the ordinal (1-based) of the finite entry
    that meets +-the accumulator, or None.  Positions 1 and 2 take the generic step; the fast loop starts at 3 (even half: 3, 5, ..;
    odd half: 4, 6, ..) if the accumulator is not empty, and leaves at the first infinity or at the same-x event.  Returns the set of
    events: ('exit', p) the loop left at an infinity at position p, ('consecutive',) that infinity is followed by another, ('last',)
    it is the run's last entry, ('ev_inf',) an infinity right behind a same-x event in the fast loop."""
    finite = 0
    acc = False
    for p in (1, 2):
        if p <= len(seq) and seq[p - 1] == "F":
            finite += 1
            acc = not (ev_at == finite and acc)            # P + (-P) inside the generic step empties it (doubling keeps it)
    out = set()
    if not acc:
        return out
    for p in range(3, len(seq) + 1):
        if seq[p - 1] == "I":
            out.add(("exit", p))
            if p < len(seq) and seq[p] == "I":
                out.add(("consecutive",))
            if p == len(seq):
                out.add(("last",))
            return out
        finite += 1
        if ev_at == finite:
            if p < len(seq) and seq[p] == "I":
                out.add(("ev_inf",))
            return out
    return out


def expected_events(k, j, ev_at, weight=1.0):
    """expected count of every lane event over ONE bucket of k entries, j of them infinity, in uniformly random order"""
    tot = {}
    sets = list(itertools.combinations(range(k), j))
    for s in sets:
        seq = ["F"] * k
        for i in s:
            seq[i] = "I"
        for e in lane_events(seq, ev_at):
            tot[e] = tot.get(e, 0.0) + weight / len(sets)
    return tot


# compositions of the single-run buckets: (name, finite entries, ev ordinal, probability that the event fires)
COMPOSITIONS = (("one", None), ("two", None), ("k-2", None), ("all-but-one", None), ("opposite-quad", 4), ("same-quad", 4),
                ("pair-opposite", 2), ("pair-same", 2))
SIZES = tuple(range(5, 13))
PER_CELL = 24        # buckets per (composition, size); late first infinities need the one-infinity buckets four times as often


def per_cell(name):
    return 4 * PER_CELL if name == "one" else PER_CELL


def infinities(name, k):
    return {"one": 1, "two": 2, "k-2": k - 2, "all-but-one": k - 1, "opposite-quad": k - 4, "same-quad": k - 4,
            "pair-opposite": k - 2, "pair-same": k - 2}[name]


def composition_expectations():
    tot = {}
    for name, ev in COMPOSITIONS:
        weight = 0.25 if name == "same-quad" else 1.0      # A + B + D meets itself only when it comes last of the four
        for k in SIZES:
            for e, x in expected_events(k, infinities(name, k), ev, 1.0).items():
                if e == ("ev_inf",):
                    x *= weight
                tot[e] = tot.get(e, 0.0) + per_cell(name) * x
    return tot


def test_fast_loop_model_expectations():
    """every event the GPU module's single-run buckets are meant to reach is expected in at least 20 buckets"""
    tot = composition_expectations()
    for p in range(3, 11):
        assert tot.get(("exit", p), 0) >= 20, p
    for e in (("consecutive",), ("last",), ("ev_inf",)):
        assert tot.get(e, 0) >= 20, e
    # the model itself on hand-checked runs
    assert lane_events("FFFI", None) == {("exit", 4), ("last",)}
    assert lane_events("IIFF", None) == set()                          # the accumulator is empty behind the generic steps
    assert lane_events("FIFII", None) == {("exit", 4), ("consecutive",)}
    assert lane_events("FFFFI", 4) == {("ev_inf",)}
    assert lane_events("FFIFF", 2) == set()                            # P + (-P) at position 2: the generic step
    assert abs(sum(expected_events(5, 1, None).get(("exit", p), 0) for p in range(3, 6)) - 3 / 5) < 1e-12


@pytest.mark.parametrize("log_n", [6, 10])
def test_shaped_circuit_is_satisfied_and_shaped(log_n):
    n, l = 1 << log_n, 40
    m = default_m(n, l)
    c = shaped_circuit(n, m, l, 11 + log_n)
    vals = c["values"]
    assert vals[0] == 1
    for g in range(n):
        su = sum(a * vals[x] for x, a in c["gate_u"][g]) % R
        sv = sum(a * vals[x] for x, a in c["gate_v"][g]) % R
        assert su * sv % R == vals[c["outputs"][g]], g
    # the same from the rows as uploaded (by wire): sum_i a_i u_i(g) * sum_i a_i v_i(g) == sum_i a_i w_i(g)
    sums = []
    for ptr, gate, val in (c["u"], c["v"], c["w"]):
        acc = [0] * n
        vv = limbs_to_ints(val)
        for x in range(m):
            for e in range(int(ptr[x]), int(ptr[x + 1])):
                acc[int(gate[e])] = (acc[int(gate[e])] + vals[x] * vv[e]) % R
        sums.append(acc)
    assert all(a * b % R == w for a, b, w in zip(*sums))
    # the shapes the GPU module relies on
    for g, width in c["wide"].items():
        assert len(c["gate_u"][g]) == width and len(c["gate_v"][g]) == width
        assert all(x == 0 for x, _ in c["gate_u"][g][:1])
    assert len({x for x, _ in c["gate_u"][4]}) < 65                  # the 65-entry row repeats a (wire, gate) pair
    assert all(any(x == 0 for x, _ in c["gate_u"][g] + c["gate_v"][g]) for g in range(n))
    unused = c["unused"]
    assert set(range(c["block_start"], m)) <= unused and (m - c["block_start"]) * 4 >= m
    assert {l + 1, m - 1} <= unused and len(unused - set(range(c["block_start"], m))) >= 2 * log_n
    assert c["only_u"] and c["only_v"] and len(c["only_w"]) == n
    assert c["unread_public"] == {3, l // 2, l}
    assert all(vals[x] != 0 for x in unused) and vals[l + 1] == vals[m - 1] == R - 1
    vals_all = limbs_to_ints(np.concatenate([c["u"][2], c["v"][2]]))
    assert R - 1 in vals_all and HALF in vals_all and R - 1 in vals and HALF in vals


def test_oracle_puts_infinity_exactly_at_unused_wires(orc):
    """n = 2^6: the oracle's setup gives the point at infinity (all-zero encoding) exactly at the sum_delta entries of the private
    wires in no row and the sum_gamma entries of the public inputs in no row, and nowhere else in those arrays"""
    log_n, l = 6, 40
    n = 1 << log_n
    m = default_m(n, l)
    c = shaped_circuit(n, m, l, 17)
    desc = zk.Context.sparse_desc(log_n, m, l, c["u"], c["v"], c["w"])
    rng = zk.SplitMix64(18)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    arrs = orc.setup_sparse(desc, td, n, m, l, False)
    inf_delta = {l + 1 + i for i in np.flatnonzero(~arrs["sum_delta_g1"].any(axis=1))}
    inf_gamma = set(np.flatnonzero(~arrs["sum_gamma_g1"].any(axis=1)).tolist())
    assert inf_delta == {x for x in c["unused"] if x > l}
    assert inf_gamma == c["unread_public"]
    assert arrs["xi_g1"].any(axis=1).all() and arrs["xi_t_g1"].any(axis=1).all()
