"""Case lists and helpers shared by test_setup_edges.py (host) and test_gpu_setup_edges.py (device): the trapdoors a random draw
never produces -- x on a root of t, elements at the ends of [1, r), scalars that reach every entry of the fixed-base tables."""
import numpy as np

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs, limbs_to_int
from zksnark_rs_amd.circuits import chain_rows, chain_weights

R = zk.R_MODULUS
HALF = (R - 1) // 2

# ---- x on the domain, roots of unity: (log_n, the indices j of x = w^j) --------------------------------------------------------
# host: the sizes the faithful oracle reaches
HOST_ON_DOMAIN = {log_n: sorted({0, 1 % (1 << log_n), (1 << log_n) // 2, (1 << log_n) - 1}) for log_n in (0, 1, 3, 5)}
# device: every j at the smallest sizes; 2^8 = exactly one 256-lane block of k_lagrange_at (first lanes, middle, last lane); 2^9 = two
# blocks (first lane, the two lanes at the block boundary, last lane)
GPU_ON_DOMAIN = {0: [0], 1: [0, 1], 3: list(range(8)), 8: [0, 1, 128, 255], 9: [0, 255, 256, 511]}
# proofs over the degenerate CRS: j = 0 (x = 1) and one more; n / 2 is x = -1
GPU_ON_DOMAIN_PROVE = {1: [0, 1], 3: [0, 5], 9: [0, 256]}
# the host verdict rule (log_n = 3)
VERDICT_LOG_N, VERDICT_J = 3, (0, 4)


def domain_point(orc, log_n, j):
    """w^j for the 2^log_n-th root of unity w the oracle (and the device) use"""
    return pow(limbs_to_int(orc.root_of_unity(log_n)), j, R)


def on_domain_trapdoor(orc, log_n, j, seed=0):
    """(alpha, beta, gamma, delta) from SplitMix64, x = w^j, as (5, 4) limbs"""
    rng = SplitMix64(31000 + 1000 * log_n + j + 100000 * seed)
    return ints_to_limbs([rng.fr() for _ in range(4)] + [domain_point(orc, log_n, j)])


def a_wire(log_n, k):
    """the wire of the chain circuit's input a_k, k = 1..n (gate k sits at domain point w^(k-1))"""
    n = 1 << log_n
    return 2 * k + 2 if k < n else 2 * n + 1


def chain_witnesses(log_n, j, seed=0):
    """(honest, a_(j+1) changed: gate j fails, a_k changed for a gate other than j: that gate fails) -- three (m, 4) limb arrays with
    the same public inputs x, y; every altered value stays in [0, r).  log_n >= 1."""
    n = 1 << log_n
    assert n >= 2 and 0 <= j < n
    rng = SplitMix64(32000 + 1000 * log_n + j + 100000 * seed)
    honest = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(n)])
    out = [honest]
    for gate in (j, (j + 1) % n):
        bad = honest.copy()
        wire = a_wire(log_n, gate + 1)
        bad[wire] = ints_to_limbs([(limbs_to_int(honest[wire]) + 1) % R])[0]
        out.append(bad)
    assert np.array_equal(out[1][:3], honest[:3]) and np.array_equal(out[2][:3], honest[:3])
    return tuple(out)


VERDICTS = (True, False, True)      # of chain_witnesses' three proofs over a CRS with x = w^j: only gate j is checked


def chain_sparse(log_n):
    """(n, m, l, u, v, w, desc) of the chain circuit over the roots of unity"""
    m, l, u, v, w = chain_rows(log_n)
    return 1 << log_n, m, l, u, v, w, zk.Context.sparse_desc(log_n, m, l, u, v, w)


def is_infinity(points):
    """per point of an (k, words) array: the all-zero encoding"""
    points = np.asarray(points)
    return ~points.reshape(len(points), points.shape[-1]).any(axis=1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
INTEGER_SIZES = (1, 2, 5, 300)        # 2n - 1 = 599 lanes of k_ap_lagrange: three blocks of 256
ARBITRARY_SIZES = (1, 5, 257)         # 257: the second block of k_arb_lagrange holds one lane


def integer_refused(n):
    """the ends of 1..2n-1 and of its two halves (the roots R = 1..n, the second set S = n+1..2n-1)"""
    return sorted({x for x in (1, n, n + 1, 2 * n - 1) if 1 <= x <= 2 * n - 1})


def integer_accepted(n):
    return [2 * n, R - 1]


BAD_ELEMENTS = ((0, "ZK_ERR_DIV_BY_ZERO"), (R, "ZK_ERR_RANGE"), (2 ** 256 - 1, "ZK_ERR_RANGE"))

# ---- trapdoor scalars at their ends (alpha, beta, gamma, delta; None = drawn) ---------------------------------------------------
SCALAR_EDGES = [("ones", (1, 1, 1, 1)), ("r-1", (R - 1,) * 4), ("half", (HALF,) * 4), ("2^253", (1 << 253,) * 4),
                ("gamma=delta,alpha=beta", ("a", "a", "g", "g"))]
SCALAR_EDGES += [("%s=r-1" % name, tuple(R - 1 if k == pos else None for k in range(4)))
                 for pos, name in enumerate(("alpha", "beta", "gamma", "delta"))]
assert (1 << 253) < R


def scalar_edge_trapdoor(spec, seed):
    rng = SplitMix64(33000 + seed)
    shared = {"a": rng.fr(), "g": rng.fr()}
    els = [shared[e] if isinstance(e, str) else (rng.fr() if e is None else e) for e in spec]
    return ints_to_limbs(els + [rng.fr()])


# ---- every entry of the fixed-base tables FT[w][d] = d 16^w base ------------------------------------------------------------------
def table_entries():
    """every (window, digit) with a table entry that a scalar < r can select: all of d = 1..15 below the top window, d <= 3 in it"""
    return [(w, d) for w in range(64) for d in range(1, 16) if d << (4 * w) < R]


def digits(s):
    """the (window, digit) pairs of the non-zero 4-bit digits of s"""
    return {(w, (s >> (4 * w)) & 15) for w in range(64)} - {(w, 0) for w in range(64)}


def digit_scalars():
    """d 16^w for every table entry (one mixed addition into an empty accumulator each), 16^w - 1 (w additions of digit 15, the
    windows above skipped), 0 (no addition: infinity), 1, r - 1 and the largest value < r whose 63 low digits are all 15"""
    out = [d << (4 * w) for w, d in table_entries()]
    top = max(d for w, d in table_entries() if w == 63)
    full = (top << 252) - 1                          # top digit one less than r's, every digit below it 15
    assert full < R and digits(full) == {(w, 15) for w in range(63)} | {(63, top - 1)}
    for s in [(1 << (4 * w)) - 1 for w in range(1, 64)] + [0, 1, R - 1, full]:      # (16^1 - 1 and 1 are table entries already)
        if s not in out:
            out.append(s)
    assert len(set(out)) == len(out) and all(0 <= s < R for s in out)
    return out


W_QAP_INPUT = 40


def unit_w_qap(scalars):
    """The one-gate QAP over the roots of unity (log_n = 0) with m = len(scalars) wires, l = 40: wire i has the single entry
    w_i(gate 0) = scalars[i] (an explicit entry also where that is 0) and no u / v entry.  With x = 1 = w^0 the Lagrange value is
    L_0 = 1, so with gamma = delta = 1 the CRS holds sum_gamma | sum_delta = [scalars[i]]_1 whatever alpha and beta are.
    -> (m, l, u, v, w)"""
    m = len(scalars)
    assert m > W_QAP_INPUT + 1
    empty = (np.zeros(m + 1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64))
    w = (np.arange(m + 1, dtype=np.uint64), np.zeros(m, np.uint32), ints_to_limbs(list(scalars)))
    return m, W_QAP_INPUT, empty, empty, w


G2_POWER_CASES = ((8, 2), (6, 16))    # (log_n, x): xi = [2^i] (one bit per scalar, wrapping past r at i = 254) and [16^i] (digit 1 of window i)
G2_ELEMENTS = [15 << (4 * w) for w in (0, 31, 62)] + [3 << 252, R - 1, 1]
assert all(0 < s < R for s in G2_ELEMENTS)
