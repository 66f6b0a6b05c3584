"""-m gpu: stand-alone inner products (zk_msm_g1 / zk_msm_g2) at the sizes where msm_run changes its mind, and buckets that end
exactly at, just before and just behind a run of the accumulation -- at T = 128, T = 256, a run_fill value and the plain 32.

Large sizes need a reference that is exact and cheap.  The points are tiled from a pool of 4096 distinct oracle-made points, so
    sum_i k_i P_(i mod 4096) = sum_j (sum_{i = j mod 4096} k_i mod r) P_j :
4096 integer sums in Python and ONE oracle product over 4096 points, independent of the GPU at any n.  The boundary constructions
use the same idea: every entry is a pool point, a point made from pool points by the oracle, or infinity, and the reference is the
oracle's product over the distinct points with the summed scalars.

After every product the plan the library recorded (Context.msm_plans()) must equal the restatement of tests/msm_plan_model.py; the sizes
come from that restatement evaluated at the device's compute-unit count, not from constants."""
import numpy as np
import pytest

import msm_plan_model as M
from msm_plan_model import assert_plans, device_cu, limbs
from zksnark_rs_amd import ints_to_limbs, R_MODULUS as R
from test_digit_recoding import recoding_cases
from test_gpu_circuit_shapes import _point_pool, options

pytestmark = pytest.mark.gpu
POOL = M.POOL
R_LIMBS = np.array([(R >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


@pytest.fixture(scope="module")
def pool(orc):
    p1, p2 = _point_pool(orc, 71, POOL)
    assert len({bytes(p) for p in p1}) == POOL and len({bytes(p) for p in p2}) == POOL
    return p1, p2


def uniform_scalars(gen, n):
    """(n, 4) limbs, uniform over [0, r): 254-bit draws, those >= r drawn again"""
    a = gen.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 62) - 1)
    while True:
        ge = np.zeros(n, bool)
        eq = np.ones(n, bool)
        for k in (3, 2, 1, 0):
            ge |= eq & (a[:, k] > R_LIMBS[k])
            eq &= a[:, k] == R_LIMBS[k]
        redo = np.flatnonzero(ge | eq)
        if not len(redo):
            return a
        fresh = gen.integers(0, 1 << 64, size=(len(redo), 4), dtype=np.uint64)
        fresh[:, 3] &= np.uint64((1 << 62) - 1)
        a[redo] = fresh


def folded(scalars):
    """per pool point j the sum of the scalars at positions j, j + 4096, ..: exact integers mod r, from 32-bit half sums"""
    n = len(scalars)
    rows = -(-n // POOL)
    a = np.zeros((rows * POOL, 4), np.uint64)
    a[:n] = scalars
    a = a.reshape(rows, POOL, 4)
    lo = (a & np.uint64(0xFFFFFFFF)).sum(axis=0)
    hi = (a >> np.uint64(32)).sum(axis=0)
    assert rows < 1 << 31
    return limbs([sum((int(lo[j, k]) + (int(hi[j, k]) << 32)) << (64 * k) for k in range(4)) % R for j in range(POOL)])


def tiled(pts, n):
    return np.ascontiguousarray(np.tile(pts, (-(-n // POOL), 1))[:n])


def scalar_sets(n, c, seed):
    """uniform scalars with the recoding's edge scalars for window size c sprinkled in; and a set where a third of the scalars take
    five small values (five heavy buckets under whatever run length the size has)"""
    gen = np.random.default_rng(seed)
    a = uniform_scalars(gen, n)
    edge = ints_to_limbs(recoding_cases(c))
    a[gen.choice(n, size=len(edge), replace=False)] = edge
    b = uniform_scalars(gen, n)
    small = gen.choice(n, size=n // 3, replace=False)
    b[small] = 0
    b[small, 0] = np.array([1, 2, 3, 5, 1 << (c - 1)], np.uint64)[gen.integers(0, 5, size=len(small))]
    return a, b


def check_tiled(ctx, orc, pool, n, g2, cu, window_bits=0):
    c = M.msm_plan(n, g2, cu, window_bits=window_bits)["c"]
    pts = tiled(pool[1] if g2 else pool[0], n)
    gpu, ref = (ctx.msm_g2, orc.msm_g2) if g2 else (ctx.msm_g1, orc.msm_g1)
    for which, k in enumerate(scalar_sets(n, c, 7700 + n % 9973)):
        want = ref(pool[1] if g2 else pool[0], folded(k))
        for quad in ((0, 1 << 22) if window_bits == 0 else (None,)):
            ctx.msm_plan_reset()
            if quad is None:
                got = gpu(pts, k, window_bits)
                want_plan = M.msm_plan(n, g2, cu, window_bits=window_bits)
            else:
                with options(ctx, msm_quad_buckets=quad):
                    got = gpu(pts, k, window_bits)
                want_plan = M.msm_plan(n, g2, cu, quad_buckets=quad)
            assert_plans(ctx, [want_plan], (n, g2, which, quad))
            assert np.array_equal(got, want), (n, g2, which, quad, M.describe(want_plan))


def test_folded_reference_is_the_plain_sum(orc, pool):
    """the reference against itself at a size the oracle sums directly: 3 * 4096 + 5 tiled points"""
    n = 3 * POOL + 5
    k = scalar_sets(n, 13, 1)[0]
    assert np.array_equal(orc.msm_g1(pool[0], folded(k)), orc.msm_g1(tiled(pool[0], n), k))
    assert np.array_equal(orc.msm_g2(pool[1], folded(k)), orc.msm_g2(tiled(pool[1], n), k))


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("slot", range(7))
def test_msm_at_the_band_sizes(ctx, orc, pool, slot, g2):
    """zk_msm at the automatic window, n on both sides of every change of the run-length rule in the c = 17 band (128 | 256 entries
    per run, whole | run_fill), in the middle of the run_fill stretch, and at 2^20 - 9 | 2^20 - 8 (c = 17 | 20): both scalar sets, both
    tail forms, the plan as restated."""
    cu = device_cu(ctx, orc)
    n = M.band_17(g2, cu)[0][slot]
    check_tiled(ctx, orc, pool, n, g2, cu)


@pytest.mark.parametrize("slot", range(12))
def test_msm_at_the_lane_count_edges(ctx, orc, pool, slot):
    """three thresholds no automatic window reaches, at an explicit window of 13 bits: the last product with shortened runs and the
    first with runs of 32; the last whose runs of 32 fit the chip's lanes and the first that takes run_fill; the last product that
    is not chained and the first that is -- in G1 and in G2"""
    cu = device_cu(ctx, orc)
    n, g2 = M.edge_sizes(cu)[slot]
    check_tiled(ctx, orc, pool, n, g2, cu, window_bits=M.EDGE_WINDOW)


# ---- buckets at the run boundaries ----------------------------------------------------------------------------------------------
def prefix_sums(orc, pts, g2):
    """PS[i] = pts[0] + .. + pts[i]  (Hillis-Steele over the oracle's batched addition)"""
    add = orc.g2_add_batch if g2 else orc.g1_add_batch
    ps = pts.copy()
    d = 1
    while d < len(ps):
        ps[d:] = add(ps[d:], ps[:-d].copy())
        d *= 2
    return ps


def boundary_product(orc, pool, T, c, n, g2, seed):
    """(points, digits, distinct points, their summed digits) of the construction for run length T (msm_plan_model.boundary_classes),
    filled up to n scalars with entries at infinity in other buckets, in random order.  Bucket d holds the entries of scalar d."""
    pts = pool[1] if g2 else pool[0]
    words = pts.shape[1]
    ext = np.concatenate([pts, pts[:3 * T + 8]])                   # windows of consecutive pool points, cyclic
    ps = prefix_sums(orc, ext, g2)
    mul = orc.g2_mul_batch if g2 else orc.g1_mul_batch
    add = orc.g2_add_batch if g2 else orc.g1_add_batch
    minus1 = ints_to_limbs([R - 1])
    specials, special_id = [], {}
    ids, digits = [], []
    d = 0
    INF = -1
    def special(keys, make):
        """ids of the oracle-made points `keys` name, made once each by make(new keys)"""
        new = sorted({key for key in keys if key not in special_id})
        if new:
            for key, p in zip(new, make(new)):
                special_id[key] = POOL + len(specials)
                specials.append(p)
        return np.array([special_id[key] for key in keys])[:, None]

    for name, z, finite, count in M.boundary_classes(T):
        starts = 1 + (np.arange(count) * 61 + 7 * z) % (POOL - 8)
        if name.startswith("copies"):                              # T copies of Q = pool[start] and S = multiplier * Q
            mult = M.copies_multiplier(name, T) % R
            cols = [np.repeat(starts[:, None], T, axis=1),
                    special([(int(a), mult, "copies") for a in starts],
                            lambda new: mul(pts[[key[0] for key in new]], np.tile(ints_to_limbs([mult]), (len(new), 1))))]
        elif name.startswith("pair"):                              # P = pool[start] and -P or P again
            other = starts[:, None] if name == "pair same" else special(
                [(int(a), R - 1, "copies") for a in starts], lambda new: mul(pts[[key[0] for key in new]], np.tile(minus1, (len(new), 1))))
            cols = [starts[:, None], other]
        else:
            k = finite - 1 if name in ("zero", "double") else finite   # distinct pool points of the bucket
            cols = [(starts[:, None] + np.arange(k)[None, :]) % POOL]
            if name in ("zero", "double"):
                def window(new):                                   # P_a + .. + P_(a + k - 1), negated for 'zero'
                    a = np.array([key[0] for key in new])
                    w = add(ps[a + k - 1], mul(ps[a - 1], np.tile(minus1, (len(a), 1))))
                    return mul(w, np.tile(minus1, (len(a), 1))) if name == "zero" else w
                cols.append(special([(int(a), k, name) for a in starts], window))
        if z > finite:
            cols.append(np.full((count, z - finite), INF))
        block = np.concatenate(cols, axis=1)
        assert block.shape == (count, z)
        ids.append(block.reshape(-1))
        digits.append(np.repeat(np.arange(d + 1, d + 1 + count), z))
        d += count
    ids, digits = np.concatenate(ids), np.concatenate(digits)
    assert len(ids) == M.boundary_entries(T) <= n and d + 64 <= 1 << (c - 1)
    filler = n - len(ids)
    ids = np.concatenate([ids, np.full(filler, INF)])
    digits = np.concatenate([digits, d + 1 + np.arange(filler) % ((1 << (c - 1)) - d)])
    assert digits.max() <= 1 << (c - 1)
    distinct = np.concatenate([pts, np.array(specials, np.uint64).reshape(-1, words), np.zeros((1, words), np.uint64)])
    order = np.random.default_rng(seed).permutation(n)              # every order of a bucket's entries is equally likely
    ids, digits = ids[order], digits[order]
    finite_mask = ids != INF
    coeff = np.bincount(ids[finite_mask], weights=digits[finite_mask].astype(np.float64), minlength=len(distinct) - 1)
    assert coeff.max() < 2.0**52
    return np.ascontiguousarray(distinct[ids]), digits.astype(np.uint64), distinct[:-1], [int(v) for v in coeff]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("kind", M.BOUNDARY_KINDS)
def test_msm_buckets_at_the_run_boundaries(ctx, orc, pool, kind, g2):
    """Buckets of T - 1, T, T + 1, 2 T and 2 T + 1 finite entries, and the events at a run's edge that
    msm_plan_model.boundary_classes places under an order the sort decides.  In a bucket of T entries (one run): P + (-P), the doubling
    and an infinity at the last entry.  In a bucket of T + 1 entries (runs of even and odd length): an infinity as the last entry of
    the first run and as the first of the second; P + (-P) and the doubling at the last entry of the first run and a second run
    headed by minus the sum of its others, from buckets of T copies of one point and one multiple of it; P + (-P) at the last
    entry of the odd-length run; opposite and EQUAL run images (the doubling in the merge) with the second run headed by -P resp. P.
    Every counted event is expected 20 times (asserted, and in tests/test_msm_plan.py on the CPU).  T = 128 and 256 (whole buckets), a
    run_fill value (44 in G1 at c = 17, 36 in G2 at c = 16 at 256 compute units) and the plain 32; the plan record must show that T
    and that rule.  Scalars as they are and negated, both tail forms."""
    cu = device_cu(ctx, orc)
    T, c, n = M.boundary_setup(kind, g2, cu)
    assert len(M.boundary_expectations(T)) == 11 and min(M.boundary_expectations(T).values()) >= M.EXPECT
    points, digits, distinct, coeff = boundary_product(orc, pool, T, c, n, g2, 7900 + T)
    gpu, ref = (ctx.msm_g2, orc.msm_g2) if g2 else (ctx.msm_g1, orc.msm_g1)
    k = np.zeros((n, 4), np.uint64)
    k[:, 0] = digits
    kn = np.tile(R_LIMBS, (n, 1))
    kn[:, 0] -= digits                                             # r - d: the low limb of r exceeds every digit
    assert int(R_LIMBS[0]) > int(digits.max())
    want = ref(distinct, limbs(coeff))
    want_neg = ref(distinct, limbs([(R - v) % R for v in coeff]))
    branch = {128: M.WHOLE, 256: M.WHOLE, "fill": M.FILL, "plain": M.PLAIN}[kind]
    for quad in (0, 1 << 22):
        for scalars, expect, what in ((k, want, "as they are"), (kn, want_neg, "negated")):
            ctx.msm_plan_reset()
            with options(ctx, msm_quad_buckets=quad):
                got = gpu(points, scalars, c)
            want_plan = M.msm_plan(n, g2, cu, window_bits=c, quad_buckets=quad)
            assert (want_plan["run_len"], want_plan["run_branch"]) == (T, branch)
            assert_plans(ctx, [want_plan], (kind, g2, quad, what))
            assert np.array_equal(got, expect), (kind, g2, quad, what)
