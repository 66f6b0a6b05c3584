"""-m gpu: the MSM and the NTT at the edges random data does not reach, against the CPU oracle.

  MSM   every window size 2..22 through zk_msm_g1 / zk_msm_g2 (and the LDS comparator up to c = 10) on the scalars of
        tests/test_digit_recoding.py: the top bucket in every window, the first negative digit, carries through every window, the largest
        top-window digit, and their negations; both forms of the reduction tail; a heavy top bucket at the product's own window sizes
        17 and 20; and a proof whose private witness is that scalar set.
  NTT   zk_ntt_fr at every size 2^0 .. 2^23 -- the two-pass split of 2^17 .. 2^22 included -- forward and inverse, plain and coset, on
        uniform values over all of [0, r), all r - 1, alternating r - 1 / 0, r - 1 at the ends only, and the same with (r - 1) / 2.
"""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs, R_MODULUS as R
from test_digit_recoding import recoding_cases, windows

pytestmark = pytest.mark.gpu

POOL = 512        # distinct random points; products of more scalars repeat them (equal points in one bucket: doublings)


@pytest.fixture(scope="module")
def pool(orc):
    rng = SplitMix64(4096)
    k = ints_to_limbs([rng.fr() for _ in range(2 * POOL)])
    p1 = orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (POOL, 1)), k[:POOL])
    p2 = orc.g2_mul_batch(np.tile(orc.enc_base_g2(), (POOL, 1)), k[POOL:])
    return p1, p2


def _points(pool, n):
    reps = -(-n // POOL)
    return np.ascontiguousarray(np.tile(pool[0], (reps, 1))[:n]), np.ascontiguousarray(np.tile(pool[1], (reps, 1))[:n])


def _both_tails(ctx, fn):
    """fn() under the one-lane tail (msm_quad_buckets 0) and the four-lane tail (every inner product); the option is restored"""
    prev = ctx.get_option("msm_quad_buckets")
    try:
        for quad in (0, 1 << 22):
            ctx.set_option("msm_quad_buckets", quad)
            fn(quad)
    finally:
        ctx.set_option("msm_quad_buckets", prev)
    assert ctx.get_option("msm_quad_buckets") == prev


@pytest.mark.parametrize("c", list(range(2, 23)))
def test_msm_digit_edges_every_window_size(ctx, orc, pool, c):
    """zk_msm_g1 / g2 at window_bits = c on the recoding edge set (padded to 256 scalars with random ones), then on its negation
    (r - k: negative top buckets, carries of the complement) == the oracle's folded double-and-add; c <= 10 also in the LDS form"""
    rng = SplitMix64(7700 + c)
    ks = recoding_cases(c)
    ks = ks + [rng.fr() for _ in range(max(0, 256 - len(ks)))]
    order = np.random.default_rng(c).permutation(len(ks))          # edge scalars spread over the array, not in one chunk
    ks = [ks[i] for i in order]
    p1, p2 = _points(pool, len(ks))
    for sign, sc in (("+", ks), ("-", [(R - k) % R for k in ks])):
        k = ints_to_limbs(sc)
        want1, want2 = orc.msm_g1(p1, k, 0), orc.msm_g2(p2, k, 0)

        def check(quad):
            assert np.array_equal(ctx.msm_g1(p1, k, c), want1), (c, sign, quad)
            assert np.array_equal(ctx.msm_g2(p2, k, c), want2), (c, sign, quad)
        _both_tails(ctx, check)
        if c <= 10:
            assert np.array_equal(ctx.msm_g1(p1, k, -c), want1), (c, sign, "lds")


@pytest.mark.parametrize("c", [17, 20])
def test_msm_heavy_top_bucket(ctx, orc, pool, c):
    """1024 entries with digit +2^(c-1) in one window (the last bucket, last bin and last sub-bucket of the sort, cut into many runs and
    summed by the heavy merge), next to the edge set, at the two window sizes the product instantiates (digit_step_c<17 / 20>)"""
    half = 1 << (c - 1)
    for w in (0, 3, windows(c) - 2):
        ks = [half << (c * w)] * 1024 + recoding_cases(c)
        order = np.random.default_rng(c + w).permutation(len(ks))
        k = ints_to_limbs([ks[i] for i in order])
        p1, p2 = _points(pool, len(ks))
        want1, want2 = orc.msm_g1(p1, k, 0), orc.msm_g2(p2, k, 0)

        def check(quad):
            assert np.array_equal(ctx.msm_g1(p1, k, c), want1), (c, w, quad)
            assert np.array_equal(ctx.msm_g2(p2, k, c), want2), (c, w, quad)
        _both_tails(ctx, check)


def _random_rows(rng, n, m, density):
    ptr, gates, vals = [0], [], []
    for _ in range(m):
        gs = sorted({int(rng.next() % n) for _ in range(rng.next() % (density + 1))})
        gates += gs
        vals += [rng.fr() for _ in gs]
        ptr.append(len(gates))
    return np.array(ptr, np.uint64), np.array(gates, np.uint32), ints_to_limbs(vals) if vals else np.zeros((0, 4), np.uint64)


@pytest.mark.parametrize("c", [17, 20])
def test_prove_private_witness_at_the_digit_edges(ctx, orc, c):
    """The private witness a_{l+1 .. m-1} is the scalar vector over sum_delta in the merged L + H product, unchanged: a 2^10-gate sparse
    QAP whose private witness is the recoding edge set of c (and its negation), proven at msm_window_bits = c with merge_lh on and off,
    == the oracle's fast prover byte for byte"""
    log_n, l = 10, 2
    cases = recoding_cases(c)
    m = 1 + l + len(cases)
    rng = SplitMix64(9100 + c)
    u, v, w = (_random_rows(rng, 1 << log_n, m, 3) for _ in range(3))
    desc = ctx.sparse_desc(log_n, m, l, u, v, w)
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    cdesc = ctx.crs_desc(1 << log_n, m, l, ctx.crs_download(crs))
    r, s = rng.fr(), rng.fr()
    public = [rng.fr() for _ in range(l)]
    wits = [ints_to_limbs([1] + public + cases), ints_to_limbs([1] + public + [(R - k) % R for k in cases])]
    wants = [orc.prove_sparse(desc, cdesc, wt, r, s, False) for wt in wits]
    prev_c, prev_merge = ctx.get_option("msm_window_bits"), ctx.get_option("merge_lh")
    try:
        ctx.set_option("msm_window_bits", c)
        for merge in (1, 0):
            ctx.set_option("merge_lh", merge)
            for i, (wt, want) in enumerate(zip(wits, wants)):
                assert ctx.prove(crs, qap, wt, r, s) == want, (c, merge, i)
    finally:
        ctx.set_option("msm_window_bits", prev_c)
        ctx.set_option("merge_lh", prev_merge)
    assert ctx.get_option("msm_window_bits") == prev_c and ctx.get_option("merge_lh") == prev_merge


# ---- NTT ---------------------------------------------------------------------------------------------------------------------
R_LIMBS = np.array([(R >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], np.uint64)


def _below_r(a):
    """rows of (n, 4) little-endian limbs that are < r"""
    lt = np.zeros(a.shape[0], bool)
    eq = np.ones(a.shape[0], bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < R_LIMBS[i])
        eq &= a[:, i] == R_LIMBS[i]
    return lt


def uniform_fr(rng, n):
    """uniform over all of [0, r) (r > 2^253: a third of the values sit in [2^253, r), where fr_reduce's bounds are closest)"""
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 62) - 1)                     # < 2^254; about a quarter is >= r and drawn again
    bad = np.flatnonzero(~_below_r(a))
    while bad.size:
        b = rng.integers(0, 1 << 64, size=(bad.size, 4), dtype=np.uint64)
        b[:, 3] &= np.uint64((1 << 62) - 1)
        a[bad] = b
        bad = bad[~_below_r(b)]
    return a


TOP = {"r-1": R - 1, "(r-1)/2": (R - 1) // 2}
SHAPES = ("all", "alternating", "ends")


def structured(n, shape, top):
    a = np.zeros((n, 4), np.uint64)
    t = ints_to_limbs([TOP[top]])[0]
    if shape == "all":
        a[:] = t
    elif shape == "alternating":
        a[0::2] = t
    else:
        a[0] = t
        a[n - 1] = t
    return a


def ntt_input(log_n, name):
    n = 1 << log_n
    if name == "uniform":
        return uniform_fr(np.random.default_rng(500 + log_n), n)
    shape, top = name.split(":")
    return structured(n, shape, top)


_ORACLE = {}


def oracle_ntt(orc, log_n, name, inverse, coset):
    """the oracle's transform of a named input, computed once per module (kept up to 2^18 elements: 8 MiB each)"""
    key = (log_n, name, inverse, coset)
    if key in _ORACLE:
        return _ORACLE[key]
    f = orc.ntt_fr(ntt_input(log_n, name), inverse=inverse, coset=coset)
    if log_n <= 18:
        _ORACLE[key] = f
    return f


ALL_INPUTS = ["uniform"] + ["%s:%s" % (s, t) for t in TOP for s in SHAPES]


def ntt_plan(log_n):
    """(input, inverse, coset) triples: up to 2^18 every input in all four modes; above, one uniform and one structured input per
    direction (structured input, and which of the two is the coset transform, rotate with the size); 2^23 two structured transforms"""
    if log_n <= 18:
        return [(name, inv, cos) for name in ALL_INPUTS for inv in (False, True) for cos in (False, True)]
    s1, s2 = ALL_INPUTS[1 + log_n % 6], ALL_INPUTS[1 + (log_n + 3) % 6]
    if log_n == 23:                     # the uniform forward transforms at 2^23: test_gpu_blocks.test_ntt_three_passes
        return [(s1, False, True), (s2, True, False)]
    return [("uniform", False, log_n % 2 == 0), (s1, False, log_n % 2 == 1), ("uniform", True, log_n % 2 == 1), (s2, True, log_n % 2 == 0)]


@pytest.mark.parametrize("log_n", list(range(0, 24)))
def test_ntt_every_size_full_range(ctx, orc, log_n):
    """zk_ntt_fr == the oracle's NTT at every size, and the inverse of the GPU transform gives the input back; up to 2^8 also == the
    naive O(n^2) dft / idft"""
    for name, inverse, coset in ntt_plan(log_n):
        a = ntt_input(log_n, name)
        f = ctx.ntt_fr(a, inverse=inverse, coset=coset)
        assert np.array_equal(f, oracle_ntt(orc, log_n, name, inverse, coset)), (log_n, name, inverse, coset)
        assert np.array_equal(ctx.ntt_fr(f, inverse=not inverse, coset=coset), a), (log_n, name, inverse, coset, "round trip")
        if log_n <= 8 and not coset:
            assert np.array_equal(f, orc.dft_fr(a, orc.root_of_unity(log_n), inverse=inverse)), (log_n, name, inverse, "dft")


def test_ntt_inputs_are_what_they_say():
    """the NTT inputs themselves: canonical, and the uniform one really spans [2^253, r)"""
    a = uniform_fr(np.random.default_rng(1), 1 << 14)
    assert _below_r(a).all()
    assert (a[:, 3] >= np.uint64(1 << 61)).mean() > 0.15          # values >= 2^253
    assert zk.limbs_to_int(structured(4, "ends", "r-1")[3]) == R - 1
    assert not _below_r(ints_to_limbs([R, R + 1, (1 << 254) - 1]).reshape(-1, 4)).any()
    assert _below_r(ints_to_limbs([R - 1, 0, (R - 1) // 2]).reshape(-1, 4)).all()
