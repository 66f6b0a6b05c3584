"""-m gpu: circuits shaped like real R1CS instances (tests/test_circuit_shapes.py) and the MSM paths they take, against the CPU oracle.

What the chain circuit and random_sparse_rows reach only by chance or not at all:
  k_spmv      rows of 63 .. 4096 entries: the lazy sum is reduced every 64 included entries (never reached by the older rows), and the
              witness length cuts a long row just before, at and after such a reduction;
  G1 / G2     table entries at infinity at every position of a run of the accumulation's fast loop, behind same-x events, whole runs
              of infinity, runs that sum to infinity through P + (-P) beside finite runs of the same bucket, a bucket of more than 96 runs;
  proofs      sum_delta with a quarter of its points at infinity -- all of the last rank's share at world 4 -- and sum_gamma points at
              infinity, through every form of the prover, every form of the CRS container and zk_verify.
All checks are bit-exact.
"""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ints_to_limbs, limbs_to_ints, R_MODULUS as R
from test_circuit_shapes import (COMPOSITIONS, HALF, SIZES, composition_expectations, default_m, infinities, per_cell,
                                 shaped_circuit)

pytestmark = pytest.mark.gpu
L = 40
RANGE = -6


@pytest.fixture(scope="module")
def shapes():
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = shaped_circuit(n, default_m(n, L), L, 100 + n)
        return cache[n]
    return get


class options:
    """set context options for a block and restore what they were"""
    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        self.old = {k: self.ctx.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)


# ---- B. k_spmv alone -------------------------------------------------------------------------------------------------------
def _gate_sums(rows, n, vals, a_len):
    acc = [0] * n
    for g in range(n):
        acc[g] = sum(a * vals[x] for x, a in rows[g] if x < a_len) % R
    return ints_to_limbs(acc).reshape(n, 4)


@pytest.mark.parametrize("roots", ["unity", "integers"])
def test_spmv_wide_rows(ctx, shapes, roots):
    """k_spmv (zk_qap_weighted_sum) on the shaped rows of 2^10 gates == the sum over each gate's entries in Python integers, for the
    satisfying witness, all r - 1, all (r - 1) / 2, all zero and uniform values; and for witnesses cut so that the 1000-entry row keeps
    63, 64, 65, 127, 128, 129, 191 and 192 entries (the lazy sum is reduced after every 64th included entry)."""
    c = shapes(1 << 10)
    n, m = c["n"], c["m"]
    qap = ctx.qap_sparse(10, m, L, c["u"], c["v"], c["w"]) if roots == "unity" else ctx.qap_sparse_integers(n, m, L, c["u"], c["v"], c["w"])
    rng = np.random.default_rng(5)
    uniform = limbs_to_ints(rng.integers(0, 1 << 64, size=(m, 4), dtype=np.uint64))
    uniform = [x % R for x in uniform]
    wits = {"satisfying": c["values"], "r-1": [R - 1] * m, "half": [HALF] * m, "zero": [0] * m, "uniform": uniform}
    for name, vals in wits.items():
        wts = ints_to_limbs(vals)
        for which, rows in enumerate((c["gate_u"], c["gate_v"])):
            assert np.array_equal(ctx.qap_weighted_sum(qap, wts, which), _gate_sums(rows, n, vals, m)), (roots, name, which)
    g = [g for g, w in c["wide"].items() if w == 1000][0]
    wires = sorted(x for x, _ in c["gate_u"][g])
    assert len(set(wires)) == len(wires)
    for keep in (63, 64, 65, 127, 128, 129, 191, 192):
        a_len = wires[keep - 1] + 1                         # entries of wires < a_len: exactly `keep` of this row
        for vals in (uniform, [R - 1] * m):
            wts = ints_to_limbs(vals[:a_len])
            for which, rows in enumerate((c["gate_u"], c["gate_v"])):
                assert np.array_equal(ctx.qap_weighted_sum(qap, wts, which), _gate_sums(rows, n, vals, a_len)), (roots, keep, which)


# ---- C. the accumulation with infinity entries ------------------------------------------------------------------------------
def _point_pool(orc, seed, count):
    """count distinct G1 and G2 points: sums of two random pools of 128"""
    rng = SplitMix64(seed)
    k = ints_to_limbs([rng.fr() for _ in range(512)])
    a1 = orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (256, 1)), k[:256])
    a2 = orc.g2_mul_batch(np.tile(orc.enc_base_g2(), (256, 1)), k[256:])
    i = np.arange(count)
    lo, hi = i % 128, 128 + (i // 128) % 128
    assert count <= 128 * 128
    return orc.g1_add_batch(a1[lo], a1[hi]), orc.g2_add_batch(a2[lo], a2[hi])


def _neg(orc, p1, p2):
    minus1 = np.tile(ints_to_limbs([R - 1]), (len(p1), 1))
    return orc.g1_mul_batch(p1, minus1), orc.g2_mul_batch(p2, minus1)


class Buckets:
    """entries of single-digit buckets: bucket d (scalar d) gets the listed G1 / G2 points"""
    def __init__(self, orc, seed, finite):
        self.orc = orc
        self.f1, self.f2 = _point_pool(orc, seed, finite)
        self.next = 0
        self.p1, self.p2, self.d = [], [], []

    def take(self, count):
        a, b = self.f1[self.next:self.next + count], self.f2[self.next:self.next + count]
        self.next += count
        assert len(a) == count
        return list(a), list(b)

    def add(self, d, pts1, pts2, infs):
        self.p1 += pts1 + [np.zeros(8, np.uint64)] * infs
        self.p2 += pts2 + [np.zeros(16, np.uint64)] * infs
        self.d += [d] * (len(pts1) + infs)

    def arrays(self, seed):
        order = np.random.default_rng(seed).permutation(len(self.d))  # a bucket's entries come from all over the scalar array
        p1 = np.ascontiguousarray(np.array(self.p1, np.uint64)[order])
        p2 = np.ascontiguousarray(np.array(self.p2, np.uint64)[order])
        return p1, p2, [self.d[i] for i in order]


def _single_run_buckets(orc):
    cells = [(name, k, per_cell(name)) for name, _ in COMPOSITIONS for k in SIZES]
    finite = sum(cnt * {"opposite-quad": 3, "same-quad": 3, "pair-opposite": 1, "pair-same": 1}.get(name, k - infinities(name, k))
                 for name, k, cnt in cells)
    bk = Buckets(orc, 61, finite)
    d = 0
    quads = []
    for name, k, cnt in cells:
        j = infinities(name, k)
        for _ in range(cnt):
            d += 1
            if name.endswith("quad"):
                quads.append((d, name, j) + tuple(bk.take(3)))
            elif name.startswith("pair"):
                (a1,), (a2,) = bk.take(1)
                if name == "pair-same":
                    bk.add(d, [a1, a1], [a2, a2], j)
                else:
                    n1, n2 = _neg(orc, a1[None, :], a2[None, :])
                    bk.add(d, [a1, n1[0]], [a2, n2[0]], j)
            else:
                a1, a2 = bk.take(k - j)
                bk.add(d, a1, a2, j)
    # the fourth point of every quad: -(A + B + D) or A + B + D
    A1 = np.array([q[3] for q in quads], np.uint64)
    A2 = np.array([q[4] for q in quads], np.uint64)
    s1 = orc.g1_add_batch(orc.g1_add_batch(A1[:, 0], A1[:, 1]), A1[:, 2])
    s2 = orc.g2_add_batch(orc.g2_add_batch(A2[:, 0], A2[:, 1]), A2[:, 2])
    n1, n2 = _neg(orc, s1, s2)
    for i, (d, name, j, a1, a2) in enumerate(quads):
        f1, f2 = (n1[i], n2[i]) if name == "opposite-quad" else (s1[i], s2[i])
        bk.add(d, list(a1) + [f1], list(a2) + [f2], j)
    return bk, d


def _check_msm(ctx, orc, p1, p2, digits, c, g2=True):
    k = ints_to_limbs(digits)
    kn = ints_to_limbs([R - x for x in digits])
    assert np.array_equal(ctx.msm_g1(p1, k, c), orc.msm_g1(p1, k, 0)), ("G1", c)
    assert np.array_equal(ctx.msm_g1(p1, kn, c), orc.msm_g1(p1, kn, 10)), ("G1 negated", c)
    if g2:
        assert np.array_equal(ctx.msm_g2(p2, k, c), orc.msm_g2(p2, k, 0)), ("G2", c)
        assert np.array_equal(ctx.msm_g2(p2, kn, c), orc.msm_g2(p2, kn, 10)), ("G2 negated", c)


def test_msm_infinity_inside_single_runs(ctx, orc):
    """Buckets of 5 .. 12 entries, each ONE run at c = 17 (2^16 buckets and few entries per bucket: msm_run keeps whole buckets), that mix finite points with 1, 2, k - 2
    and k - 1 infinities, and buckets where infinities surround the same-x events: {A, B, D, -(A+B+D)} (P + (-P) at the fourth finite
    entry), {A, B, D, A+B+D} (doubling when the sum comes last), {P, -P} and {P, P}.  Scalar d < 2^(c-1) puts exactly bucket d's points
    in bucket d of window 0.  The order of a bucket's entries is the sort's (LDS atomics): under uniformly random order the model of
    tests/test_circuit_shapes.py expects the fast loop to leave at an infinity at position 3, 4, .., 10 (even half at odd positions,
    odd half at even ones) in 549, 232, 155, 101, 78, 59, 44, 30 buckets; the leaving infinity to be followed by another in 375, to be
    the run's last entry in 114, and an infinity right behind a same-x event in 49 (all >= 20, asserted).  Every case also with the
    scalars negated, in both tail forms, at c = 13 as well (runs of 4 entries: a small product's short runs), G2 alongside, and the LDS
    form of G1."""
    tot = composition_expectations()
    assert all(tot[("exit", p)] >= 20 for p in range(3, 11)) and min(tot[("consecutive",)], tot[("last",)], tot[("ev_inf",)]) >= 20
    bk, buckets = _single_run_buckets(orc)
    p1, p2, digits = bk.arrays(13)
    for c in (17, 13):
        assert buckets <= 1 << (c - 1)
        for quad in (0, 1 << 22):
            with options(ctx, msm_quad_buckets=quad):
                _check_msm(ctx, orc, p1, p2, digits, c)
    lds = [(x - 1) % 512 + 1 for x in digits]              # LDS comparator: 512 buckets at c = 10 (several compositions per bucket)
    k = ints_to_limbs(lds)
    assert np.array_equal(ctx.msm_g1(p1, k, -10), orc.msm_g1(p1, k, 0))
    kn = ints_to_limbs([R - x for x in lds])
    assert np.array_equal(ctx.msm_g1(p1, kn, -10), orc.msm_g1(p1, kn, 10))


def test_msm_infinity_across_runs(ctx, orc):
    """Buckets cut into runs of 32 entries, whose run images are merged.  msm_run cuts the buckets of a product of 2.1 .. 6.3 M digits at
    32 entries (fewer: shorter runs; more: as long as one round of lanes allows): 110000 scalars at c = 12, 21 windows; the entries
    beyond the buckets below are infinity points in the buckets 200 .. 2047.
      40 buckets of 160 entries, 4 finite: under uniform order ~81 runs hold no finite point at all (images at infinity, cleared);
      120 buckets of 64 entries {P, -P, A} + 61 infinities: in ~30 of them P and -P share a run without A -- a run image at infinity
          through P + (-P) beside the finite run of A in the same bucket;
      one bucket of 3200 entries (100 runs: more than 96, the k_msm_merge_heavy path) with 16 finite points and 8 pairs {P, -P}.
    Both tail forms (k_msm_merge and the four-lane merge), every case also with negated scalars, G2 alongside."""
    bk = Buckets(orc, 62, 40 * 4 + 120 * 2 + 16 + 8)
    d = 0
    for _ in range(40):
        d += 1
        a1, a2 = bk.take(4)
        bk.add(d, a1, a2, 156)
    for _ in range(120):
        d += 1
        (a1, b1), (a2, b2) = bk.take(2)
        n1, n2 = _neg(orc, b1[None, :], b2[None, :])
        bk.add(d, [a1, b1, n1[0]], [a2, b2, n2[0]], 61)
    d += 1
    a1, a2 = bk.take(16)
    b1, b2 = bk.take(8)
    n1, n2 = _neg(orc, np.array(b1), np.array(b2))
    bk.add(d, a1 + b1 + list(n1), a2 + b2 + list(n2), 3200 - 32)
    filler = 110000 - len(bk.d)
    bk.p1 += [np.zeros(8, np.uint64)] * filler
    bk.p2 += [np.zeros(16, np.uint64)] * filler
    bk.d += [200 + i % 1848 for i in range(filler)]
    p1, p2, digits = bk.arrays(14)
    for quad in (0, 1 << 22):
        with options(ctx, msm_quad_buckets=quad):
            _check_msm(ctx, orc, p1, p2, digits, 12)


# ---- D. proofs of the shaped circuit -----------------------------------------------------------------------------------------
def _instance(ctx, c, seed, roots="unity"):
    n, m = c["n"], c["m"]
    rng = SplitMix64(seed)
    td = ints_to_limbs([rng.fr() for _ in range(5)])
    r, s = rng.fr(), rng.fr()
    if roots == "unity":
        log_n = n.bit_length() - 1
        desc = ctx.sparse_desc(log_n, m, L, c["u"], c["v"], c["w"])
        qap = ctx.qap_sparse(log_n, m, L, c["u"], c["v"], c["w"])
    else:
        desc = ctx.sparse_desc(0, m, L, c["u"], c["v"], c["w"])
        qap = ctx.qap_sparse_integers(n, m, L, c["u"], c["v"], c["w"])
    crs = ctx.setup(qap, td)
    return dict(n=n, m=m, desc=desc, qap=qap, crs=crs, td=td, r=r, s=s, w=c["weights"])


def _other_unused_values(c, seed):
    """the same witness with different (non-zero) values on every unused wire: they multiply infinity points only"""
    w = c["weights"].copy()
    rng = np.random.default_rng(seed)
    idx = np.array(sorted(c["unused"]))
    w[idx] = rng.integers(1, 1 << 62, size=(len(idx), 4), dtype=np.uint64)
    w[idx, 3] >>= np.uint64(4)                                # < 2^58 in the top limb: below r
    return w


@pytest.mark.parametrize("log_n", [10, 16])
def test_shaped_proofs(ctx, orc, shapes, log_n):
    """2^10 and 2^16 gates: zk_prove == the trapdoor closed form (and at 2^10 the oracle's fast prover over the downloaded CRS), the
    proof verifies; other values on the unused wires give the same bytes; an altered used wire gives the closed form's bytes and fails
    verification; merge_lh 0 and 1; zk_prove_submit / zk_prove_wait with two in flight; a batch of three witnesses, one truncated."""
    torch = pytest.importorskip("torch")
    c = shapes(1 << log_n)
    I = _instance(ctx, c, 300 + log_n)
    crs, qap, desc, td, r, s, w, m = I["crs"], I["qap"], I["desc"], I["td"], I["r"], I["s"], I["w"], I["m"]
    want = orc.trapdoor_proof_sparse(desc, td, w, r, s)
    got = ctx.prove(crs, qap, w, r, s)
    assert got == want
    assert ctx.verify(crs, w[1:1 + L], got)
    if log_n == 10:
        cdesc = ctx.crs_desc(I["n"], m, L, ctx.crs_download(crs))
        assert got == orc.prove_sparse(desc, cdesc, w, r, s, False)
    w_other = _other_unused_values(c, log_n)
    assert ctx.prove(crs, qap, w_other, r, s) == got
    bad = w.copy()
    bad[c["outputs"][5], 0] ^= np.uint64(1)
    want_bad = orc.trapdoor_proof_sparse(desc, td, bad, r, s)
    assert ctx.prove(crs, qap, bad, r, s) == want_bad != want
    assert not ctx.verify(crs, bad[1:1 + L], want_bad)
    with options(ctx, merge_lh=0):
        assert ctx.prove(crs, qap, w, r, s) == got
        assert ctx.prove(crs, qap, bad, r, s) == want_bad
    # pipelined: two in flight
    want_sr = orc.trapdoor_proof_sparse(desc, td, w, s, r)
    dw = torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).cuda()
    torch.cuda.synchronize()
    t1 = ctx.prove_submit(crs, qap, dw.data_ptr(), m, r, s)
    t2 = ctx.prove_submit(crs, qap, dw.data_ptr(), m, s, r)
    assert ctx.prove_wait(t1) == got and ctx.prove_wait(t2) == want_sr
    # a batch of three witnesses: the satisfying one, an altered one, one truncated inside the used wires
    cut = c["block_start"] - 7
    wits = [w, bad, w[:cut]]
    rs, ss = [r, s, r], [s, r, r]
    want_b = [orc.trapdoor_proof_sparse(desc, td, x, a, b) for x, a, b in zip(wits, rs, ss)]
    dws = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda() for x in wits]
    torch.cuda.synchronize()
    for merge in (1, 0):
        with options(ctx, merge_lh=merge):
            t = ctx.prove_batch_submit(crs, qap, [x.data_ptr() for x in dws], [x.shape[0] for x in wits], rs, ss)
            assert ctx.prove_batch_wait(t, 3) == want_b, merge


@pytest.mark.parametrize("log_n", [10, 16])
def test_shaped_proofs_distributed(ctx, orc, shapes, log_n):
    """The three cuts of the tables over ranks, played rank by rank on one device: the scalar exchange at worlds 1, 2, 4 with rank
    tables (cut by point range: at world 4 the last rank's share of sum_delta is all infinity) and without; zk_prove_partial +
    zk_prove_combine by windows, point ranges and bucket ranges (msm_shard_points 0, 1, 2) at worlds 2, 4, 8.  == the closed form."""
    torch = pytest.importorskip("torch")
    c = shapes(1 << log_n)
    I = _instance(ctx, c, 400 + log_n)
    crs, qap, desc, td, r, s, w, m = I["crs"], I["qap"], I["desc"], I["td"], I["r"], I["s"], I["w"], I["m"]
    tail = m - L - 1 - (m - L - 1) * 3 // 4                   # the last quarter of sum_delta
    assert tail <= m - c["block_start"]
    w2 = w[:c["block_start"] + 5]                             # truncated inside the block of unused wires
    proofs = [(w, r, s), (w2, s, r)]
    want = [orc.trapdoor_proof_sparse(desc, td, x, a, b) for x, a, b in proofs]
    dws = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda() for x, _, _ in proofs]
    torch.cuda.synchronize()
    for world in (1, 2, 4, -2, -4):
        with options(ctx, rank_tables=0 if world < 0 else 1):
            world = abs(world)
            elems = ctx.prove_exchange_elems(qap, world)
            send = [[torch.zeros(32 * e, dtype=torch.uint8, device="cuda") for e in elems] for _ in proofs]
            for j, (x, a, b) in enumerate(proofs):
                t = ctx.prove_scalars_submit(crs, qap, dws[j].data_ptr(), x.shape[0], a, b, world, [y.data_ptr() for y in send[j]])
                ctx.prove_wait(t, partial=True)
            blobs = [[None] * world for _ in proofs]
            for g in range(world):
                recv = [torch.cat([send[j][k][g * (32 * e // world):(g + 1) * (32 * e // world)] for j in range(len(proofs))])
                        for k, e in enumerate(elems)]
                part = torch.zeros(len(proofs) * zk.PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
                t = ctx.prove_msm_submit(crs, qap, len(proofs), g, world, [y.data_ptr() for y in recv], part.data_ptr())
                ctx.prove_wait(t, partial=True)
                for j in range(len(proofs)):
                    blobs[j][g] = part[j * zk.PARTIAL_BYTES:(j + 1) * zk.PARTIAL_BYTES].clone()
            for j, (x, a, b) in enumerate(proofs):
                gathered = torch.cat(blobs[j])
                torch.cuda.synchronize()
                assert ctx.prove_combine(crs, gathered.data_ptr(), world, a, b) == want[j], (world, j, ctx.get_option("rank_tables"))
    for shard in (0, 1, 2):
        with options(ctx, msm_shard_points=shard):
            for world in (2, 4, 8):
                buf = torch.zeros(world * zk.PARTIAL_BYTES, dtype=torch.uint8, device="cuda")
                for rank in range(world):
                    ctx.prove_partial(crs, qap, dws[0].data_ptr(), m, r, s, rank, world, buf.data_ptr() + rank * zk.PARTIAL_BYTES)
                torch.cuda.synchronize()
                assert ctx.prove_combine(crs, buf.data_ptr(), world, r, s) == want[0], (shard, world)


def test_shaped_proofs_other_domains(ctx, orc, shapes):
    """The same rows over the integers 1..n (qap_sparse_integers: closed form trapdoor_proof_integers) and over the arbitrary roots
    a k + b, n = 1000 (the integer-roots proof with trapdoor x = (x' - b) / a, as tests/test_arbitrary_roots.py argues); both verify."""
    c = shapes(1 << 10)
    I = _instance(ctx, c, 500, roots="integers")
    got = ctx.prove(I["crs"], I["qap"], I["w"], I["r"], I["s"])
    assert got == orc.trapdoor_proof_integers(I["desc"], I["n"], I["td"], I["w"], I["r"], I["s"])
    assert ctx.verify(I["crs"], I["w"][1:1 + L], got)
    assert ctx.prove(I["crs"], I["qap"], _other_unused_values(c, 3), I["r"], I["s"]) == got
    n = 1000
    c = shapes(n)
    m, w = c["m"], c["weights"]
    rng = SplitMix64(501)
    a, b = rng.fr() | 1, rng.fr()
    roots = ints_to_limbs([(a * k + b) % R for k in range(1, n + 1)]).reshape(n, 4)
    td_ints = [rng.fr() for _ in range(5)]
    td_int = ints_to_limbs(td_ints[:4] + [(td_ints[4] - b) * pow(a, -1, R) % R])
    qap = ctx.qap_sparse_roots(roots, m, L, c["u"], c["v"], c["w"])
    crs = ctx.setup(qap, ints_to_limbs(td_ints))
    r, s = rng.fr(), rng.fr()
    desc = ctx.sparse_desc(0, m, L, c["u"], c["v"], c["w"])
    got = ctx.prove(crs, qap, w, r, s)
    assert got == orc.trapdoor_proof_integers(desc, n, td_int, w, r, s)
    assert ctx.verify(crs, w[1:1 + L], got)


# ---- E. containers and uploads with infinity points ---------------------------------------------------------------------------
def _fnv(payload):
    h = 0xcbf29ce484222325
    for byte in payload:
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shaped_crs_containers(ctx, orc, shapes, tmp_path):
    """The shaped CRS of 2^10 gates -- over the roots of unity (ZKCRSv1) and over the integers (ZKCRSv2, with the Lagrange-basis arrays)
    -- through crs_save -> crs_load and crs_download -> crs_upload: the same arrays (infinity stays all-zero, exactly at the unused
    wires), the same proof bytes.  An off-curve point next to an infinity entry of sum_delta is still refused, in a file and in an upload."""
    c = shapes(1 << 10)
    n, m = c["n"], c["m"]
    inf_delta = np.array(sorted(x - L - 1 for x in c["unused"] if x > L))
    inf_gamma = np.array(sorted(c["unread_public"]))
    for roots in ("unity", "integers"):
        I = _instance(ctx, c, 600, roots=roots)
        crs, qap, w, r, s = I["crs"], I["qap"], I["w"], I["r"], I["s"]
        want = ctx.prove(crs, qap, w, r, s)
        arrs = ctx.crs_download(crs)
        assert np.flatnonzero(~arrs["sum_delta_g1"].any(axis=1)).tolist() == inf_delta.tolist()
        assert np.flatnonzero(~arrs["sum_gamma_g1"].any(axis=1)).tolist() == inf_gamma.tolist()
        path = tmp_path / (roots + ".zkcrs")
        ctx.crs_save(crs, path)
        raw = path.read_bytes()
        assert raw[:8] == (b"ZKCRSv1\0" if roots == "unity" else b"ZKCRSv2\0")
        loaded = ctx.crs_load(path)
        uploaded = ctx.crs_upload(n, m, L, arrs)
        for other in (loaded, uploaded):
            got = ctx.crs_download(other)
            for k in arrs:
                assert np.array_equal(got[k], arrs[k]), (roots, k)
            assert ctx.prove(other, qap, w, r, s) == want, roots
            assert ctx.verify(other, w[1:1 + L], want)
        ctx.crs_save(loaded, tmp_path / "again.zkcrs")
        assert (tmp_path / "again.zkcrs").read_bytes() == raw
        # an off-curve point (x ^ 1) right behind an infinity entry of sum_delta
        i = int([x for x in inf_delta if x + 1 not in set(inf_delta.tolist())][0]) + 1
        assert arrs["sum_delta_g1"][i].any() and not arrs["sum_delta_g1"][i - 1].any()
        bad = {k: np.array(v, copy=True) for k, v in arrs.items()}
        bad["sum_delta_g1"][i, 0] ^= np.uint64(1)
        with pytest.raises(zk.ZkError) as e:
            ctx.crs_upload(n, m, L, bad)
        assert e.value.status == RANGE, roots
        off = 40 + 64 * (3 + n + L + 1 + i)
        assert raw[off:off + 64] == arrs["sum_delta_g1"][i].tobytes()
        flipped = bytearray(raw)
        flipped[off] ^= 1
        flipped[32:40] = _fnv(flipped[40:]).to_bytes(8, "little")
        (tmp_path / "bad.zkcrs").write_bytes(bytes(flipped))
        with pytest.raises(zk.ZkError) as e:
            ctx.crs_load(tmp_path / "bad.zkcrs")
        assert e.value.status == RANGE, roots
