"""The size-dependent choices of the inner products (csrc/msm_impl.hpp: msm_auto_window, msm_auto_window_g2, msm_run; csrc/crs.hip:
crs_ensure_tables; csrc/prove.hip: the order and sizes of a proof's products) restated in plain Python, as tests/test_digit_recoding.py
restates the recoding.  tests/test_msm_plan.py checks the restatement on the CPU; the GPU tests compare it with the record the library
keeps of every product (Context.msm_plans(): the "msm_plan" keys of zk_get_option, include/zkgpu_measure.h), field by field.

Nothing here is read by the library: a rule changed there must be changed here by hand, and the GPU tests say where."""
import numpy as np

RUN_MAX = 256            # msm_impl.hpp
RUN_ENTRIES = 32         # common.hpp: opt_run_entries
RUN_WHOLE = 128          # opt_run_whole
SMALL_LANES = 65536      # opt_small_lanes
UNCHAIN_LANES = 140000   # opt_unchain_lanes
QUAD_BUCKETS = 65536     # opt_quad_buckets
PLAIN, WHOLE, FILL, SMALL = 0, 1, 2, 3     # zkgpu_measure.h: ZK_MSM_RUN_*
BRANCH_NAMES = {PLAIN: "plain", WHOLE: "whole", FILL: "fill", SMALL: "small"}
PLAN_FIELDS = ("n_used", "g2", "groups", "c", "windows_owned", "buckets", "run_len", "run_branch", "quad_tail", "unchained", "cu_count")

# the planted slips of test_msm_plan.py: each names one comparison or constant of the rules below, altered
SLIPS = ("plus8_dropped", "whole_lt_128", "whole_le_64_is_lt", "fill_ge", "small_le", "unchain_le", "quad_lt", "g2_lanes_as_g1",
         "fill_round_down", "window_17_from_2p18")


def auto_window(n, slip=None):
    if n + (0 if slip == "plus8_dropped" else 8) >= 1 << 20:
        return 20
    lg = n.bit_length() - 1 if n else 0
    if lg >= (18 if slip == "window_17_from_2p18" else 17):
        return 17
    if lg >= 16:
        return 16
    if lg >= 14:
        return 15
    if lg >= 11:
        return 13
    return 8


def auto_window_g2(n, slip=None):
    return auto_window(n, slip)      # (the library states the 2^20 clause twice; the values are the same)


def windows(c):
    return 254 // c + 1


def plan(n_used, g2, c, cu, groups=1, quad_buckets=QUAD_BUCKETS, slip=None):
    """msm_run's decisions for one product of n_used scalars (all groups together) over a table of window size c: the fields of
    the plan record.  Unsharded: every window owned, no bucket ranges."""
    owned = windows(c)
    buckets = (1 << (c - 1)) * groups
    entries = owned * n_used
    per_bucket = entries // buckets
    lanes = (3 if (not g2 or slip == "g2_lanes_as_g1") else 2) * 256 * cu
    T = RUN_ENTRIES
    is_whole = (per_bucket < RUN_WHOLE if slip == "whole_lt_128" else per_bucket <= RUN_WHOLE) and buckets >= SMALL_LANES
    if is_whole:
        T = 128 if (per_bucket < 64 if slip == "whole_le_64_is_lt" else per_bucket <= 64) else RUN_MAX
        branch = WHOLE
    elif (entries // T >= lanes if slip == "fill_ge" else entries // T > lanes):
        T = min(RUN_MAX, (entries // lanes + (0 if slip == "fill_round_down" else 3)) & ~3)
        branch = FILL
    elif (entries // T <= SMALL_LANES if slip == "small_le" else entries // T < SMALL_LANES):
        T = max(4, min(T, entries // SMALL_LANES) & ~3)
        branch = SMALL
    else:
        branch = PLAIN
    max_runs = min(buckets, entries) + entries // T + 1
    lanes_est = min(max_runs, entries // min(T, 32) + 1)
    unchained = lanes_est <= UNCHAIN_LANES if slip == "unchain_le" else lanes_est < UNCHAIN_LANES
    quad = buckets < quad_buckets if slip == "quad_lt" else buckets <= quad_buckets
    return dict(n_used=n_used, g2=int(g2), groups=groups, c=c, windows_owned=owned, buckets=buckets, run_len=T, run_branch=branch,
                quad_tail=int(quad), unchained=int(unchained), cu_count=cu)


def msm_plan(n, g2, cu, window_bits=0, quad_buckets=QUAD_BUCKETS, slip=None):
    """zk_msm_g1 / zk_msm_g2 over n points (msm_host): the table is built over exactly these points"""
    c = window_bits or (auto_window_g2(n, slip) if g2 else auto_window(n, slip))
    return plan(n, g2, c, cu, quad_buckets=quad_buckets, slip=slip)


def table_points(n, m, l, integers=False):
    """(A, B, merged) points of a CRS's three tables (crs_ensure_tables): xi, xi in G2, and xi_t | xi | sum_delta -- xi_t has n - 1
    points, padded to n in the bit-reversed order the roots-of-unity form uses"""
    nl = m - l - 1
    return n, n, (n - 1 if integers else n) + n + nl


def proof_plans(n, m, l, cu, integers=False, merge_lh=True, witness_len=None, slip=None):
    """the products of one zk_prove in the order the host enqueues them (chain_order 1): A, B in G2, then the merged L + H product;
    with merge_lh = 0: L, A, B, H.  L and H take the merged table's window whether merged or not; a product without scalars is
    not recorded."""
    a_len = m if witness_len is None else min(witness_len, m)
    n_l = min(a_len - l - 1, m - l - 1) if a_len > l + 1 else 0
    n_h = 2 * n - 1 if integers else 2 * n
    pa, pb, plh = table_points(n, m, l, integers)
    ca, cb, clh = auto_window(pa, slip), auto_window_g2(pb, slip), auto_window(plh, slip)
    prods = [(n, False, ca), (n, True, cb)]
    if merge_lh:
        prods.append((n_h + n_l, False, clh))
    else:
        prods = [(n_l, False, clh)] + prods + [(n_h, False, clh)]
    return [plan(cnt, g2, c, cu, slip=slip) for cnt, g2, c in prods if cnt]


def batch_plans(n, m, l, count, cu, slip=None):
    """zk_prove_batch_submit over the roots of unity with merge_lh = 1: B in G2, A, the merged product; proof j is group j, a group
    as long as its table's scalars.  One proof takes the ungrouped call."""
    pa, pb, plh = table_points(n, m, l)
    ca, cb, clh = auto_window(pa, slip), auto_window_g2(pb, slip), auto_window(plh, slip)
    return [plan(cnt * count, g2, c, cu, groups=count, slip=slip) for cnt, g2, c in ((n, True, cb), (n, False, ca), (plh, False, clh))]


def batch_fits(n, m, l, count):
    """msm_run's size checks for a batch: the level-1 counters of all bins (4 bytes each) in 64 KiB of LDS, 2^24 buckets, 2^32
    digit records"""
    for pts, c in zip(table_points(n, m, l), (auto_window(n), auto_window_g2(n), auto_window(table_points(n, m, l)[2]))):
        sub_bits = min(11, max(0, c - 1 - 8))
        bins = (1 << (c - 1 - sub_bits)) * count
        if bins * 4 > 65536 or count << (c - 1) > 1 << 24 or windows(c) * pts * count >= 1 << 32:
            return False
    return True


def chain_dims(log_n):
    """(n, m, l) of the chain circuit (zksnark_rs_amd/circuits.py)"""
    n = 1 << log_n
    return n, 2 * n + 2, 2


def describe(p):
    return "%s c=%d %s T=%d %s %s" % ("G2" if p["g2"] else "G1", p["c"], BRANCH_NAMES[p["run_branch"]], p["run_len"],
                                      "quad" if p["quad_tail"] else "one-lane", "unchained" if p["unchained"] else "chained")


# ---- the sizes the GPU tests run at, derived from the rules --------------------------------------------------------------------
LADDER = tuple(range(0, 22))                 # tests/test_gpu_size_ladder.py: every log_n
NEW_SIZES = (7, 15, 17, 18, 19, 21)          # proven by no other test
BATCHES = ((4, 64), (16, 64), (10, 17))      # (log_n, proofs)


def first_n(pred, lo, hi):
    """the smallest n in (lo, hi] with pred(n), pred monotone and false at lo, true at hi"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def whole_end(c):
    """the first n no longer kept whole at a window of c >= 17 bits (more than RUN_WHOLE entries per bucket): where the searches
    below stop, since beyond it run_fill may give any run length again"""
    return -(-(RUN_WHOLE + 1) * (1 << (c - 1)) // windows(c))


def whole_ranges(g2, c, cu):
    """(first n with 256-entry runs, first n no longer kept whole) of a stand-alone product at window size c >= 17"""
    top = whole_end(c)
    kept_128 = lambda n: (lambda p: p["run_branch"] == WHOLE and p["run_len"] == 128)(plan(n, g2, c, cu))
    n256 = first_n(lambda n: not kept_128(n), 1, top)
    nfill = first_n(lambda n: plan(n, g2, c, cu)["run_branch"] != WHOLE, n256 - 1, top)
    return n256, nfill


def band_17(g2, cu):
    """The stand-alone sizes for one group: n just below and just above each place where the run-length rule changes
    inside the c = 17 band (2^17 <= n < 2^20 - 8), the middle of the run_fill stretch, and both sides of the 2^20 - 8 clause.
    Returns (sizes, (first n with 256-entry runs, first n of the fill stretch))."""
    lo, hi = 1 << 17, (1 << 20) - 9
    assert msm_plan(lo - 1, g2, cu)["c"] == 16 and msm_plan(lo, g2, cu)["c"] == 17 == msm_plan(hi, g2, cu)["c"] and msm_plan(hi + 1, g2, cu)["c"] == 20
    n256, nfill = whole_ranges(g2, 17, cu)
    assert lo < n256 < nfill < hi
    return [n256 - 1, n256, nfill - 1, nfill, (nfill + hi) // 2, hi, hi + 1], (n256, nfill)


def stand_alone_sizes(cu):
    return sorted(set(band_17(False, cu)[0]) | set(band_17(True, cu)[0]))


# ---- buckets at the run boundaries ---------------------------------------------------------------------------------------
def run_bounds(z, T):
    """k_msm_runs_emit: a bucket of z entries is cut into r = ceil(z / T) runs, run j = entries [z j / r, z (j + 1) / r)"""
    r = (z + T - 1) // T
    return [(z * j // r, z * (j + 1) // r) for j in range(r)]


EXPECT = 20                                   # an event counted on is expected at least this often at the wanted position
PLAIN_BUCKETS = 6                             # finite buckets of each plain size
POOL = 4096


def boundary_classes(T):
    """The bucket classes of the boundary construction for run length T: (name, entries, finite entries, buckets).

    What the sort leaves open is the ORDER of a bucket's entries, and the construction permutes the scalar array, so every order
    is equally likely.  A bucket of T entries is one run; a bucket of T + 1 entries is two, of k = (T + 1) // 2 (even at these T) and
    T + 1 - k (odd) entries, and the sort also decides which entries share a run.  Classes and what they place:
      plain        z distinct pool points, z = T - 1, T, T + 1, 2 T, 2 T + 1: the cut itself.
      zero         z - 1 distinct pool points and minus their sum.  z = T: the run sums to infinity, so whatever the order the
                   accumulator in front of the last entry is minus that entry: P + (-P) at the last entry of EVERY such bucket.
                   z = T + 1: the two run images are opposite, P + (-P) in the merge.
      double       z - 1 distinct pool points and their sum: the doubling at the last entry when the sum comes last (1 / z at z = T).
      inf          z - 1 distinct pool points and ONE infinity: at any wanted position with probability 1 / z; at z = T + 1 the same
                   buckets serve the last entry of the first run and the first entry of the second.
      copies       T copies of ONE pool point Q and one special point S, T + 1 entries.  Whatever the order, the entries of a run
                   other than S are copies of Q, so their sum is known ahead of time -- the same-x events of a bucket of T + 1
                   entries, which distinct points cannot place:
        last-      S = -(k - 1) Q: when S is the last entry of the first run (1 / (T + 1)) the accumulator in front of it is
                   (k - 1) Q: P + (-P) at the last entry, inside the fast loop (the one Q + Q of entries 1 and 2 is the generic
                   second step's).
        last+      S = +(k - 1) Q: the doubling at the last entry of the first run, likewise.
        head-      S = -(T + 1 - k - 1) Q: when S heads the second run (1 / (T + 1)) it is minus the sum of the run's others.  And
                   whenever S falls into the second run at all ((T + 1 - k) / (T + 1)) that run sums to infinity: P + (-P) at the
                   last entry of a run of ODD length -- the buckets of T entries only have runs of even length.
      pair         {P, -P} or {P, P} and T - 1 infinities: with P in the first run and the other heading the second
                   (k / (T (T + 1))) the two run images are opposite resp. EQUAL -- the doubling in the merge."""
    k = run_bounds(T + 1, T)[0][1]
    out = []
    for z in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        out.append(("plain", z, z, PLAIN_BUCKETS))
    out.append(("zero", T, T, EXPECT))
    out.append(("double", T, T, EXPECT * T))
    out.append(("inf", T, T - 1, EXPECT * T))
    out.append(("zero", T + 1, T + 1, EXPECT))
    out.append(("double", T + 1, T + 1, EXPECT))
    out.append(("inf", T + 1, T, EXPECT * (T + 1)))
    for name in ("copies last-", "copies last+", "copies head-"):
        out.append((name, T + 1, T + 1, EXPECT * (T + 1)))
    for name in ("pair opposite", "pair same"):
        out.append((name, T + 1, 2, -(-EXPECT * T * (T + 1) // k)))
    return out


def copies_multiplier(name, T):
    """S = multiplier * Q of a 'copies' bucket"""
    k = run_bounds(T + 1, T)[0][1]
    return {"copies last-": -(k - 1), "copies last+": k - 1, "copies head-": -(T + 1 - k - 1)}[name]


def boundary_expectations(T):
    """expected number of buckets in which each counted event sits at the wanted position, under uniformly random order"""
    k = run_bounds(T + 1, T)[0][1]
    assert len(run_bounds(T + 1, T)) == 2 and len(run_bounds(T, T)) == 1 and k % 2 == 0 and (T + 1 - k) % 2 == 1
    exp = {}
    for name, z, finite, count in boundary_classes(T):
        if name == "zero" and z == T:
            exp["opposite at the last entry of a run of T"] = float(count)              # every order
        elif name == "double" and z == T:
            exp["doubling at the last entry of a run of T"] = count / z
        elif name == "inf" and z == T:
            exp["infinity at the last entry of a run of T"] = count / z
        elif name == "inf":
            exp["infinity last of the first run of T + 1"] = count / z
            exp["infinity first of the second run of T + 1"] = count / z
        elif name == "copies last-":
            exp["opposite at the last entry of the first run of T + 1"] = count / z
        elif name == "copies last+":
            exp["doubling at the last entry of the first run of T + 1"] = count / z
        elif name == "copies head-":
            exp["minus the others heads the second run of T + 1"] = count / z
            exp["opposite at the last entry of a run of odd length"] = count * (z - k) / z
        elif name == "pair opposite":
            exp["opposite run images, -P heads the second run"] = count * k / (T * z)
        elif name == "pair same":
            exp["equal run images, P heads the second run"] = count * k / (T * z)
    return exp


def boundary_entries(T):
    return sum(z * count for _, z, _, count in boundary_classes(T))


def boundary_setup(kind, g2, cu):
    """(T, c, n) for the boundary construction.  kind 128 / 256: the smallest window from 17 on at which a product that holds the
    construction is kept whole with that run length, and the smallest such n.  'fill': the first window of 17, 16, 15, 14 bits and the smallest
    32 < T < 256 at which the sizes with that run_fill value hold the construction.  'plain': the smallest window with room for the buckets and the smallest n at which
    msm_run_entries stands as it is (T = 32)."""
    if kind == "fill":
        # T grows with n and the construction with T^2: the first (window, T) whose stretch of n holds the construction
        for c in (17, 16, 15, 14):
            start = whole_end(c) if c >= 17 else first_n(lambda n: plan(n, g2, c, cu)["run_branch"] == FILL, 1, 1 << 27)
            for T in range(RUN_ENTRIES + 4, RUN_MAX, 4):
                if sum(cl[3] for cl in boundary_classes(T)) + 64 > 1 << (c - 1) or plan(start, g2, c, cu)["run_len"] > T:
                    continue
                at = start if plan(start, g2, c, cu)["run_len"] == T else first_n(lambda n: plan(n, g2, c, cu)["run_len"] >= T, start, 1 << 27)
                n = max(boundary_entries(T), at)
                p = plan(n, g2, c, cu)
                if p["run_branch"] == FILL and p["run_len"] == T:
                    return T, c, n
        raise AssertionError("no window holds a run_fill construction")
    T = RUN_ENTRIES if kind == "plain" else kind
    need, room = boundary_entries(T), sum(cl[3] for cl in boundary_classes(T)) + 64
    for c in range(10 if kind == "plain" else 17, 23):
        if room > 1 << (c - 1):
            continue
        if kind == "plain":
            n = max(need, first_n(lambda n: plan(n, g2, c, cu)["run_branch"] != SMALL, 1, 1 << 27))
            if plan(n, g2, c, cu)["run_branch"] == PLAIN:
                return T, c, n
            continue
        n256, nfill = whole_ranges(g2, c, cu)
        lo, hi = (1, n256 - 1) if kind == 128 else (n256, nfill - 1)
        n = max(lo, need)
        if n <= hi:
            p = plan(n, g2, c, cu)
            assert p["run_branch"] == WHOLE and p["run_len"] == kind
            return T, c, n
    raise AssertionError("no window holds %d entries at T = %d" % (need, T))


BOUNDARY_KINDS = (128, 256, "fill", "plain")
INTEGER_SIZES = ("band", 1 << 18)             # integer-roots proofs: the first size of the run_fill band, and 2^18


def integer_sizes(cu):
    return [max(band_17(False, cu)[1][1], band_17(True, cu)[1][1]) if x == "band" else x for x in INTEGER_SIZES]


EDGE_WINDOW = 13


def edge_sizes(cu):
    """Three thresholds no automatic window puts a proof or a band size on, reached by stand-alone products at an explicit window
    of 13 bits: (n, g2) on both sides of the first product whose runs of 32 fill msm_small_lanes lanes (small -> plain), of the first
    with more runs of 32 than the chip has lanes (plain -> fill), and of the first product that is chained."""
    out = []
    for g2 in (False, True):
        np_ = first_n(lambda n: plan(n, g2, EDGE_WINDOW, cu)["run_branch"] != SMALL, 1, 1 << 24)
        nf = first_n(lambda n: plan(n, g2, EDGE_WINDOW, cu)["run_branch"] == FILL, 1, 1 << 24)
        nc = first_n(lambda n: not plan(n, g2, EDGE_WINDOW, cu)["unchained"], 1, 1 << 24)
        out += [(np_ - 1, g2), (np_, g2), (nf - 1, g2), (nf, g2), (nc - 1, g2), (nc, g2)]
    return out


def chosen_products(cu, slip=None):
    """(label, plan) of every product the GPU tests of the size ladder, the stand-alone sizes and the boundary constructions run
    -- with the SIZES chosen by the rules as they stand and the plans evaluated with `slip` planted"""
    out = []
    for log_n in LADDER:
        n, m, l = chain_dims(log_n)
        for merge in (True, False) if log_n in NEW_SIZES else (True,):
            out += [(("ladder", log_n, merge, i), p) for i, p in enumerate(proof_plans(n, m, l, cu, merge_lh=merge, slip=slip))]
    for n in integer_sizes(cu):
        out += [(("integers", n, i), p) for i, p in enumerate(proof_plans(n, 2 * n + 2, 2, cu, integers=True, slip=slip))]
    for log_n, count in BATCHES:
        n, m, l = chain_dims(log_n)
        out += [(("batch", log_n, count, i), p) for i, p in enumerate(batch_plans(n, m, l, count, cu, slip=slip))]
    for n in stand_alone_sizes(cu):
        for g2 in (False, True):
            for quad in (0, 1 << 22):
                out.append((("msm", n, g2, quad), msm_plan(n, g2, cu, quad_buckets=quad, slip=slip)))
    for n, g2 in edge_sizes(cu):
        out.append((("edge", n, g2), msm_plan(n, g2, cu, window_bits=EDGE_WINDOW, slip=slip)))
    for kind in BOUNDARY_KINDS:
        for g2 in (False, True):
            T, c, n = boundary_setup(kind, g2, cu)
            for quad in (0, 1 << 22):
                out.append((("boundary", kind, g2, quad), msm_plan(n, g2, cu, window_bits=c, quad_buckets=quad, slip=slip)))
    return out



# ---- what the GPU tests share -------------------------------------------------------------------------------------------------------
def limbs(values):
    """(len, 4) uint64 limbs of a list of integers below 2^256: ints_to_limbs for millions of values"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def device_cu(ctx, orc):
    """the compute-unit count the library plans with: read off the record of a one-point product"""
    ctx.msm_plan_reset()
    ctx.msm_g1(orc.enc_base_g1()[None, :], limbs([1]))
    return ctx.msm_plans()[0]["cu_count"]


def assert_plans(ctx, want, what):
    """the record since the last reset == the restated plans, product by product; empties the record"""
    got = ctx.msm_plans()
    ctx.msm_plan_reset()
    assert len(got) == len(want), (what, [describe(p) for p in got], [describe(p) for p in want])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, i, g, w)
