// crs_contribute.hip -- zk_g1_scale_batch, zk_crs_contribute and zk_crs_contribution_check.
//
// k_g1_scale: out[i] = k P[i] for ONE scalar k and a resident array of affine Montgomery points -- what a delta contribution does to
// sum_delta_g1, xi_t_g1 and lagS_t1 (k = 1 / d).  k_point_mul (field_kernels.hip) takes a scalar per lane: 254 doublings, ~127 general
// additions and an inversion per point; gb_mul (gbasis.hip) splits by the endomorphism but recodes and branches per lane.  With one
// scalar for the whole array everything that depends on the scalar is done ONCE, on the host (crs_contribution.hip scalar_recode):
//   k = k1 + k2 lambda, |k1|, |k2| < 2^128;  each half as a width-4 non-adjacent form, digits 0 or odd in [-7, 7], the half's sign
//   folded in: ~128 doublings and 2 x 128 / 5 ~ 52 mixed additions for every point.
// The digits are a kernel argument, so every branch on a digit is a scalar branch and all lanes of the array execute the same sequence;
// lanes part only where madd_lazy / dbl_lazy report the special cases (an infinity entry, an accumulator that meets its own table
// entry).
//   table      P, 3P, 5P, 7P per lane WITHOUT an inversion: D = 2P = (Xd : Yd : C) is an affine point (Xd, Yd) on the isomorphic curve
//              E': (x, y) -> (x C^2, y C^3) (a = 0: no formula contains b), where P is (x C^2, y C^3); three mixed additions of D give
//              3P, 5P, 7P with Z = H1, H1 H2, H1 H2 H3 (the H of each addition), all brought to the LAST entry's Z by the ratios H3,
//              H2 H3, Z7: (X r^2, Y r^3).  The loop then runs on the curve isomorphic by G = Z7 C with four AFFINE entries, and the
//              result's true Z is Z G.  (The table construction of libsecp256k1's ecmult: ~50 multiplications instead of ~400 for an
//              inversion.)  The phi images are formed where they are used: phi(x, y) = (beta x, y) commutes with the isomorphisms.
//   placement  the table lives in LDS, [entry][coordinate][limb][lane] (18 KiB per 64 lanes, conflict-free): a digit indexes it with
//              a scalar, where a register table would need a select per limb; the accumulator and the temporaries of lazy29.cuh's
//              formulas stay in VGPRs with no scratch (tools/kernel_resources.sh prints the compiler's figures; DESIGN 4l quotes them).
//   inversion  a lane owns SC_PPL points, block b the points [b SC_TILE, (b + 1) SC_TILE), lane t the points b SC_TILE + j SC_BLOCK
//              + t (coalesced).  Pass 1 leaves (X, Y) of point j in out[] and Z_j with the prefix product Z_0 .. Z_{j-1} in a side
//              buffer; ONE inversion (Fermat, constant time: Z depends on the secret scalar) of the lane's product; pass 2 peels
//              1 / Z_j off backwards.  An infinity result takes Z_j = 1 in the chain and is written as zeros.  Reads and writes of a
//              point are the owning lane's alone, so out may be the input.
// Limb bounds (lazy29.cuh's rules: a multiplier operand has |limb| < 2^29, one side may reach 2^30; `norm` restores [0, 2^29)):
//   dbl_lazy on a canonical load, madd_lazy and dbl_lazy on their own results are lazy29.cuh's own sequences (test_gpu_point_forms.py).
//   New here: D.X, D.Y (norm'ed, |value| < 13 p) are multiplied by R mod p once, which makes them Montgomery outputs in (-p/4, 1.3 p)
//   before they serve as the affine operand (x2, y2) of the three table additions; scale_madd is madd_lazy's general branch verbatim
//   and hands out H = U2 - X1 (a difference of two normal forms, norm'ed before it is squared or multiplied by another H); table
//   entries, G, the prefix products and the pass-2 products are products of Montgomery outputs or norm'ed values only.
#include <random>
#include "pipeline.hpp"
#include "pairing.cuh"
#include "lazy29.cuh"
#include "crs_contribution.hpp"

namespace zk {

constexpr int SC_BLOCK = 64;                  // lanes per work-group: one wave
constexpr int SC_PPL = 4;                     // points a lane owns (and inverts together)
constexpr int SC_TILE = SC_BLOCK * SC_PPL;    // points per work-group

typedef FpR<FqParams> ScL;

// madd_lazy's general branch (no special case can occur between P, 3P, 5P and 2P for a point of prime order r > 7), H handed out
__device__ __forceinline__ void scale_madd(JacR<Fq>& p, const ScL& qx, const ScL& qy, ScL& Hn) {
    ScL Z1Z1 = p.Z.sqr();
    ScL U2 = qx * Z1Z1;
    ScL S2 = (qy * p.Z) * Z1Z1;
    ScL H = U2 - p.X;
    ScL R = S2 - p.Y;
    ScL HH = H.sqr();
    ScL HHH = H * HH;
    ScL W = p.X * HH;
    ScL X3 = (R.sqr() - HHH - (W + W)).norm();
    ScL Y3 = (R * (W - X3) - p.Y * HHH).norm();
    p.Z = p.Z * H;
    p.X = X3;
    p.Y = Y3;
    Hn = H.norm();
}

// x^(q - 2): Fermat's inverse in the lazy radix; the exponent's bits are wave-uniform.  0 -> 0.
__device__ __forceinline__ ScL scale_inv(const ScL& x) {
    ScL acc = ScL::load(Fq::one());
    for (int i = 253; i >= 0; --i) {
        acc = acc.sqr();
        uint32_t w = FqParams::P[i >> 5];
        if (i < 32) w -= 2;   // q - 2: q is odd and its low word is >= 2
        if ((w >> (i & 31)) & 1) acc = acc * x;
    }
    return acc;
}

__global__ __launch_bounds__(SC_BLOCK) void k_g1_scale(const G1A* in, G1A* out, Fq* __restrict__ side, size_t count, ScaleDigits dg, Fq beta) {
    __shared__ int32_t tab[4][2][9][SC_BLOCK];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SC_TILE + t;
    if (base >= count) return;   // the lane owns no point (its later points lie further out still)
    const ScL one = ScL::load(Fq::one()), betaL = ScL::load(beta);
    ScL run = one;               // Z_0 .. Z_{j-1}
    uint32_t finite = 0;
    for (int j = 0; j < SC_PPL; ++j) {
        const size_t i = base + (size_t)j * SC_BLOCK;
        if (i >= count) break;
        const G1A p = in[i];
        JacR<Fq> acc;
        acc.inf = true;
        acc.X = acc.Y = acc.Z = one;
        ScL G = one;
        if (!p.is_inf() && dg.top >= 0) {
            {   // the table: P, 3P, 5P, 7P over a common Z, on the isomorphic curve
                const ScL x = ScL::load(p.x), y = ScL::load(p.y);
                JacR<Fq> P1;
                P1.inf = false; P1.X = x; P1.Y = y; P1.Z = one;
                const JacR<Fq> D = dbl_lazy(P1);
                const ScL C = D.Z, C2 = C.sqr(), C3 = C2 * C;
                const ScL dx = D.X * one, dy = D.Y * one;
                JacR<Fq> A;
                A.inf = false; A.X = x * C2; A.Y = y * C3; A.Z = one;
                const ScL x1 = A.X, y1 = A.Y;
                ScL H1, H2, H3;
                scale_madd(A, dx, dy, H1);
                const ScL x3 = A.X, y3 = A.Y;
                scale_madd(A, dx, dy, H2);
                const ScL x5 = A.X, y5 = A.Y;
                scale_madd(A, dx, dy, H3);
                const ScL r3 = H2 * H3, r1 = A.Z;
                G = r1 * C;
                auto put = [&](int e, const ScL& X, const ScL& Y, const ScL& r, bool scale) {
                    ScL ex = X, ey = Y;
                    if (scale) {
                        const ScL r2 = r.sqr();
                        ex = X * r2;
                        ey = (Y * r2) * r;
                    }
#pragma unroll
                    for (int l = 0; l < 9; ++l) { tab[e][0][l][t] = ex.v[l]; tab[e][1][l][t] = ey.v[l]; }
                };
                put(0, x1, y1, r1, true);
                put(1, x3, y3, r3, true);
                put(2, x5, y5, H3, true);
                put(3, A.X, A.Y, one, false);
            }
            for (int b = dg.top; b >= 0; --b) {
                if (!acc.inf) acc = dbl_lazy(acc);
                const int e1 = dg.d1[b], e2 = dg.d2[b];   // the same for every lane: scalar branches
                if (e1) {
                    const int e = (e1 < 0 ? -e1 : e1) >> 1;
                    ScL qx, qy;
#pragma unroll
                    for (int l = 0; l < 9; ++l) { qx.v[l] = tab[e][0][l][t]; qy.v[l] = tab[e][1][l][t]; }
                    if (e1 < 0) qy = qy.neg().norm();
                    if (!madd_lazy(acc, qx, qy)) acc = dbl_lazy(acc);
                }
                if (e2) {
                    const int e = (e2 < 0 ? -e2 : e2) >> 1;
                    ScL qx, qy;
#pragma unroll
                    for (int l = 0; l < 9; ++l) { qx.v[l] = tab[e][0][l][t]; qy.v[l] = tab[e][1][l][t]; }
                    qx = qx * betaL;
                    if (e2 < 0) qy = qy.neg().norm();
                    if (!madd_lazy(acc, qx, qy)) acc = dbl_lazy(acc);
                }
            }
        }
        const bool fin = !acc.inf;
        const ScL z = fin ? acc.Z * G : one;
        out[i] = fin ? G1A{acc.X.store_exact(), acc.Y.store_exact()} : G1A::infinity();
        side[2 * i] = z.store_exact();
        side[2 * i + 1] = run.store_exact();
        run = run * z;
        finite |= (fin ? 1u : 0u) << j;
    }
    ScL inv = scale_inv(run);
    for (int j = SC_PPL - 1; j >= 0; --j) {
        const size_t i = base + (size_t)j * SC_BLOCK;
        if (i >= count) continue;
        const ScL zi = inv * ScL::load(side[2 * i + 1]);   // 1 / Z_j
        inv = inv * ScL::load(side[2 * i]);
        if (!((finite >> j) & 1)) continue;
        const G1A q = out[i];
        const ScL zi2 = zi.sqr();
        out[i] = G1A{(ScL::load(q.x) * zi2).store_exact(), ((ScL::load(q.y) * zi2) * zi).store_exact()};
    }
}

namespace {

const uint32_t SC_BETA_G1[8] = {0x607cfd48u, 0xe4bd44e5u, 0xbb966e3du, 0xc28f069fu, 0xe0acccb0u, 0x5e6dd9e7u, 0xe131a029u, 0x30644e72u};   // gbasis.hip GLV_BETA_G1

// d_out[i] = k d_in[i], i < count, on `st`; d_out may be d_in.  k canonical, below r.  The side buffer is freed after a synchronisation.
void g1_scale(zk_ctx* ctx, hipStream_t st, const G1A* d_in, G1A* d_out, size_t count, const Fr& k_can) {
    if (!count) return;
    ScaleDigits dg;
    scalar_recode(k_can.l, dg);
    Fq beta;
    for (int i = 0; i < 8; ++i) beta.l[i] = SC_BETA_G1[i];
    beta = Fq::from_canonical(beta);
    DevBuf<Fq> side(2 * count);
    {
        ProfScope ps(ctx, "g1_scale", 2.0 * sizeof(G1A) * count, st);
        hipLaunchKernelGGL(k_g1_scale, dim3(ceil_div(count, SC_TILE)), dim3(SC_BLOCK), 0, st, d_in, d_out, side.p, count, dg, beta);
    }
    wipe(&dg, sizeof(dg));
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));   // the side buffer goes out of scope
}

// ctx->stream is what the shared launchers (pts_to_mont, fr_powers, msm_build_table) enqueue on: for the length of one call it is
// the call's own stream, so that nothing is ordered into -- or waits behind -- the prover's main stream (as crs_check.hip)
struct OwnStream {
    zk_ctx* ctx;
    hipStream_t saved, own = nullptr;
    explicit OwnStream(zk_ctx* c) : ctx(c), saved(c->stream) {
        ZK_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        ctx->stream = own;
    }
    ~OwnStream() {
        ctx->stream = saved;
        (void)hipStreamSynchronize(own);
        (void)hipStreamDestroy(own);
    }
};

template <class T>
T fetch(const T* d, hipStream_t st) {
    T h;
    ZK_HIP(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return h;
}
template <class T>
void copy_buf(DevBuf<T>& dst, const DevBuf<T>& src, hipStream_t st) {
    dst.alloc(src.n);
    if (src.n) ZK_HIP(hipMemcpyAsync(dst.p, src.p, src.n * sizeof(T), hipMemcpyDeviceToDevice, st));
}
Fr fr_words(const uint64_t* w) {
    Fr x;
    for (int i = 0; i < 4; ++i) { x.l[2 * i] = (uint32_t)w[i]; x.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return x;
}
void g1_words(const G1A& p, uint64_t* w) {
    const Fq x = p.x.to_canonical(), y = p.y.to_canonical();
    for (int i = 0; i < 4; ++i) {
        w[i] = (uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32);
        w[4 + i] = (uint64_t)y.l[2 * i] | ((uint64_t)y.l[2 * i + 1] << 32);
    }
}

zk_crs* crs_contribute(zk_ctx* ctx, const zk_crs& src, Fr& d_can, const uint8_t* tag, zk_crs_contribution* record) {
    OwnStream scope(ctx);
    hipStream_t st = ctx->stream;
    const size_t n = src.n, nl = src.m - src.input - 1;
    Fr d_inv = Fr::from_canonical(d_can).inv().to_canonical(), nonce = draw_scalar_nonzero();
    struct Wipe {
        Fr &a, &b, &c;
        ~Wipe() { wipe(&a, sizeof(Fr)); wipe(&b, sizeof(Fr)); wipe(&c, sizeof(Fr)); }
    } wiper{d_can, d_inv, nonce};
    std::unique_ptr<zk_crs> c(new zk_crs());
    c->ctx = ctx;
    c->n = n; c->m = src.m; c->input = src.input;
    copy_buf(c->alpha1, src.alpha1, st); copy_buf(c->beta1, src.beta1, st);
    copy_buf(c->xi1, src.xi1, st); copy_buf(c->sum_gamma1, src.sum_gamma1, st);
    copy_buf(c->beta2, src.beta2, st); copy_buf(c->gamma2, src.gamma2, st); copy_buf(c->xi2, src.xi2, st);
    // the two single points: host code (one point each)
    const G1A delta1 = fetch(src.delta1.p, st);
    const G2A delta2 = fetch(src.delta2.p, st);
    const G1A nd1 = jac_to_affine(jac_mul_words(G1J::from_affine(delta1), d_can.l));
    const G2A nd2 = jac_to_affine(jac_mul_words(G2J::from_affine(delta2), d_can.l));
    c->delta1.alloc(1); c->delta2.alloc(1);
    ZK_HIP(hipMemcpyAsync(c->delta1.p, &nd1, sizeof(nd1), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(c->delta2.p, &nd2, sizeof(nd2), hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));   // nd1, nd2 are stack objects
    // the arrays that carry 1 / delta
    c->sum_delta1.alloc(src.sum_delta1.n);
    c->xi_t1.alloc(src.xi_t1.n);
    g1_scale(ctx, st, src.sum_delta1.p, c->sum_delta1.p, nl, d_inv);
    g1_scale(ctx, st, src.xi_t1.p, c->xi_t1.p, n - 1, d_inv);
    if (src.ap) {
        copy_buf(c->lag1, src.lag1, st); copy_buf(c->lag2, src.lag2, st);
        c->lagS_t1.alloc(src.lagS_t1.n);
        g1_scale(ctx, st, src.lagS_t1.p, c->lagS_t1.p, n - 1, d_inv);
        c->ap = true;
    }
    ZK_HIP(hipStreamSynchronize(st));
    uint64_t before_words[8];
    g1_words(delta1, before_words);
    zk_crs_contribution rec;
    ZK_REQUIRE(contribution_prove(before_words, d_can, nonce, tag, &rec), ZK_ERR_ARG, "zk_crs_contribute: the source's delta_g1 is infinity or off the curve");
    *record = rec;
    return c.release();
}

// ---- the check ----
struct CmpSeg {
    const uint32_t *a, *b;
    uint32_t words;
};
struct CmpSegs {
    CmpSeg s[7];
    uint32_t total;
};
// *flag = 1 when any word of any segment differs
__global__ void k_contrib_compare(CmpSegs segs, int* __restrict__ flag) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= segs.total) return;
    int k = 0;
    while (k < 6 && w >= segs.s[k].words) { w -= segs.s[k].words; ++k; }
    if (w < segs.s[k].words && segs.s[k].a[w] != segs.s[k].b[w]) atomicOr(flag, 1);
}

bool pairing_eq(const G1A& p1, const G2A& q1, const G1A& p2, const G2A& q2) {   // e(p1, q1) == e(p2, q2)
    const Fq12 f = ml_proj(p1, q1) * ml_proj(p2.neg(), q2);
    return final_exp_exact(f) == Fq12::one();
}

void contribution_check(zk_ctx* ctx, const zk_crs& a, const zk_crs& b, const zk_crs_contribution& rec, const uint8_t* tag, const Fr& s_can,
                        zk_crs_contribution_result* result) {
    const size_t n = a.n, l = a.input, nl = a.m - l - 1, N = std::max<size_t>(std::max(nl, n), 1);
    ZK_REQUIRE(n < ((size_t)1 << 26) && a.m < ((size_t)1 << 26), ZK_ERR_SIZE, "zk_crs_contribution_check: too large");
    OwnStream scope(ctx);
    hipStream_t st = ctx->stream;
    uint32_t failed = 0;
    // ---- the arrays a contribution leaves alone ----
    DevBuf<int> flag(1);
    ZK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    CmpSegs segs;
    auto seg = [](const void* x, const void* y, size_t bytes) { return CmpSeg{(const uint32_t*)x, (const uint32_t*)y, (uint32_t)(bytes / 4)}; };
    segs.s[0] = seg(a.alpha1.p, b.alpha1.p, sizeof(G1A));
    segs.s[1] = seg(a.beta1.p, b.beta1.p, sizeof(G1A));
    segs.s[2] = seg(a.beta2.p, b.beta2.p, sizeof(G2A));
    segs.s[3] = seg(a.gamma2.p, b.gamma2.p, sizeof(G2A));
    segs.s[4] = seg(a.xi1.p, b.xi1.p, n * sizeof(G1A));
    segs.s[5] = seg(a.xi2.p, b.xi2.p, n * sizeof(G2A));
    segs.s[6] = seg(a.sum_gamma1.p, b.sum_gamma1.p, (l + 1) * sizeof(G1A));
    segs.total = 0;
    for (int k = 0; k < 7; ++k) segs.total += segs.s[k].words;
    hipLaunchKernelGGL(k_contrib_compare, dim3(ceil_div(segs.total, 256)), dim3(256), 0, st, segs, flag.p);
    ZK_HIP(hipGetLastError());
    // ---- the random sums ----
    DevBuf<Fr> rho(N);
    fr_powers(ctx, Fr::from_canonical(s_can), Fr::one(), rho.p, N);
    fr_from_mont(ctx, rho.p, rho.p, N);
    MsmTable<Fq> t[4];
    MsmWorkspace ws;
    DevBuf<G1J> sums(4);
    const G1J inf = G1J::infinity();
    auto sum = [&](int k, const G1A* pts, size_t count) {
        if (!count) { ZK_HIP(hipMemcpyAsync(sums.p + k, &inf, sizeof(inf), hipMemcpyHostToDevice, st)); return; }
        msm_build_table<Fq>(ctx, pts, count, msm_auto_window(count), t[k]);
        msm_run<Fq>(ctx, ws, st, t[k], rho.p, count, 0, 1, sums.p + k);
    };
    sum(0, a.sum_delta1.p, nl);
    sum(1, b.sum_delta1.p, nl);
    sum(2, a.xi_t1.p, n - 1);
    sum(3, b.xi_t1.p, n - 1);
    G1J hs[4];
    int differs = 0;
    ZK_HIP(hipMemcpyAsync(hs, sums.p, sizeof(hs), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&differs, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    if (differs) failed |= ZK_CONTRIB_UNCHANGED;
    // ---- the single points, the record ----
    const G1A G = fetch(b.xi1.p, st), d1a = fetch(a.delta1.p, st), d1b = fetch(b.delta1.p, st);
    const G2A H = fetch(b.xi2.p, st), d2a = fetch(a.delta2.p, st), d2b = fetch(b.delta2.p, st);
    uint64_t wa[8], wb[8];
    g1_words(d1a, wa);
    g1_words(d1b, wb);
    if (std::memcmp(wa, rec.delta_before_g1, sizeof(wa)) || std::memcmp(wb, rec.delta_after_g1, sizeof(wb))) failed |= ZK_CONTRIB_RECORD;
    if (!contribution_verify(rec, tag)) failed |= ZK_CONTRIB_KNOWLEDGE;
    if (d1b.is_inf() || d2b.is_inf()) failed |= ZK_CONTRIB_DEGENERATE;
    if (!pairing_eq(d1b, H, G, d2b)) failed |= ZK_CONTRIB_DELTA_TWINS;
    if (!pairing_eq(jac_to_affine(hs[1]), d2b, jac_to_affine(hs[0]), d2a)) failed |= ZK_CONTRIB_SUM_DELTA;
    if (n >= 2 && !pairing_eq(jac_to_affine(hs[3]), d2b, jac_to_affine(hs[2]), d2a)) failed |= ZK_CONTRIB_XI_T;
    ZK_HIP(hipStreamSynchronize(st));   // the tables and the workspace go out of scope
    result->failed = failed;
    result->flags = 0;
}

}  // namespace

void g1_scale_resident(zk_ctx* ctx, hipStream_t st, const G1A* d_in, G1A* d_out, size_t count, const Fr& k_canonical) {
    g1_scale(ctx, st, d_in, d_out, count, k_canonical);
}

void g1_scale_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalar, uint64_t* out, size_t n) {
    ZK_REQUIRE(points && scalar && out, ZK_ERR_ARG, "zk_g1_scale_batch: null pointer");
    Fr k = fr_words(scalar);
    ZK_REQUIRE(k.raw_in_range(), ZK_ERR_RANGE, "coordinate or scalar >= modulus");
    if (!n) return;
    hipStream_t st = ctx->stream;
    DevBuf<G1A> dp(n);
    DevBuf<int> flag(1);
    ZK_HIP(hipMemcpyAsync(dp.p, points, n * sizeof(G1A), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    pts_to_mont<G1A>(ctx, dp.p, dp.p, n, flag.p);
    int hflag = 0;
    ZK_HIP(hipMemcpyAsync(&hflag, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_REQUIRE(!hflag, ZK_ERR_RANGE, "coordinate or scalar >= modulus");
    g1_scale(ctx, st, dp.p, dp.p, n, k);
    pts_from_mont<G1A>(ctx, dp.p, dp.p, n);
    ZK_HIP(hipMemcpyAsync(out, dp.p, n * sizeof(G1A), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_g1_scale_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t scalar[4], uint64_t* out, size_t n) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] { g1_scale_batch(ctx, points, scalar, out, n); ctx->resolve_profile(); });
}

int zk_crs_contribute(zk_ctx* ctx, const zk_crs* crs, const uint64_t d[4], const uint8_t tag[32], zk_crs** out, zk_crs_contribution* contribution) {
    if (out) *out = nullptr;
    if (!ctx || !crs || !out || !contribution) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(crs->ctx == ctx, ZK_ERR_ARG, "zk_crs_contribute: the CRS belongs to another context");
        Fr dc;
        if (d) {
            dc = fr_words(d);
            ZK_REQUIRE(dc.raw_in_range(), ZK_ERR_RANGE, "zk_crs_contribute: d >= r");
            ZK_REQUIRE(!dc.is_zero(), ZK_ERR_DIV_BY_ZERO, "zk_crs_contribute: d = 0");
        } else {
            dc = draw_scalar_nonzero();
        }
        *out = crs_contribute(ctx, *crs, dc, tag, contribution);   // wipes dc
        ctx->resolve_profile();
    });
}

int zk_crs_contribution_check(zk_ctx* ctx, const zk_crs* before, const zk_crs* after, const zk_crs_contribution* c, const uint8_t tag[32],
                              const uint64_t challenge[4], zk_crs_contribution_result* out) {
    if (!ctx || !before || !after || !c || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(before->ctx == ctx && after->ctx == ctx, ZK_ERR_ARG, "zk_crs_contribution_check: a CRS belongs to another context");
        ZK_REQUIRE(before->n == after->n && before->m == after->m && before->input == after->input, ZK_ERR_ARG,
                   "zk_crs_contribution_check: the two CRSs differ in (n, m, input)");
        Fr s;
        if (challenge) {
            ZK_REQUIRE(challenge[0] | challenge[1] | challenge[2] | challenge[3], ZK_ERR_ARG, "zk_crs_contribution_check: the challenge must be non-zero");
            s = fr_words(challenge);
            ZK_REQUIRE(s.raw_in_range(), ZK_ERR_RANGE, "zk_crs_contribution_check: challenge >= r");
        } else {
            s = draw_scalar_nonzero();
        }
        zk_crs_contribution_result res{0, 0};
        contribution_check(ctx, *before, *after, *c, tag, s, &res);
        ctx->resolve_profile();
        *out = res;
    });
}

}  // extern "C"
