// powers.hip -- phase 1 of a trustless setup: a resident powers-of-tau transcript (zk_powers), its check, a contribution
// to it and the check of a contribution; and k_mul_each, the kernel a contribution multiplies the transcript with.
//
// k_mul_each<F, W>: out[i] = scalar[i] P[i], a DIFFERENT scalar for every point.  k_point_mul (field_kernels.hip) walks 254 bits per
// lane; gb_mul (gbasis.cuh) splits by the endomorphism but walks a per-lane non-adjacent form: a wave skips an addition only where all
// 64 lanes have a zero digit, which is practically never, so it executes ~260 mixed additions where one lane needs ~86.  k_g1_scale
// (crs_contribute.hip) made the digits a kernel argument, which works for ONE scalar only.  Here every lane
//   splits      its own scalar, k = k1 + k2 lambda (mul_each_recode.hpp, branch-free), and
//   recodes     both halves into a REGULAR signed window form: ND digits of width W, every one odd and non-zero.  All lanes add at
//               the same 2 ND positions; only the table index and the sign differ, and those are a per-lane LDS address and a select.
//               An even (or zero) half is recoded as |k_h| + 1 and the point is subtracted once at the end.
//   table       P, 3P, .., (2^W - 1) P per point WITHOUT an inversion: k_g1_scale's construction (D = 2P is an affine point of the
//               isomorphic curve on which P is (x C^2, y C^3); 2^(W-1) - 1 mixed additions of D; every entry brought to the last
//               entry's Z by the products of the later additions' H).  The entries are first stored as they come and rescaled in a
//               second pass backwards, so that only the H values stay in registers.  In LDS, [entry][coordinate][limb][lane]: a
//               lane reads its own column, 64 consecutive words per (entry, coordinate, limb) row whatever the entry: conflict-free.
//               phi(x, y) = (beta x, y) is formed where it is used.
//   widths      G1: W = 4, 8 entries, 36 KiB a wave, 32 digits a half: 64 additions + 124 doublings.  G2: W = 3, 4 entries, 36 KiB,
//               43 digits: 86 additions + 126 doublings (W = 4 would take 72 KiB a wave, two waves a compute unit).
//   inversion   as k_g1_scale: a lane owns ppl points (4; 2 or 1 for arrays that would not fill the machine twice over) and inverts the product of their Z once, by Fermat's exponentiation (constant
//               time: Z depends on the secret scalars); over Fq2 through the norm, conj(z) / (z0^2 + z1^2).
// Special cases are lazy29.cuh's own: madd_lazy reports P + P (doubled) and clears the accumulator on P - P; an infinity input skips
// everything and stays infinity; the scalar 0 recodes as (1, 1) with both corrections: P + phi(P) - P - phi(P) = infinity.
// Limb bounds: the table is k_g1_scale's sequence (crs_contribute.hip's header) with more entries of the same kind: every entry is a
// product of Montgomery outputs or norm'ed values, except the last, which is madd's own norm'ed (X3, Y3); a ratio is an H (norm'ed)
// times a Montgomery output.  The loop is dbl_lazy / madd_lazy on their own results, the affine operand a table entry, its x times
// beta (a Montgomery output) or its y negated and norm'ed -- what k_g1_scale feeds them.  The select between y and -y moves limbs only.
#include "pipeline.hpp"
#include "check_sums.hpp"
#include "gbasis.cuh"
#include "mul_each_recode.hpp"
#include "crs_contribution.hpp"

namespace zk {

constexpr int ME_BLOCK = 64;                  // lanes per work-group: one wave
constexpr int ME_PPL = 4;                     // points a lane owns (and inverts together) when the array is long enough; 2 or 1 otherwise (mul_each)

typedef FpR<FqParams> MeL;
template <class F> struct MeWidth;
template <> struct MeWidth<Fq> { static constexpr int W = ME_W_G1; };
template <> struct MeWidth<Fq2> { static constexpr int W = ME_W_G2; };

// a value's limbs <-> one lane's column of LDS rows (ME_BLOCK words apart)
template <class L> struct MeLimbs;
template <> struct MeLimbs<MeL> {
    static constexpr int N = 9;
    static __device__ __forceinline__ void put(int32_t* col, const MeL& x) {
#pragma unroll
        for (int l = 0; l < 9; ++l) col[l * ME_BLOCK] = x.v[l];
    }
    static __device__ __forceinline__ void get(const int32_t* col, MeL& x) {
#pragma unroll
        for (int l = 0; l < 9; ++l) x.v[l] = col[l * ME_BLOCK];
    }
    static __device__ __forceinline__ MeL select(bool c, const MeL& a, const MeL& b) {
        MeL r;
#pragma unroll
        for (int l = 0; l < 9; ++l) r.v[l] = c ? a.v[l] : b.v[l];
        return r;
    }
    // 1 / z, constant time: z^(q - 2), the exponent's bits are wave-uniform.  0 -> 0.
    static __device__ __forceinline__ MeL inv(const MeL& x) {
        MeL acc = MeL::load(Fq::one());
        for (int i = 253; i >= 0; --i) {
            acc = acc.sqr();
            uint32_t w = FqParams::P[i >> 5];
            if (i < 32) w -= 2;   // q - 2: q is odd and its low word is >= 2
            if ((w >> (i & 31)) & 1) acc = acc * x;
        }
        return acc;
    }
};
template <> struct MeLimbs<Fp2R<FqParams>> {
    typedef Fp2R<FqParams> L2;
    static constexpr int N = 18;
    static __device__ __forceinline__ void put(int32_t* col, const L2& x) {
        MeLimbs<MeL>::put(col, x.c0);
        MeLimbs<MeL>::put(col + 9 * ME_BLOCK, x.c1);
    }
    static __device__ __forceinline__ void get(const int32_t* col, L2& x) {
        MeLimbs<MeL>::get(col, x.c0);
        MeLimbs<MeL>::get(col + 9 * ME_BLOCK, x.c1);
    }
    static __device__ __forceinline__ L2 select(bool c, const L2& a, const L2& b) {
        return L2{MeLimbs<MeL>::select(c, a.c0, b.c0), MeLimbs<MeL>::select(c, a.c1, b.c1)};
    }
    static __device__ __forceinline__ L2 inv(const L2& z) {   // conj(z) / (z0^2 + z1^2)
        const MeL ni = MeLimbs<MeL>::inv(MeL::mont_sum(z.c0, z.c0, z.c1, z.c1));
        return L2{z.c0 * ni, (z.c1 * ni).neg().norm()};
    }
};

// madd_lazy's general branch (no special case can occur between the odd multiples of P below 2^W and 2P for a point of prime order
// r), H handed out in normal form: crs_contribute.hip's scale_madd over either field
template <class F>
__device__ __forceinline__ void me_madd(JacR<F>& p, const typename LazyOf<F>::type& qx, const typename LazyOf<F>::type& qy,
                                        typename LazyOf<F>::type& Hn) {
    typedef typename LazyOf<F>::type L;
    L Z1Z1 = p.Z.sqr();
    L U2 = qx * Z1Z1;
    L S2 = (qy * p.Z) * Z1Z1;
    L H = U2 - p.X;
    L R = S2 - p.Y;
    L HH = H.sqr();
    L HHH = H * HH;
    L Wv = p.X * HH;
    L X3 = (R.sqr() - HHH - (Wv + Wv)).norm();
    L Y3 = (R * (Wv - X3) - p.Y * HHH).norm();
    p.Z = p.Z * H;
    p.X = X3;
    p.Y = Y3;
    Hn = H.norm();
}

template <class F, int W>
__global__ __launch_bounds__(ME_BLOCK) void k_mul_each(const Aff<F>* in, const Fr* __restrict__ sc, Aff<F>* out, F* __restrict__ side,
                                                       size_t count, int ppl, Fq beta) {
    typedef typename LazyOf<F>::type L;
    typedef MeLimbs<L> ML;
    typedef RegularRecode<W> RR;
    constexpr int E = 1 << (W - 1);               // table entries: P, 3P, .., (2^W - 1) P
    constexpr int ROW = ML::N * ME_BLOCK;         // words of one (entry, coordinate)
    __shared__ int32_t tab[E * 2 * ROW];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * ME_BLOCK * ppl + t;   // block b: the points [b 64 ppl, (b + 1) 64 ppl), lane t those at t + 64 j
    if (base >= count) return;   // the lane owns no point (its later points lie further out still)
    const L one = L::load(F::one());
    const MeL betaL = MeL::load(beta);
    L run = one;                 // Z_0 .. Z_{j-1}
    uint32_t finite = 0;
    for (int j = 0; j < ppl; ++j) {
        const size_t i = base + (size_t)j * ME_BLOCK;
        if (i >= count) break;
        const Aff<F> p = in[i];
        JacR<F> acc;
        acc.inf = true;
        acc.X = acc.Y = acc.Z = one;
        L G = one;
        if (!p.is_inf()) {
            uint32_t b1[RR::NW], b2[RR::NW];
            bool neg1, neg2, even1, even2;
            {
                const Fr k = sc[i];
                uint32_t k1[5], k2[5];
                glv_split_nearest(k.l, k1, neg1, k2, neg2);
                regular_recode<W>(k1, b1, even1);
                regular_recode<W>(k2, b2, even2);
            }
            {   // the table over a common Z, on the isomorphic curve
                const L x = L::load(p.x), y = L::load(p.y);
                JacR<F> P1;
                P1.inf = false; P1.X = x; P1.Y = y; P1.Z = one;
                const JacR<F> D = dbl_lazy(P1);
                const L C = D.Z, C2 = C.sqr(), C3 = C2 * C;
                const L dx = D.X * one, dy = D.Y * one;
                JacR<F> A;
                A.inf = false; A.X = x * C2; A.Y = y * C3; A.Z = one;
                ML::put(tab + t, A.X);
                ML::put(tab + ROW + t, A.Y);
                L H[E];
#pragma unroll
                for (int e = 1; e < E; ++e) {
                    me_madd<F>(A, dx, dy, H[e]);
                    ML::put(tab + (2 * e) * ROW + t, A.X);
                    ML::put(tab + (2 * e + 1) * ROW + t, A.Y);
                }
                G = A.Z * C;
                L r = H[E - 1];   // Z_last / Z_e
#pragma unroll
                for (int e = E - 2; e >= 0; --e) {
                    L X, Y;
                    ML::get(tab + (2 * e) * ROW + t, X);
                    ML::get(tab + (2 * e + 1) * ROW + t, Y);
                    const L r2 = r.sqr();
                    ML::put(tab + (2 * e) * ROW + t, X * r2);
                    ML::put(tab + (2 * e + 1) * ROW + t, (Y * r2) * r);
                    if (e) r = r * H[e];
                }
            }
            // acc += (-1)^negate [phi] (2 e + 1) P
            auto add = [&](uint32_t e, bool negate, bool phi) {
                L qx, qy;
                ML::get(tab + (2 * e) * ROW + t, qx);
                ML::get(tab + (2 * e + 1) * ROW + t, qy);
                if (phi) qx = GlvPhi<F>::mul(qx, betaL);
                qy = ML::select(negate, qy.neg().norm(), qy);
                if (!madd_lazy(acc, qx, qy)) acc = dbl_lazy(acc);
            };
#pragma unroll 1
            for (int d = 0; d < RR::ND; ++d) {
                if (d) {
#pragma unroll 1
                    for (int w = 0; w < W; ++w) acc = dbl_lazy(acc);
                }
                uint32_t e1, e2;
                bool n1, n2;
                regular_next<W>(b1, e1, n1);
                regular_next<W>(b2, e2, n2);
                add(e1, n1 != neg1, false);
                add(e2, n2 != neg2, true);
            }
            if (even1) add(0, !neg1, false);   // |k1| + 1 was recoded: take sign(k1) P off again
            if (even2) add(0, !neg2, true);
        }
        const bool fin = !acc.inf;
        const L z = fin ? acc.Z * G : one;
        out[i] = fin ? Aff<F>{acc.X.store_exact(), acc.Y.store_exact()} : Aff<F>::infinity();
        side[2 * i] = z.store_exact();
        side[2 * i + 1] = run.store_exact();
        run = run * z;
        finite |= (fin ? 1u : 0u) << j;
    }
    L inv = ML::inv(run);
    for (int j = ppl - 1; j >= 0; --j) {
        const size_t i = base + (size_t)j * ME_BLOCK;
        if (i >= count) continue;
        const L zi = inv * L::load(side[2 * i + 1]);   // 1 / Z_j
        inv = inv * L::load(side[2 * i]);
        if (!((finite >> j) & 1)) continue;
        const Aff<F> q = out[i];
        const L zi2 = zi.sqr();
        out[i] = Aff<F>{(L::load(q.x) * zi2).store_exact(), ((L::load(q.y) * zi2) * zi).store_exact()};
    }
}

// powers_mul_form = 1: gb_mul per point, one lane a point -- what there was before k_mul_each; the comparator of tools/time_powers.py
template <class F>
__global__ __launch_bounds__(64) void k_mul_each_gb(const Aff<F>* in, const Fr* __restrict__ sc, Aff<F>* out, size_t count, Fq beta) {
    __shared__ Jac<F> prod[64];   // jac_to_affine takes its argument by reference: LDS keeps it out of scratch
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    prod[threadIdx.x] = jacr_store(gb_mul(jacr_load(Jac<F>::from_affine(in[i])), sc[i], beta));
    out[i] = jac_to_affine(prod[threadIdx.x]);
}

template <class A>
__global__ void k_pw_fill(A* __restrict__ out, A v, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = v;
}

namespace {

// d_out[i] = d_sc[i] d_in[i], i < count, on `st`; d_out may be d_in; d_sc canonical, below r.  Synchronises (the side buffer).
template <class F>
void mul_each(zk_ctx* ctx, hipStream_t st, const Aff<F>* d_in, const Fr* d_sc, Aff<F>* d_out, size_t count) {
    if (!count) return;
    const Fq beta = glv_beta<F>();
    const bool g2 = sizeof(F) > sizeof(Fq);
    if (ctx->opt_powers_mul_form == 1) {
        ProfScope ps(ctx, g2 ? "mul_each_gb_g2" : "mul_each_gb_g1", (2.0 * sizeof(Aff<F>) + sizeof(Fr)) * count, st);
        hipLaunchKernelGGL(k_mul_each_gb<F>, dim3(ceil_div(count, 64)), dim3(64), 0, st, d_in, d_sc, d_out, count, beta);
        ZK_HIP(hipGetLastError());
        return;
    }
    // Points a lane owns.  The table's LDS leaves one wave a SIMD, 4 cu_count waves at a time; a lane's further points run one after
    // the other and save only their share of the inversion (about a fifth of a multiplication), so they pay once the array fills the
    // machine for two rounds of waves anyway -- below that the points are spread over more waves instead.
    const size_t two_rounds = 2 * 4 * (size_t)std::max(ctx->cu_count, 1);
    int ppl = ME_PPL;
    while (ppl > 1 && ceil_div(count, (size_t)ME_BLOCK * ppl) < two_rounds) ppl >>= 1;
    if (ctx->opt_powers_mul_ppl == 1 || ctx->opt_powers_mul_ppl == 2 || ctx->opt_powers_mul_ppl == 4) ppl = (int)ctx->opt_powers_mul_ppl;   // tests: every value at every length
    DevBuf<F> side(2 * count);
    {
        ProfScope ps(ctx, g2 ? "mul_each_g2" : "mul_each_g1", (2.0 * sizeof(Aff<F>) + sizeof(Fr)) * count, st);
        hipLaunchKernelGGL((k_mul_each<F, MeWidth<F>::W>), dim3(ceil_div(count, (size_t)ME_BLOCK * ppl)), dim3(ME_BLOCK), 0, st, d_in, d_sc, d_out,
                           side.p, count, ppl, beta);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemsetAsync(side.p, 0, side.bytes(), st));   // the Z values depend on the scalars
    ZK_HIP(hipStreamSynchronize(st));                      // the side buffer goes out of scope
}

// a device array of secret scalars: zeroed before it is freed, on every path
struct SecretBuf {
    DevBuf<Fr> buf;
    hipStream_t st;
    SecretBuf(size_t n, hipStream_t s) : buf(n), st(s) {}
    ~SecretBuf() {
        if (buf.p) {
            (void)hipMemsetAsync(buf.p, 0, buf.bytes(), st);
            (void)hipStreamSynchronize(st);
        }
    }
};

template <class A>
void pw_up(zk_ctx* ctx, DevBuf<A>& d, const uint64_t* src, size_t count, int* d_flag) {
    d.alloc(count);
    ZK_HIP(hipMemcpyAsync(d.p, src, count * sizeof(A), hipMemcpyHostToDevice, ctx->stream));
    pts_to_mont<A>(ctx, d.p, d.p, count, d_flag);
    pts_check_on_curve<A>(ctx, d.p, count, d_flag);
}
template <class A>
void pw_down(zk_ctx* ctx, const DevBuf<A>& d, uint64_t* dst, size_t count) {
    if (!dst || !count) return;
    DevBuf<A> tmp(count);
    pts_from_mont<A>(ctx, d.p, tmp.p, count);
    ZK_HIP(hipMemcpyAsync(dst, tmp.p, count * sizeof(A), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
}
int pw_flag(zk_ctx* ctx, const int* d_flag) {
    int h = 0;
    ZK_HIP(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    return h;
}
void pw_g1_words(const G1A& p, uint64_t* w) {   // Montgomery -> canonical words; infinity = zeros
    const Fq x = p.x.to_canonical(), y = p.y.to_canonical();
    for (int i = 0; i < 4; ++i) {
        w[i] = (uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32);
        w[4 + i] = (uint64_t)y.l[2 * i] | ((uint64_t)y.l[2 * i + 1] << 32);
    }
}
Fr pw_challenge(const uint64_t* challenge, const char* who) {
    if (!challenge) return draw_challenge();
    ZK_REQUIRE(challenge[0] | challenge[1] | challenge[2] | challenge[3], ZK_ERR_ARG, std::string(who) + ": the challenge must be non-zero");
    const Fr c = fr_from_u64x4(challenge);
    ZK_REQUIRE(c.raw_in_range(), ZK_ERR_RANGE, std::string(who) + ": challenge >= r");
    return c;
}

// the ZK_POWERS_CHECK_* bits of one transcript, on ctx->stream (the caller's StreamScope)
uint32_t check_bits(zk_ctx* ctx, const zk_powers& p, const Fr& c_can) {
    const size_t N1 = p.n1, N2 = p.n2;
    ZK_REQUIRE(N1 < ((size_t)1 << 31), ZK_ERR_SIZE, "zk_powers_check: too large");
    hipStream_t st = ctx->stream;
    uint32_t failed = 0;
    DevBuf<Fr> rho(N1);
    fr_powers(ctx, Fr::from_canonical(c_can), Fr::one(), rho.p, N1);
    fr_from_mont(ctx, rho.p, rho.p, N1);
    MsmTable<Fq> t_tau, t_alpha, t_beta;
    MsmTable<Fq2> t_tau2;
    msm_build_table<Fq>(ctx, p.tau1.p, N1, msm_auto_window(N1), t_tau);
    msm_build_table<Fq>(ctx, p.alpha_tau1.p, N2, msm_auto_window(N2), t_alpha);
    msm_build_table<Fq>(ctx, p.beta_tau1.p, N2, msm_auto_window(N2), t_beta);
    msm_build_table<Fq2>(ctx, p.tau2.p, N2, msm_auto_window_g2(N2), t_tau2);
    Sums S(ctx);
    const size_t i_p = S.g1(t_tau, rho.p, N1 - 1);
    const size_t i_q = S.g1(t_tau, rho.p, N1 - 1, 1);   // the same weights over tau_g1[1 ..]: msm_run's point offset
    const size_t i_t = S.g1(t_tau, rho.p, N2);
    const size_t i_a = S.g1(t_alpha, rho.p, N2);
    const size_t i_b = S.g1(t_beta, rho.p, N2);
    const size_t i_2 = S.g2(t_tau2, rho.p, N2);
    S.read();
    const G1A G = fetch(p.tau1.p, st), tau1_1 = fetch(p.tau1.p + 1, st), alpha0 = fetch(p.alpha_tau1.p, st), beta0 = fetch(p.beta_tau1.p, st);
    const G2A H = fetch(p.tau2.p, st), tau2_1 = fetch(p.tau2.p + 1, st), beta2 = fetch(p.beta2.p, st);
    G1A gen1;
    G2A gen2;
    crs_generators(&gen1, &gen2);
    if (!same_point(G, gen1) || !same_point(H, gen2)) failed |= ZK_POWERS_CHECK_GENERATORS;
    if (tau1_1.is_inf() || tau2_1.is_inf() || alpha0.is_inf() || beta0.is_inf() || beta2.is_inf()) failed |= ZK_POWERS_CHECK_DEGENERATE;
    const G2A S2 = S.h2[i_2];
    if (!pairing_product_is_one({{S.h1[i_p], tau2_1}, {S.h1[i_q].neg(), H}})) failed |= ZK_POWERS_CHECK_POWERS_G1;
    if (!pairing_product_is_one({{S.h1[i_t], H}, {G.neg(), S2}})) failed |= ZK_POWERS_CHECK_POWERS_G2;
    if (!pairing_product_is_one({{S.h1[i_a], H}, {alpha0.neg(), S2}})) failed |= ZK_POWERS_CHECK_ALPHA;
    if (!pairing_product_is_one({{S.h1[i_b], H}, {beta0.neg(), S2}})) failed |= ZK_POWERS_CHECK_BETA;
    if (!pairing_product_is_one({{beta0, H}, {G.neg(), beta2}})) failed |= ZK_POWERS_CHECK_BETA_TWINS;
    ZK_HIP(hipStreamSynchronize(st));   // the tables and the workspace go out of scope
    return failed;
}

std::unique_ptr<zk_powers> new_powers(zk_ctx* ctx, size_t n1, size_t n2) {
    ZK_REQUIRE(n2 >= 2 && n1 >= n2, ZK_ERR_ARG, "zk_powers: n_rest >= 2 and n_tau_g1 >= n_rest are required");
    std::unique_ptr<zk_powers> p(new zk_powers());
    p->ctx = ctx;
    p->n1 = n1;
    p->n2 = n2;
    return p;
}

}  // namespace

zk_powers* powers_upload(zk_ctx* ctx, const zk_powers_desc& d) {
    ZK_REQUIRE(d.tau_g1 && d.tau_g2 && d.alpha_tau_g1 && d.beta_tau_g1 && d.beta_g2, ZK_ERR_ARG, "zk_powers_upload: null point array");
    std::unique_ptr<zk_powers> p = new_powers(ctx, d.n_tau_g1, d.n_rest);
    StreamScope scope(ctx);
    DevBuf<int> flag(1);
    ZK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), ctx->stream));
    pw_up(ctx, p->tau1, d.tau_g1, p->n1, flag.p);
    pw_up(ctx, p->alpha_tau1, d.alpha_tau_g1, p->n2, flag.p);
    pw_up(ctx, p->beta_tau1, d.beta_tau_g1, p->n2, flag.p);
    pw_up(ctx, p->tau2, d.tau_g2, p->n2, flag.p);
    pw_up(ctx, p->beta2, d.beta_g2, 1, flag.p);
    int h = pw_flag(ctx, flag.p);
    ZK_REQUIRE(!(h & 2), ZK_ERR_RANGE, "zk_powers_upload: coordinate >= q");
    ZK_REQUIRE(!(h & 4), ZK_ERR_RANGE, "zk_powers_upload: point not on the curve");
    g2_subgroup_check(ctx, p->beta2.p, 1, flag.p);
    g2_subgroup_check(ctx, p->tau2.p, p->n2, flag.p);
    h = pw_flag(ctx, flag.p);
    ZK_REQUIRE(!(h & 8), ZK_ERR_RANGE, "zk_powers_upload: G2 point outside the subgroup of order r");
    return p.release();
}

zk_powers* powers_initial(zk_ctx* ctx, size_t n1, size_t n2) {
    std::unique_ptr<zk_powers> p = new_powers(ctx, n1, n2);
    StreamScope scope(ctx);
    hipStream_t st = ctx->stream;
    G1A g;
    G2A h;
    crs_generators(&g, &h);
    p->tau1.alloc(n1); p->alpha_tau1.alloc(n2); p->beta_tau1.alloc(n2); p->tau2.alloc(n2); p->beta2.alloc(1);
    hipLaunchKernelGGL(k_pw_fill<G1A>, dim3(ceil_div(n1, 256)), dim3(256), 0, st, p->tau1.p, g, n1);
    hipLaunchKernelGGL(k_pw_fill<G1A>, dim3(ceil_div(n2, 256)), dim3(256), 0, st, p->alpha_tau1.p, g, n2);
    hipLaunchKernelGGL(k_pw_fill<G1A>, dim3(ceil_div(n2, 256)), dim3(256), 0, st, p->beta_tau1.p, g, n2);
    hipLaunchKernelGGL(k_pw_fill<G2A>, dim3(ceil_div(n2, 256)), dim3(256), 0, st, p->tau2.p, h, n2);
    hipLaunchKernelGGL(k_pw_fill<G2A>, dim3(1), dim3(256), 0, st, p->beta2.p, h, (size_t)1);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));
    return p.release();
}

void powers_download(zk_ctx* ctx, const zk_powers& p, const zk_powers_out& o) {
    StreamScope scope(ctx);
    pw_down(ctx, p.tau1, o.tau_g1, p.n1);
    pw_down(ctx, p.tau2, o.tau_g2, p.n2);
    pw_down(ctx, p.alpha_tau1, o.alpha_tau_g1, p.n2);
    pw_down(ctx, p.beta_tau1, o.beta_tau_g1, p.n2);
    pw_down(ctx, p.beta2, o.beta_g2, 1);
}

void powers_check(zk_ctx* ctx, const zk_powers& p, const uint64_t* challenge, zk_powers_check_result* out) {
    const Fr c = pw_challenge(challenge, "zk_powers_check");
    StreamScope scope(ctx);
    const uint32_t failed = check_bits(ctx, p, c);
    out->failed = failed;
    out->flags = 0;
}

zk_powers* powers_contribute(zk_ctx* ctx, const zk_powers& src, const uint64_t* secrets, const uint8_t* tag, zk_powers_contribution* record) {
    uint64_t sec[12];
    Fr v[3], vm[3];
    struct Wipe {
        uint64_t* s;
        Fr *a, *b;
        ~Wipe() { wipe(s, 12 * sizeof(uint64_t)); wipe(a, 3 * sizeof(Fr)); wipe(b, 3 * sizeof(Fr)); }
    } wiper{sec, v, vm};
    for (int i = 0; i < 3; ++i) {
        if (secrets) {
            v[i] = fr_from_u64x4(secrets + 4 * i);
            ZK_REQUIRE(v[i].raw_in_range(), ZK_ERR_RANGE, "zk_powers_contribute: a secret >= r");
            ZK_REQUIRE(!v[i].is_zero(), ZK_ERR_DIV_BY_ZERO, "zk_powers_contribute: a secret = 0");
        } else {
            v[i] = draw_scalar_nonzero();
        }
        for (int w = 0; w < 4; ++w) sec[4 * i + w] = (uint64_t)v[i].l[2 * w] | ((uint64_t)v[i].l[2 * w + 1] << 32);
        vm[i] = Fr::from_canonical(v[i]);
    }
    StreamScope scope(ctx);
    hipStream_t st = ctx->stream;
    const size_t N1 = src.n1, N2 = src.n2;
    // the record: host code over the three before-points
    uint64_t before[24];
    pw_g1_words(fetch(src.tau1.p + 1, st), before);
    pw_g1_words(fetch(src.alpha_tau1.p, st), before + 8);
    pw_g1_words(fetch(src.beta_tau1.p, st), before + 16);
    zk_powers_contribution rec;
    const int status = powers_contribution_prove(before, sec, nullptr, tag, &rec);
    ZK_REQUIRE(status == ZK_OK, status, "zk_powers_contribute: a before-point of the record is out of range or off the curve");
    std::unique_ptr<zk_powers> p = new_powers(ctx, N1, N2);
    p->tau1.alloc(N1); p->alpha_tau1.alloc(N2); p->beta_tau1.alloc(N2); p->tau2.alloc(N2); p->beta2.alloc(1);
    {
        // s^k, a s^k, b s^k as canonical integers, on the device only
        SecretBuf S(N1, st), A(N2, st), B(N2, st);
        fr_powers(ctx, vm[0], Fr::one(), S.buf.p, N1);
        fr_powers(ctx, vm[0], vm[1], A.buf.p, N2);
        fr_powers(ctx, vm[0], vm[2], B.buf.p, N2);
        fr_from_mont(ctx, S.buf.p, S.buf.p, N1);
        fr_from_mont(ctx, A.buf.p, A.buf.p, N2);
        fr_from_mont(ctx, B.buf.p, B.buf.p, N2);
        mul_each<Fq>(ctx, st, src.tau1.p, S.buf.p, p->tau1.p, N1);
        mul_each<Fq2>(ctx, st, src.tau2.p, S.buf.p, p->tau2.p, N2);
        mul_each<Fq>(ctx, st, src.alpha_tau1.p, A.buf.p, p->alpha_tau1.p, N2);
        mul_each<Fq>(ctx, st, src.beta_tau1.p, B.buf.p, p->beta_tau1.p, N2);
        mul_each<Fq2>(ctx, st, src.beta2.p, B.buf.p, p->beta2.p, 1);   // b s^0
        ZK_HIP(hipStreamSynchronize(st));
    }
    *record = rec;
    return p.release();
}

void powers_contribution_check(zk_ctx* ctx, const zk_powers& a, const zk_powers& b, const zk_powers_contribution& rec, const uint8_t* tag,
                               const uint64_t* challenge, zk_powers_check_result* out) {
    const Fr c = pw_challenge(challenge, "zk_powers_contribution_check");
    StreamScope scope(ctx);
    hipStream_t st = ctx->stream;
    uint32_t failed = check_bits(ctx, b, c);
    uint64_t wa[24], wb[24];
    pw_g1_words(fetch(a.tau1.p + 1, st), wa);
    pw_g1_words(fetch(a.alpha_tau1.p, st), wa + 8);
    pw_g1_words(fetch(a.beta_tau1.p, st), wa + 16);
    pw_g1_words(fetch(b.tau1.p + 1, st), wb);
    pw_g1_words(fetch(b.alpha_tau1.p, st), wb + 8);
    pw_g1_words(fetch(b.beta_tau1.p, st), wb + 16);
    const zk_crs_contribution* part[3] = {&rec.tau, &rec.alpha, &rec.beta};
    for (int i = 0; i < 3; ++i) {
        if (std::memcmp(wa + 8 * i, part[i]->delta_before_g1, 64) || std::memcmp(wb + 8 * i, part[i]->delta_after_g1, 64)) failed |= ZK_POWERS_CHECK_RECORD;
        bool inf = true;
        for (int w = 0; w < 8; ++w) inf = inf && part[i]->delta_after_g1[w] == 0;
        if (inf) failed |= ZK_POWERS_CHECK_DEGENERATE;
    }
    if (!powers_contribution_verify(rec, tag)) failed |= ZK_POWERS_CHECK_KNOWLEDGE;
    out->failed = failed;
    out->flags = 0;
}

template <class F>
void mul_each_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n) {
    ZK_REQUIRE(points && scalars && out, ZK_ERR_ARG, "zk_g*_mul_each: null pointer");
    if (!n) return;
    hipStream_t st = ctx->stream;
    DevBuf<Aff<F>> dp(n);
    DevBuf<Fr> ds(n);
    DevBuf<int> flag(1);
    ZK_HIP(hipMemcpyAsync(dp.p, points, n * sizeof(Aff<F>), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(ds.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    pts_to_mont<Aff<F>>(ctx, dp.p, dp.p, n, flag.p);
    fr_check_range(ctx, ds.p, n, flag.p);
    ZK_REQUIRE(!pw_flag(ctx, flag.p), ZK_ERR_RANGE, "coordinate or scalar >= modulus");
    mul_each<F>(ctx, st, dp.p, ds.p, dp.p, n);
    pts_from_mont<Aff<F>>(ctx, dp.p, dp.p, n);
    ZK_HIP(hipMemcpyAsync(out, dp.p, n * sizeof(Aff<F>), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
}
template void mul_each_batch<Fq>(zk_ctx*, const uint64_t*, const uint64_t*, uint64_t*, size_t);
template void mul_each_batch<Fq2>(zk_ctx*, const uint64_t*, const uint64_t*, uint64_t*, size_t);

}  // namespace zk

using namespace zk;

extern "C" {

int zk_g1_mul_each(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] { mul_each_batch<Fq>(ctx, points, scalars, out, n); ctx->resolve_profile(); });
}
int zk_g2_mul_each(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] { mul_each_batch<Fq2>(ctx, points, scalars, out, n); ctx->resolve_profile(); });
}

int zk_powers_upload(zk_ctx* ctx, const zk_powers_desc* desc, zk_powers** out) {
    if (out) *out = nullptr;
    if (!ctx || !desc || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] { *out = powers_upload(ctx, *desc); });
}
int zk_powers_initial(zk_ctx* ctx, size_t n_tau_g1, size_t n_rest, zk_powers** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] { *out = powers_initial(ctx, n_tau_g1, n_rest); });
}
int zk_powers_dims(const zk_powers* powers, size_t* n_tau_g1, size_t* n_rest) {
    if (!powers) return ZK_ERR_ARG;
    if (n_tau_g1) *n_tau_g1 = powers->n1;
    if (n_rest) *n_rest = powers->n2;
    return ZK_OK;
}
int zk_powers_download(zk_ctx* ctx, const zk_powers* powers, const zk_powers_out* out) {
    if (!ctx || !powers || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(powers->ctx == ctx, ZK_ERR_ARG, "zk_powers_download: the transcript belongs to another context");
        powers_download(ctx, *powers, *out);
    });
}
void zk_powers_free(zk_powers* powers) {
    if (!powers) return;
    (void)hipSetDevice(powers->ctx->device);
    delete powers;
}
int zk_powers_check(zk_ctx* ctx, const zk_powers* powers, const uint64_t challenge[4], zk_powers_check_result* out) {
    if (!ctx || !powers || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(powers->ctx == ctx, ZK_ERR_ARG, "zk_powers_check: the transcript belongs to another context");
        zk_powers_check_result res{0, 0};
        powers_check(ctx, *powers, challenge, &res);
        ctx->resolve_profile();
        *out = res;
    });
}
int zk_powers_contribute(zk_ctx* ctx, const zk_powers* before, const uint64_t secrets[12], const uint8_t tag[32], zk_powers** out,
                         zk_powers_contribution* record) {
    if (out) *out = nullptr;
    if (!ctx || !before || !out || !record) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(before->ctx == ctx, ZK_ERR_ARG, "zk_powers_contribute: the transcript belongs to another context");
        *out = powers_contribute(ctx, *before, secrets, tag, record);
        ctx->resolve_profile();
    });
}
int zk_powers_contribution_check(zk_ctx* ctx, const zk_powers* before, const zk_powers* after, const zk_powers_contribution* record,
                                 const uint8_t tag[32], const uint64_t challenge[4], zk_powers_check_result* out) {
    if (!ctx || !before || !after || !record || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(before->ctx == ctx && after->ctx == ctx, ZK_ERR_ARG, "zk_powers_contribution_check: a transcript belongs to another context");
        ZK_REQUIRE(before->n1 == after->n1 && before->n2 == after->n2, ZK_ERR_ARG, "zk_powers_contribution_check: the two transcripts differ in size");
        zk_powers_check_result res{0, 0};
        powers_contribution_check(ctx, *before, *after, *record, tag, challenge, &res);
        ctx->resolve_profile();
        *out = res;
    });
}

}  // extern "C"
