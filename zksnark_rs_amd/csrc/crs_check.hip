// crs_check.hip -- zk_crs_check: are these arrays a Groth16 CRS for THIS QAP?  No trapdoor needed.
//
// zk_crs_upload / zk_crs_load check ranges, curves and the G2 subgroup; nothing there ties the arrays to each other or to the circuit.
// With xi_g1[k] = [x^k]_1 etc. (groth16/mod.rs:134-197) every such tie is linear in the exponent once it is paired, so each ARRAY is
// tested through ONE random linear combination with the weights rho_k = s^k of a secret challenge s:
//   point side   every sum is an inner product of a resident array with a scalar vector: the MSM launcher over one-off tables
//                (msm_build_table / msm_run, as g2_subgroup_check in crs.hip); the prover's tables are neither read nor built
//   scalar side  k_cc_powers   rho_k = s^k, Montgomery form and canonical integers, CC_CHAIN consecutive powers per lane from the
//                              lane's own start power s^(CC_CHAIN t) (no serial chain over the array)
//                k_cc_geometric S_d(z) = sum_{k<d} (s z)^k by its closed form at consecutive integers z (the Lagrange-basis arrays)
//                the weighted wire sums sum_i rho_i u_i / v_i / w_i by the prover's own kernels (k_spmv over the rows by gate,
//                k_dense_matvec), taken to coefficients by the prover's own transforms (inverse NTT / interpolation tree)
//   pairings     fewer than twenty, on the host over pairing.cuh: one product of Miller values and one final exponentiation a relation
// Everything runs on a stream of the call's own.  Q = sum rho_k xi_g1[k + 1] needs no shifted copy: msm_run takes a point offset.
#include <random>
#include "pipeline.hpp"
#include "qap_kernels.hpp"
#include "pairing.cuh"
#include "check_sums.hpp"   // the call's own stream, the Sums gatherer, pairing_product_is_one: shared with powers.hip

namespace zk {

static constexpr int CC_CHAIN = 16;   // powers per lane of k_cc_powers
static constexpr int CC_BLOCK = 256;

__device__ __forceinline__ Fr cc_pow(Fr base, uint64_t e) {
    Fr acc = Fr::one();
    for (int i = 63 - __clzll((long long)(e | 1)); i >= 0; --i) {
        acc = acc.sqr();
        if ((e >> i) & 1) acc = acc * base;
    }
    return acc;
}

// mont[k] = s^k (Montgomery), can[k] = the same as a canonical integer, k < count
__global__ void __launch_bounds__(CC_BLOCK) k_cc_powers(Fr s, Fr* __restrict__ mont, Fr* __restrict__ can, size_t count) {
    const size_t first = ((size_t)blockIdx.x * CC_BLOCK + threadIdx.x) * CC_CHAIN;
    if (first >= count) return;
    Fr p = cc_pow(s, first);
    const size_t end = first + CC_CHAIN < count ? first + CC_CHAIN : count;
    for (size_t k = first; k < end; ++k) {
        mont[k] = p;
        can[k] = p.to_canonical();
        p = p * s;
    }
}

// out[j] = S_d(z0 + j) = sum_{k<d} (s (z0 + j))^k as a canonical integer, j < count: ((s z)^d - 1) / (s z - 1), or d where s z = 1
__global__ void __launch_bounds__(CC_BLOCK) k_cc_geometric(Fr s, uint64_t z0, uint64_t d, Fr* __restrict__ out, size_t count) {
    const size_t j = (size_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t z = z0 + j;
    Fr zf = Fr::zero();
    zf.l[0] = (uint32_t)z; zf.l[1] = (uint32_t)(z >> 32);
    const Fr sz = s * Fr::from_canonical(zf);
    const Fr den = sz - Fr::one();
    Fr v;
    if (den.is_zero()) {
        Fr df = Fr::zero();
        df.l[0] = (uint32_t)d; df.l[1] = (uint32_t)(d >> 32);
        v = df;                                   // already the canonical integer
    } else {
        v = ((cc_pow(sz, d) - Fr::one()) * den.inv()).to_canonical();
    }
    out[j] = v;
}

namespace {

template <class F>
Aff<F> host_sub(const Aff<F>& a, const Aff<F>& b) {
    return jac_to_affine(jac_add(Jac<F>::from_affine(a), Jac<F>::from_affine(b.neg())));
}

// canonical coefficients (n each) of sum_{i < a_len} rho_i u_i | v_i | w_i, in this order, in `coef` (3 n elements)
void wire_sum_coefficients(zk_ctx* ctx, const zk_qap& q, const Fr* rho_mont, const Fr* rho_can, size_t a_len, Fr* coef) {
    const size_t n = q.n;
    hipStream_t st = ctx->stream;
    if (q.dense) {
        dense_matvec(ctx, q.du.p, rho_mont, a_len, n, coef);
        dense_matvec(ctx, q.dv.p, rho_mont, a_len, n, coef + n);
        dense_matvec(ctx, q.dw.p, rho_mont, a_len, n, coef + 2 * n);
        fr_from_mont(ctx, coef, coef, 3 * n);
        return;
    }
    // values by gate: the prover's SpMV with rho in the witness's place (canonical, as a witness is)
    DevBuf<Fr> vals(3 * n);
    spmv(ctx, q.u_gate, rho_can, a_len, vals.p);
    spmv(ctx, q.v_gate, rho_can, a_len, vals.p + n);
    spmv(ctx, q.w_gate, rho_can, a_len, vals.p + 2 * n);
    if (q.roots == 0) {
        if (q.log_n == 0) {
            ZK_HIP(hipMemcpyAsync(coef, vals.p, 3 * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        } else {
            ntt_dif(ctx, vals.p, q.log_n, true, true, 3);
            for (int k = 0; k < 3; ++k) bitrev_permute(ctx, vals.p + k * n, coef + k * n, q.log_n);
        }
    } else {
        const InterpTree& t = *q.arb->tree;
        const size_t npad = (size_t)1 << t.log_npad;
        DevBuf<Fr> work(9 * npad), out(3 * npad);
        interp_run(ctx, t, vals.p, n, 3, work.p, out.p);
        for (int k = 0; k < 3; ++k) ZK_HIP(hipMemcpyAsync(coef + k * n, out.p + k * npad, n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        fr_from_mont(ctx, coef, coef, 3 * n);
        ZK_HIP(hipStreamSynchronize(st));   // work and out go out of scope
        return;
    }
    fr_from_mont(ctx, coef, coef, 3 * n);
    ZK_HIP(hipStreamSynchronize(st));       // vals goes out of scope
}

void crs_check(zk_ctx* ctx, const zk_crs& c, const zk_qap& q, const Fr& s_can, zk_crs_check_result* result) {
    const size_t n = c.n, m = c.m, l = c.input, nl = m - l - 1, N = std::max(n, m);
    ZK_REQUIRE(n < ((size_t)1 << 31) && m < ((size_t)1 << 31), ZK_ERR_SIZE, "zk_crs_check: too large");
    StreamScope scope(ctx);
    hipStream_t st = ctx->stream;
    uint32_t failed = 0, flags = c.ap ? ZK_CRS_CHECK_LAGRANGE_PRESENT : 0u;

    // ---- what the QAP contributes: t as canonical coefficients, the tables of its form ----
    if (!q.dense) qc_ensure_w_gate(q, st);
    if (!q.dense && q.roots == 1) arb_attach_integer_roots(ctx, const_cast<zk_qap&>(q));   // the tree of the roots 1..n (and t, its root)
    DevBuf<Fr> tcan(n + 1);
    if (!q.dense && q.roots == 0) {   // t = X^n - 1
        ZK_HIP(hipMemsetAsync(tcan.p, 0, (n + 1) * sizeof(Fr), st));
        Fr minus_one = (-Fr::one()).to_canonical(), one = Fr::zero();
        one.l[0] = 1;
        ZK_HIP(hipMemcpyAsync(tcan.p, &minus_one, sizeof(Fr), hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(tcan.p + n, &one, sizeof(Fr), hipMemcpyHostToDevice, st));
        ZK_HIP(hipStreamSynchronize(st));
    } else {
        ZK_REQUIRE(q.dt.n >= n + 1, ZK_ERR_ARG, "zk_crs_check: the QAP holds no t");
        fr_from_mont(ctx, q.dt.p, tcan.p, n + 1);
    }
    const Fr t0 = fetch(tcan.p, st);

    // ---- scalar side ----
    const Fr s_mont = Fr::from_canonical(s_can);
    DevBuf<Fr> rho_m(N), rho_c(N), coef(3 * n), coef_in(3 * n);
    hipLaunchKernelGGL(k_cc_powers, dim3(ceil_div(ceil_div(N, CC_CHAIN), CC_BLOCK)), dim3(CC_BLOCK), 0, st, s_mont, rho_m.p, rho_c.p, N);
    ZK_HIP(hipGetLastError());
    wire_sum_coefficients(ctx, q, rho_m.p, rho_c.p, m, coef.p);

    // ---- point side ----
    MsmTable<Fq> t_xi1, t_xit, t_sg, t_sd;
    MsmTable<Fq2> t_xi2;
    msm_build_table<Fq>(ctx, c.xi1.p, n, msm_auto_window(n), t_xi1);
    msm_build_table<Fq2>(ctx, c.xi2.p, n, msm_auto_window_g2(n), t_xi2);
    if (n >= 2) msm_build_table<Fq>(ctx, c.xi_t1.p, n - 1, msm_auto_window(n - 1), t_xit);
    msm_build_table<Fq>(ctx, c.sum_gamma1.p, l + 1, msm_auto_window(l + 1), t_sg);
    if (nl) msm_build_table<Fq>(ctx, c.sum_delta1.p, nl, msm_auto_window(nl), t_sd);
    Sums S(ctx);
    const size_t i_all1 = S.g1(t_xi1, rho_c.p, n);
    const size_t i_all2 = S.g2(t_xi2, rho_c.p, n);
    const size_t i_p = S.g1(t_xi1, rho_c.p, n - 1);          // n == 1: empty sums, infinity
    const size_t i_q = S.g1(t_xi1, rho_c.p, n - 1, 1);
    const size_t i_xt = S.g1(t_xit, rho_c.p, n - 1);
    const size_t i_tp = S.g2(t_xi2, tcan.p + 1, n);           // [t'(x)]_2
    const size_t i_u = S.g1(t_xi1, coef.p, n);
    const size_t i_v = S.g2(t_xi2, coef.p + n, n);
    const size_t i_w = S.g1(t_xi1, coef.p + 2 * n, n);
    const size_t i_sg = S.g1(t_sg, rho_c.p, l + 1);
    const size_t i_sd = S.g1(t_sd, rho_c.p + l + 1, nl);
    size_t i_l1 = 0, i_l2 = 0, i_ls = 0;
    MsmTable<Fq> t_lag1, t_lagS;
    MsmTable<Fq2> t_lag2;
    DevBuf<Fr> sd_n(c.ap ? n : 0), sd_s(c.ap ? std::max<size_t>(n - 1, 1) : 0);
    if (c.ap) {
        hipLaunchKernelGGL(k_cc_geometric, dim3(ceil_div(n, CC_BLOCK)), dim3(CC_BLOCK), 0, st, s_mont, (uint64_t)1, (uint64_t)n, sd_n.p, n);
        if (n >= 2)
            hipLaunchKernelGGL(k_cc_geometric, dim3(ceil_div(n - 1, CC_BLOCK)), dim3(CC_BLOCK), 0, st, s_mont, (uint64_t)n + 1, (uint64_t)n - 1, sd_s.p, n - 1);
        ZK_HIP(hipGetLastError());
        msm_build_table<Fq>(ctx, c.lag1.p, n, msm_auto_window(n), t_lag1);
        msm_build_table<Fq2>(ctx, c.lag2.p, n, msm_auto_window_g2(n), t_lag2);
        if (n >= 2) msm_build_table<Fq>(ctx, c.lagS_t1.p, n - 1, msm_auto_window(n - 1), t_lagS);
        i_l1 = S.g1(t_lag1, sd_n.p, n);
        i_l2 = S.g2(t_lag2, sd_n.p, n);
        i_ls = S.g1(t_lagS, sd_s.p, n - 1);
    }
    S.read();

    // ---- the single points ----
    const G1A G = fetch(c.xi1.p, st), alpha1 = fetch(c.alpha1.p, st), beta1 = fetch(c.beta1.p, st), delta1 = fetch(c.delta1.p, st);
    const G2A H = fetch(c.xi2.p, st), beta2 = fetch(c.beta2.p, st), gamma2 = fetch(c.gamma2.p, st), delta2 = fetch(c.delta2.p, st);
    G1A gen1;
    G2A gen2;
    crs_generators(&gen1, &gen2);
    if (!same_point(G, gen1) || !same_point(H, gen2)) failed |= ZK_CRS_CHECK_GENERATORS;
    if (gamma2.is_inf() || delta2.is_inf() || delta1.is_inf() || alpha1.is_inf() || beta1.is_inf() || beta2.is_inf()) failed |= ZK_CRS_CHECK_DEGENERATE;
    if (!pairing_product_is_one({{beta1, H}, {G.neg(), beta2}}) || !pairing_product_is_one({{delta1, H}, {G.neg(), delta2}}))
        failed |= ZK_CRS_CHECK_TWINS;

    // ---- the arrays of powers ----
    const G1A P = S.h1[i_p], Q = S.h1[i_q];
    if (n >= 2) {
        const G2A xi2_1 = fetch(c.xi2.p + 1, st);
        if (fetch(c.xi_t1.p, st).is_inf()) flags |= ZK_CRS_CHECK_T_ZERO;
        if (!pairing_product_is_one({{P, xi2_1}, {Q.neg(), H}})) failed |= ZK_CRS_CHECK_POWERS_G1;
        const G1A t0P = jac_to_affine(jac_mul_words(G1J::from_affine(P), t0.l));
        if (!pairing_product_is_one({{S.h1[i_xt], delta2}, {Q.neg(), S.h2[i_tp]}, {t0P.neg(), H}})) failed |= ZK_CRS_CHECK_XI_T;
    }
    if (!pairing_product_is_one({{S.h1[i_all1], H}, {G.neg(), S.h2[i_all2]}})) failed |= ZK_CRS_CHECK_POWERS_G2;

    // ---- the wires ----
    const G1A U = S.h1[i_u], W = S.h1[i_w], SG = S.h1[i_sg], SD = S.h1[i_sd];
    const G2A V = S.h2[i_v];
    if (!pairing_product_is_one({{SG, gamma2}, {SD, delta2}, {U.neg(), beta2}, {alpha1.neg(), V}, {W.neg(), H}})) {
        failed |= ZK_CRS_CHECK_WIRES;
        // once more over the wires i <= l alone; the wires behind them are the difference
        wire_sum_coefficients(ctx, q, rho_m.p, rho_c.p, l + 1, coef_in.p);
        Sums R(ctx);
        const size_t j_u = R.g1(t_xi1, coef_in.p, n), j_v = R.g2(t_xi2, coef_in.p + n, n), j_w = R.g1(t_xi1, coef_in.p + 2 * n, n);
        R.read();
        const G1A Ui = R.h1[j_u], Wi = R.h1[j_w];
        const G2A Vi = R.h2[j_v];
        if (!pairing_product_is_one({{SG, gamma2}, {Ui.neg(), beta2}, {alpha1.neg(), Vi}, {Wi.neg(), H}})) failed |= ZK_CRS_CHECK_WIRES_GAMMA;
        if (!pairing_product_is_one({{SD, delta2}, {host_sub(U, Ui).neg(), beta2}, {alpha1.neg(), host_sub(V, Vi)}, {host_sub(W, Wi).neg(), H}}))
            failed |= ZK_CRS_CHECK_WIRES_DELTA;
    }

    // ---- the same CRS in the Lagrange bases: plain point equalities ----
    if (c.ap) {
        if (!same_point(S.h1[i_l1], S.h1[i_all1]) || !same_point(S.h2[i_l2], S.h2[i_all2]) || !same_point(S.h1[i_ls], S.h1[i_xt]))
            failed |= ZK_CRS_CHECK_LAGRANGE;
    }
    ZK_HIP(hipStreamSynchronize(st));   // the tables and the workspace go out of scope
    result->failed = failed;
    result->flags = flags;
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zk_crs_check(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const uint64_t challenge[4], zk_crs_check_result* out) {
    if (!ctx || !crs || !qap || !out) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(crs->ctx == ctx && qap->ctx == ctx, ZK_ERR_ARG, "zk_crs_check: the CRS or the QAP belongs to another context");
        ZK_REQUIRE(crs->n == qap->n && crs->m == qap->m && crs->input == qap->input, ZK_ERR_ARG,
                   "zk_crs_check: the CRS and the QAP differ in (n, m, input)");
        Fr s;
        if (challenge) {
            ZK_REQUIRE(challenge[0] | challenge[1] | challenge[2] | challenge[3], ZK_ERR_ARG, "zk_crs_check: the challenge must be non-zero");
            s = fr_from_u64x4(challenge);
            ZK_REQUIRE(s.raw_in_range(), ZK_ERR_RANGE, "zk_crs_check: challenge >= r");
        } else {
            s = draw_challenge();
        }
        zk_crs_check_result res{0, 0};
        crs_check(ctx, *crs, *qap, s, &res);
        ctx->resolve_profile();
        *out = res;
    });
}

}  // extern "C"
