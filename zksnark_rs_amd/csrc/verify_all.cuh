// verify_all.cuh -- zk_verify_batch_all's per-lane step and final combination for host and device (ZK_HD): one pairing check
// for a whole batch of proofs over one CRS by a random linear combination with secret 128-bit multipliers z_j != 0,
//
//   prod_j e(A_j, B_j)^{z_j} == e(alpha, beta)^{t_0} e(T_S, gamma) e(T_C, delta),
//   t_0 = sum_j z_j,  t_i = sum_j z_j x_ji (mod r),  T_S = sum_{i=0..k} t_i sum_gamma_i,  T_C = sum_j z_j C_j,
//
// checked as FE( prod_j ml(-z_j A_j, B_j) * ml(t_0 alpha, beta) ml(T_S, gamma) ml(T_C, delta) ) == 1 (FE: the exact final
// exponentiation of pairing.cuh).  The kernels of verify_batch_all.hip and tests/cpp/verify_all_check.hip call the same functions.
#pragma once
#include "pairing.cuh"

namespace zk {

// what a lane (one proof) contributes and what the reductions carry: the Miller product, the C sum, the decode flag
struct VbaAcc {
    Fq12 f;
    G1J c;
    int ok;
};
ZK_HD VbaAcc vba_identity() { return VbaAcc{Fq12::one(), G1J::infinity(), 1}; }
// complete: jac_add handles P + P and P - P (the same proof twice, cancelling C's)
ZK_HD VbaAcc vba_combine(const VbaAcc& a, const VbaAcc& b) {
    return VbaAcc{fq12_mul_ni(a.f, b.f), jac_add_ni(a.c, b.c), (a.ok && b.ok) ? 1 : 0};
}

// k P for P affine and k given as little-endian 32-bit words, of which the low `bits` are scanned (MSB first, complete additions)
ZK_HD G1J g1_mul_bits(const G1A& p, const uint32_t* k, int bits) {
    G1J acc = G1J::infinity();
    for (int i = bits - 1; i >= 0; --i) {
        acc = jac_dbl_ni(acc);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = jac_madd_ni(acc, p);
    }
    return acc;
}

// one proof: zk_verify's decoder, z A and z C (z: 4 words, 128 bits), the Miller loop of (-z A, B) with B's lines on the fly.
// A proof that fails to decode contributes ok = 0 and the identity otherwise.
ZK_HD VbaAcc vba_lane(const uint8_t* proof, const uint32_t* z) {
    G1A a = G1A::infinity(), c = G1A::infinity();
    G2A b = G2A::infinity();
    const bool ok = dec_g1(proof, a) && dec_g2(proof + 65, b) && dec_g1(proof + 194, c);
    if (!ok) {
        a = c = G1A::infinity();
        b = G2A::infinity();
    }
    const G1A za = jac_to_affine(g1_mul_bits(a, z, 128)).neg();
    return VbaAcc{ml_proj(za, b), g1_mul_bits(c, z, 128), ok ? 1 : 0};
}

// the terms of T_S: t_i sum_gamma_i, t_i canonical (< r < 2^254)
ZK_HD G1J vba_ts_term(const Fr& t, const G1A& sg) { return g1_mul_bits(sg, t.l, 254); }

// z_j x_ji for x canonical and zm = z_j in Montgomery form: the Montgomery product (z R) x R^-1 is z x mod r, canonical
ZK_HD Fr vba_zx(const Fr& zm, const uint64_t* x) {
    Fr v;
    for (int h = 0; h < 4; ++h) { v.l[2 * h] = (uint32_t)x[h]; v.l[2 * h + 1] = (uint32_t)(x[h] >> 32); }
    return zm * v;
}
ZK_HD Fr vba_z_mont(const uint32_t* z) {
    Fr v = Fr::zero();
    for (int h = 0; h < 4; ++h) v.l[h] = z[h];
    return Fr::from_canonical(v);
}

// the fixed arguments of the final combination, computed once per call on the host: the lines of beta, gamma and delta
// (pairing.cuh ml_lines), t_0 alpha, and which of beta, gamma, delta is finite
struct VbaFixed {
    Line lines[3][ATE_LINES];
    G1A t0_alpha;
    int finite[3];
};

// prod of three fixed-argument Miller loops with one shared squaring per step
ZK_HD Fq12 ml_fixed3(const G1A* P, const VbaFixed& fx) {
    bool live[3];
    for (int q = 0; q < 3; ++q) live[q] = fx.finite[q] && !P[q].is_inf();
    Fq12 f = Fq12::one();
    int n = 0;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        f = fq12_sqr_ni(f);
        for (int q = 0; q < 3; ++q) f = mul_line(f, fx.lines[q][n], P[q], live[q]);
        ++n;
        if (ate_bit(i)) {
            for (int q = 0; q < 3; ++q) f = mul_line(f, fx.lines[q][n], P[q], live[q]);
            ++n;
        }
    }
    for (int s = 0; s < 2; ++s, ++n)
        for (int q = 0; q < 3; ++q) f = mul_line(f, fx.lines[q][n], P[q], live[q]);
    return f;
}

// the verdict: every proof decoded and FE(prod_j ml(-z_j A_j, B_j) ml(t_0 alpha, beta) ml(T_S, gamma) ml(T_C, delta)) == 1
ZK_HD bool vba_finish(const VbaAcc& acc, const G1J& ts, const VbaFixed& fx) {
    const G1A P[3] = {fx.t0_alpha, jac_to_affine(ts), jac_to_affine(acc.c)};
    const Fq12 f = fq12_mul_ni(acc.f, ml_fixed3(P, fx));
    return acc.ok && final_exp_exact(f) == Fq12::one();
}

}  // namespace zk
