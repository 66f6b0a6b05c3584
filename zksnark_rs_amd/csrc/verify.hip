// verify.hip -- groth16::verify (/root/reference/src/groth16/mod.rs:299-320) and the pairing it
// needs (EllipticEncryptable::pairing = bn::pairing, /root/reference/src/groth16/fr.rs:120-122;
// GtLocal "+" = Gt multiplication, fr.rs:225-231).
//
// verify is not on the accelerated path: it is one call per proof with l+1 scalar multiplications
// and four pairings, CPU code in the reference and host code here (the same ff.cuh / ec.cuh
// arithmetic compiled for the host).  Optimal ate pairing on BN254: tower Fq2 = Fq[i]/(i^2+1),
// Fq6 = Fq2[v]/(v^3 - xi), xi = 9 + i, Fq12 = Fq6[w]/(w^2 - v); D-type twist
// psi(x', y') = (x' w^2, y' w^3); affine line functions; final exponentiation by square-and-multiply
// with (q^12 - 1)/r.  The four pairings of the check share one final exponentiation:
//   e(alpha,beta) e(S,gamma) e(C,delta) == e(A,B)  <=>  FE(ml(alpha,beta) ml(S,gamma) ml(C,delta) ml(-A,B)) == 1.
#include "pipeline.hpp"
#include "pairing.cuh"
#include "verify_host.hpp"

namespace zk {

// line through T and Q2 on the twist (tangent when `dbl`), evaluated at P; T <- T + Q2
static Fq12 line_and_add(G2A& T, const G2A& Q2, bool dbl, const G1A& P) {
    Fq2 lam;
    if (dbl) {
        Fq2 x2 = T.x.sqr();
        lam = (x2.dbl() + x2) * T.y.dbl().inv();
    } else {
        lam = (Q2.y - T.y) * (Q2.x - T.x).inv();
    }
    Fq2 x3 = lam.sqr() - T.x - Q2.x;
    Fq2 y3 = lam * (T.x - x3) - T.y;
    // l = yP - lam xP w + (lam xT - yT) v w
    Fq12 l;
    l.c0 = Fq6{Fq2{P.y, Fq::zero()}, Fq2::zero(), Fq2::zero()};
    l.c1 = Fq6{-(lam * Fq2{P.x, Fq::zero()}), lam * T.x - T.y, Fq2::zero()};
    T = G2A{x3, y3};
    return l;
}

static Fq12 miller_loop(const G1A& P, const G2A& Q) {
    if (P.is_inf() || Q.is_inf()) return Fq12::one();
    Fq12 f = Fq12::one();
    G2A T = Q;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        Fq12 l = line_and_add(T, T, true, P);
        f = f.sqr() * l;
        if ((ATE_LOOP[i >> 5] >> (i & 31)) & 1) {
            l = line_and_add(T, Q, false, P);
            f = f * l;
        }
    }
    const Fq2 gx = fq2_from_words(GAMMA_X), gy = fq2_from_words(GAMMA_Y);
    G2A Q1{fq2_conj(Q.x) * gx, fq2_conj(Q.y) * gy};
    G2A Q2{fq2_conj(Q1.x) * gx, -(fq2_conj(Q1.y) * gy)};   // -pi^2(Q)
    f = f * line_and_add(T, Q1, false, P);
    f = f * line_and_add(T, Q2, false, P);
    return f;
}
static Fq12 final_exponentiation(const Fq12& f) { return f.pow_words(FINAL_EXP, FINAL_EXP_WORDS); }

static void fq12_to_words(const Fq12& f, uint64_t* out) {
    const Fq2* parts[6] = {&f.c0.a0, &f.c0.a1, &f.c0.a2, &f.c1.a0, &f.c1.a1, &f.c1.a2};
    for (int k = 0; k < 6; ++k) {
        Fq c[2] = {parts[k]->c0.to_canonical(), parts[k]->c1.to_canonical()};
        for (int h = 0; h < 2; ++h)
            for (int i = 0; i < 4; ++i) out[(2 * k + h) * 4 + i] = (uint64_t)c[h].l[2 * i] | ((uint64_t)c[h].l[2 * i + 1] << 32);
    }
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_pairing(const uint64_t g1[ZK_G1_WORDS], const uint64_t g2[ZK_G2_WORDS], uint64_t out[48]) {
    if (!g1 || !g2 || !out) return ZK_ERR_ARG;
    G1A P;
    G2A Q;
    if (!rd_g1(g1, P) || !rd_g2(g2, Q)) return ZK_ERR_RANGE;
    fq12_to_words(final_exponentiation(miller_loop(P, Q)), out);
    return ZK_OK;
}

int zk_verify(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t proof[ZK_PROOF_BYTES], int* ok) {
    if (!ctx || !crs || !proof || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    *ok = 0;
    return guarded(ctx, [&] {
        const size_t l = crs->input;
        // host copies of the handful of CRS points verify reads
        std::vector<uint64_t> sg((l + 1) * 8), a1(8), b2(16), g2(16), d2(16);
        zk_crs_out o{};
        o.alpha_g1 = a1.data(); o.sum_gamma_g1 = sg.data(); o.beta_g2 = b2.data(); o.gamma_g2 = g2.data(); o.delta_g2 = d2.data();
        crs_download(ctx, *crs, o);
        G1A alpha, A, C;
        G2A beta, gamma, delta, B;
        ZK_REQUIRE(rd_g1(a1.data(), alpha) && rd_g2(b2.data(), beta) && rd_g2(g2.data(), gamma) && rd_g2(d2.data(), delta), ZK_ERR_ARG, "verify: CRS point not on the curve or outside G2");
        G1A S;
        if (!verify_decode_sum(sg.data(), l, inputs, n_inputs, proof, A, B, C, S)) return;   // malformed / off-curve proof: rejected
        Fq12 f = miller_loop(alpha, beta) * miller_loop(S, gamma) * miller_loop(C, delta) * miller_loop(A.neg(), B);
        *ok = final_exponentiation(f) == Fq12::one() ? 1 : 0;
    });
}

}  // extern "C"
