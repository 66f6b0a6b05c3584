// pairing.cuh -- the BN254 optimal ate pairing for host and device (ZK_HD): the tower Fq6 = Fq2[v]/(v^3 - xi),
// Fq12 = Fq6[w]/(w^2 - v), xi = 9 + i; Frobenius maps; the proof-point decoder; Miller-loop steps in homogeneous projective
// coordinates with sparse lines (no inversion per step); the exact final exponentiation f^((q^12 - 1) / r).
//
// zk_verify / zk_pairing (verify.hip) run the affine Miller loop and the square-and-multiply final exponentiation;
// zk_verify_batch (verify_batch.hip) runs the projective steps, fixed-argument lines for gamma and delta, and the exponentiation
// split into its easy part (q^6 - 1)(q^2 + 1) and its hard part (q^4 - q^2 + 1) / r.  Both give the same pairing value: the two
// Miller loops differ by factors in proper subfields of Fq12, which the final exponentiation sends to 1.
#pragma once
#include "ec.cuh"
#include "pairing_consts.hpp"

namespace zk {

ZK_HD Fq fq_small(uint32_t v) { return Fq::from_u32(v); }
ZK_HD Fq2 fq2_mul_xi(const Fq2& a) {   // (9 + i) * a
    Fq n0 = a.c0.dbl().dbl().dbl() + a.c0, n1 = a.c1.dbl().dbl().dbl() + a.c1;
    return Fq2{n0 - a.c1, n1 + a.c0};
}
ZK_HD Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, -a.c1}; }
ZK_HD Fq2 fq2_mul_fq(const Fq2& a, const Fq& b) { return Fq2{a.c0 * b, a.c1 * b}; }
ZK_HD Fq2 fq2_from_words(const uint32_t* w) {
    Fq2 x;
    for (int i = 0; i < 8; ++i) { x.c0.l[i] = w[i]; x.c1.l[i] = w[8 + i]; }
    return Fq2::from_canonical(x);
}
// a / 2: a + (a odd ? q : 0) is even and < 2^255, so the shift loses nothing (halving commutes with the Montgomery factor)
ZK_HD Fq fq_half(const Fq& a) {
    const uint32_t mask = 0u - (a.l[0] & 1u);
    Fq s;
    uint64_t c = 0;
    for (int i = 0; i < 8; ++i) {
        c += (uint64_t)a.l[i] + (FqParams::P[i] & mask);
        s.l[i] = (uint32_t)c;
        c >>= 32;
    }
    for (int i = 0; i < 7; ++i) s.l[i] = (s.l[i] >> 1) | (s.l[i + 1] << 31);
    s.l[7] >>= 1;
    return s;
}
ZK_HD Fq2 fq2_half(const Fq2& a) { return Fq2{fq_half(a.c0), fq_half(a.c1)}; }

struct Fq6 {
    Fq2 a0, a1, a2;
    ZK_HD static Fq6 zero() { return Fq6{Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
    ZK_HD static Fq6 one() { return Fq6{Fq2::one(), Fq2::zero(), Fq2::zero()}; }
    ZK_HD Fq6 operator+(const Fq6& o) const { return Fq6{a0 + o.a0, a1 + o.a1, a2 + o.a2}; }
    ZK_HD Fq6 operator-(const Fq6& o) const { return Fq6{a0 - o.a0, a1 - o.a1, a2 - o.a2}; }
    ZK_HD Fq6 operator-() const { return Fq6{-a0, -a1, -a2}; }
    ZK_HD Fq6 operator*(const Fq6& o) const {
        Fq2 c0 = a0 * o.a0 + fq2_mul_xi(a1 * o.a2 + a2 * o.a1);
        Fq2 c1 = a0 * o.a1 + a1 * o.a0 + fq2_mul_xi(a2 * o.a2);
        Fq2 c2 = a0 * o.a2 + a1 * o.a1 + a2 * o.a0;
        return Fq6{c0, c1, c2};
    }
    // *this * (e0 + e1 v)
    ZK_HD Fq6 mul_01(const Fq2& e0, const Fq2& e1) const {
        return Fq6{a0 * e0 + fq2_mul_xi(a2 * e1), a0 * e1 + a1 * e0, a1 * e1 + a2 * e0};
    }
    ZK_HD Fq6 mul_v() const { return Fq6{fq2_mul_xi(a2), a0, a1}; }
    ZK_HD Fq6 inv() const {
        Fq2 t0 = a0.sqr() - fq2_mul_xi(a1 * a2);
        Fq2 t1 = fq2_mul_xi(a2.sqr()) - a0 * a1;
        Fq2 t2 = a1.sqr() - a0 * a2;
        Fq2 d = (a0 * t0 + fq2_mul_xi(a2 * t1 + a1 * t2)).inv();
        return Fq6{t0 * d, t1 * d, t2 * d};
    }
    ZK_HD bool operator==(const Fq6& o) const { return a0 == o.a0 && a1 == o.a1 && a2 == o.a2; }
    // the q^k-power Frobenius, k = 1..3 (v = w^2, v^2 = w^4)
    ZK_HD Fq6 frobenius(int k) const {
        const bool odd = k & 1;
        return Fq6{odd ? fq2_conj(a0) : a0, (odd ? fq2_conj(a1) : a1) * fq2_from_words(FROB[k - 1][2]),
                   (odd ? fq2_conj(a2) : a2) * fq2_from_words(FROB[k - 1][4])};
    }
};

struct Fq12 {
    Fq6 c0, c1;
    ZK_HD static Fq12 one() { return Fq12{Fq6::one(), Fq6::zero()}; }
    ZK_HD Fq12 operator*(const Fq12& o) const {   // Karatsuba over Fq6
        Fq6 t0 = c0 * o.c0, t1 = c1 * o.c1;
        return Fq12{t0 + t1.mul_v(), (c0 + c1) * (o.c0 + o.c1) - t0 - t1};
    }
    ZK_HD Fq12 sqr() const {   // (a + b w)^2 = a^2 + v b^2 + 2ab w, a^2 + v b^2 = (a + b)(a + v b) - ab - v ab
        Fq6 ab = c0 * c1;
        Fq6 t = (c0 + c1) * (c0 + c1.mul_v());
        return Fq12{t - ab - ab.mul_v(), ab + ab};
    }
    ZK_HD bool operator==(const Fq12& o) const { return c0 == o.c0 && c1 == o.c1; }
    ZK_HD Fq12 pow_words(const uint32_t* e, int nwords) const {
        Fq12 acc = one();
        bool started = false;
        for (int i = nwords * 32 - 1; i >= 0; --i) {
            if (started) acc = acc.sqr();
            if ((e[i >> 5] >> (i & 31)) & 1) { acc = acc * *this; started = true; }
        }
        return acc;
    }
    ZK_HD Fq12 conj() const { return Fq12{c0, -c1}; }   // the q^6-power Frobenius
    ZK_HD Fq12 inv() const {
        Fq6 d = (c0 * c0 - (c1 * c1).mul_v()).inv();
        return Fq12{c0 * d, -(c1 * d)};
    }
    // the q^k-power Frobenius, k = 1..3: the coefficient of w^j (c0.a0, c1.a0, c0.a1, c1.a1, c0.a2, c1.a2 for j = 0..5) is
    // conjugated k times and multiplied by xi^(j (q^k - 1) / 6)
    ZK_HD Fq12 frobenius(int k) const {
        const bool odd = k & 1;
        return Fq12{c0.frobenius(k), Fq6{(odd ? fq2_conj(c1.a0) : c1.a0) * fq2_from_words(FROB[k - 1][1]),
                                         (odd ? fq2_conj(c1.a1) : c1.a1) * fq2_from_words(FROB[k - 1][3]),
                                         (odd ? fq2_conj(c1.a2) : c1.a2) * fq2_from_words(FROB[k - 1][5])}};
    }
    // squaring in the cyclotomic subgroup (the elements of order dividing q^4 - q^2 + 1, where the easy part lands): Granger and
    // Scott, "Faster squaring in the cyclotomic subgroup of sixth degree extensions" (PKC 2010), Fq12 seen as Fq4^3 with
    // Fq4 = Fq2[y]/(y^2 - xi): six Fq2 multiplications instead of the 12 of sqr()
    ZK_HD Fq12 cyclotomic_sqr() const {
        const Fq2 &r0 = c0.a0, &r4 = c0.a1, &r3 = c0.a2, &r2 = c1.a0, &r1 = c1.a1, &r5 = c1.a2;
        Fq2 tmp = r0 * r1;
        const Fq2 t0 = (r0 + r1) * (fq2_mul_xi(r1) + r0) - tmp - fq2_mul_xi(tmp), t1 = tmp.dbl();
        tmp = r2 * r3;
        const Fq2 t2 = (r2 + r3) * (fq2_mul_xi(r3) + r2) - tmp - fq2_mul_xi(tmp), t3 = tmp.dbl();
        tmp = r4 * r5;
        const Fq2 t4 = (r4 + r5) * (fq2_mul_xi(r5) + r4) - tmp - fq2_mul_xi(tmp), t5 = tmp.dbl();
        const Fq2 xt5 = fq2_mul_xi(t5);
        Fq12 z;
        z.c0.a0 = (t0 - r0).dbl() + t0;     // 3 t0 - 2 r0
        z.c1.a1 = (t1 + r1).dbl() + t1;     // 3 t1 + 2 r1
        z.c1.a0 = (r2 + xt5).dbl() + xt5;   // 3 xi t5 + 2 r2
        z.c0.a2 = (t4 - r3).dbl() + t4;     // 3 t4 - 2 r3
        z.c0.a1 = (t2 - r4).dbl() + t2;     // 3 t2 - 2 r4
        z.c1.a2 = (r5 + t3).dbl() + t3;     // 3 t3 + 2 r5
        return z;
    }
    // *this * (d0 + (d1 + d2 v) w), the sparse value of a line
    ZK_HD Fq12 mul_034(const Fq2& d0, const Fq2& d1, const Fq2& d2) const {
        const Fq6 t0{c0.a0 * d0, c0.a1 * d0, c0.a2 * d0};
        const Fq6 t1 = c1.mul_01(d1, d2);
        const Fq6 s = (c0 + c1).mul_01(d0 + d1, d2);
        return Fq12{t0 + t1.mul_v(), s - t0 - t1};
    }
};

// out-of-line bodies: one copy per translation unit for the device loops (an Fq12 product inlines 81 base-field multiplications)
static ZK_NI Fq12 fq12_mul_ni(const Fq12& a, const Fq12& b) { return a * b; }
static ZK_NI Fq12 fq12_sqr_ni(const Fq12& a) { return a.sqr(); }
static ZK_NI Fq12 fq12_cyc_sqr_ni(const Fq12& a) { return a.cyclotomic_sqr(); }

// ---- the proof-point decoder (zk_verify and the batch kernels share it) ----
ZK_HD Fq fq_from_u64x4(const uint64_t* w) {
    Fq x;
    for (int i = 0; i < 4; ++i) { x.l[2 * i] = (uint32_t)w[i]; x.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return x;
}
ZK_HD bool rd_g1(const uint64_t* w, G1A& out) {
    Fq x = fq_from_u64x4(w), y = fq_from_u64x4(w + 4);
    if (!x.raw_in_range() || !y.raw_in_range()) return false;
    out = G1A{Fq::from_canonical(x), Fq::from_canonical(y)};
    if (out.is_inf()) return true;
    return out.y.sqr() == out.x.sqr() * out.x + fq_small(3);
}
ZK_HD bool rd_g2(const uint64_t* w, G2A& out) {
    Fq2 x{fq_from_u64x4(w), fq_from_u64x4(w + 4)}, y{fq_from_u64x4(w + 8), fq_from_u64x4(w + 12)};
    if (!x.raw_in_range() || !y.raw_in_range()) return false;
    out = G2A{Fq2::from_canonical(x), Fq2::from_canonical(y)};
    if (out.is_inf()) return true;
    if (!(out.y.sqr() == out.x.sqr() * out.x + fq2_from_words(TWIST_B))) return false;
    // r-torsion: the twist E'(Fq2) has order r * (2q - r) and the cofactor has small factors; the ate Miller loop is
    // bilinear only on the order-r subgroup G2, so a twist point outside it is rejected ([r]Q must be infinity).
    // G1 needs no such test: E(Fq) has prime order r.
    return jac_mul_words(G2J::from_affine(out), FrParams::P).is_inf();
}
ZK_HD void be_to_words(const uint8_t* be, uint64_t* w) {
    for (int i = 0; i < 4; ++i) {
        uint64_t v = 0;
        for (int b = 0; b < 8; ++b) v = (v << 8) | be[(3 - i) * 8 + b];
        w[i] = v;
    }
}
// decode the canonical 65 / 129 byte blocks of a proof
// The encoding is canonical, so that a proof has exactly one byte string: infinity is tag 0x00 followed by zeros ONLY,
// a finite point is tag 0x04 with coordinates < q that satisfy the curve equation ((0, 0), the in-memory
// image of infinity, is not on either curve and is rejected under tag 0x04).
ZK_HD bool all_zero(const uint8_t* p, size_t n) {
    uint8_t acc = 0;
    for (size_t i = 0; i < n; ++i) acc |= p[i];
    return acc == 0;
}
ZK_HD bool dec_g1(const uint8_t* p, G1A& out) {
    if (p[0] == 0) { out = G1A::infinity(); return all_zero(p + 1, 64); }
    if (p[0] != 4) return false;
    uint64_t w[8];
    be_to_words(p + 1, w); be_to_words(p + 33, w + 4);
    return rd_g1(w, out) && !out.is_inf();
}
ZK_HD bool dec_g2(const uint8_t* p, G2A& out) {
    if (p[0] == 0) { out = G2A::infinity(); return all_zero(p + 1, 128); }
    if (p[0] != 4) return false;
    uint64_t w[16];
    be_to_words(p + 1, w + 4); be_to_words(p + 33, w);          // x.c1 | x.c0
    be_to_words(p + 65, w + 12); be_to_words(p + 97, w + 8);    // y.c1 | y.c0
    return rd_g2(w, out) && !out.is_inf();
}

// ---- Miller loop in homogeneous projective coordinates (x = X/Z, y = Y/Z on the twist) ----
// Costello, Lange, Naehrig, "Faster pairing computations on curves with high-degree twists" (PKC 2010), D-type twist: a step
// returns the line l(P) = c0 yP + c1 xP w + c2 v w up to a factor in Fq2, which the final exponentiation sends to 1.
struct G2Proj {
    Fq2 X, Y, Z;
};
struct Line {
    Fq2 c0, c1, c2;
};

// T <- 2T; b3 = 3 b' (b' = 3 / xi, the twist's constant)
static ZK_NI Line dbl_step(G2Proj& T, const Fq2& b3) {
    const Fq2 a = fq2_half(T.X * T.Y);
    const Fq2 b = T.Y.sqr(), c = T.Z.sqr();
    const Fq2 e = b3 * c;
    const Fq2 f = e.dbl() + e;
    const Fq2 g = fq2_half(b + f);
    const Fq2 h = (T.Y + T.Z).sqr() - (b + c);   // 2 Y Z
    const Fq2 i = e - b;
    const Fq2 j = T.X.sqr();
    const Fq2 e2 = e.sqr();
    T.X = a * (b - f);
    T.Y = g.sqr() - (e2.dbl() + e2);
    T.Z = b * h;
    return Line{-h, j.dbl() + j, i};
}
// T <- T + Q (Q affine, T != +-Q)
static ZK_NI Line add_step(G2Proj& T, const G2A& Q) {
    const Fq2 theta = T.Y - Q.y * T.Z;
    const Fq2 lambda = T.X - Q.x * T.Z;
    const Fq2 c = theta.sqr(), d = lambda.sqr();
    const Fq2 e = lambda * d, f = T.Z * c, g = T.X * d;
    const Fq2 h = e + f - g.dbl();
    T.X = lambda * h;
    T.Y = theta * (g - h) - e * T.Y;
    T.Z = T.Z * e;
    return Line{lambda, -theta, theta * Q.x - lambda * Q.y};
}
// f * l(P); a pair with a point at infinity contributes 1: its line is replaced by 1 through selects
static ZK_NI Fq12 mul_line(const Fq12& f, const Line& l, const G1A& P, bool live) {
    const Fq2 d0 = fq2_mul_fq(l.c0, P.y), d1 = fq2_mul_fq(l.c1, P.x);
    return f.mul_034(live ? d0 : Fq2::one(), live ? d1 : Fq2::zero(), live ? l.c2 : Fq2::zero());
}
ZK_HD Fq2 twist_b3() {
    const Fq2 b = fq2_from_words(TWIST_B);
    return b.dbl() + b;
}
// pi(Q) and -pi^2(Q) on the twist
ZK_HD void twist_frobenius_pair(const G2A& Q, G2A& Q1, G2A& Q2) {
    const Fq2 gx = fq2_from_words(GAMMA_X), gy = fq2_from_words(GAMMA_Y);
    Q1 = G2A{fq2_conj(Q.x) * gx, fq2_conj(Q.y) * gy};
    Q2 = G2A{fq2_conj(Q1.x) * gx, -(fq2_conj(Q1.y) * gy)};
}
ZK_HD bool ate_bit(int i) { return (ATE_LOOP[i >> 5] >> (i & 31)) & 1; }
// lines of one Miller loop: one per doubling, one per set bit of 6u + 2 below the top, two for pi(Q) and -pi^2(Q)
constexpr int ate_line_count() {
    int n = 2;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) n += 1 + ((ATE_LOOP[i >> 5] >> (i & 31)) & 1);
    return n;
}
static constexpr int ATE_LINES = ate_line_count();

// fixed argument: the ATE_LINES lines of Q, computed once and evaluated at many P (ml_fixed)
ZK_HD void ml_lines(const G2A& Q, Line* out) {
    const Fq2 b3 = twist_b3();
    G2Proj T{Q.x, Q.y, Fq2::one()};
    int n = 0;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        out[n++] = dbl_step(T, b3);
        if (ate_bit(i)) out[n++] = add_step(T, Q);
    }
    G2A Q1, Q2;
    twist_frobenius_pair(Q, Q1, Q2);
    out[n++] = add_step(T, Q1);
    out[n++] = add_step(T, Q2);
}
// the Miller loop over Q's precomputed lines (live = false when P or Q is infinity)
ZK_HD Fq12 ml_fixed(const G1A& P, const Line* lines, bool live) {
    Fq12 f = Fq12::one();
    int n = 0;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        f = fq12_sqr_ni(f);
        f = mul_line(f, lines[n++], P, live);
        if (ate_bit(i)) f = mul_line(f, lines[n++], P, live);
    }
    f = mul_line(f, lines[n++], P, live);
    return mul_line(f, lines[n], P, live);
}
// the Miller loop with the steps computed on the fly
ZK_HD Fq12 ml_proj(const G1A& P, const G2A& Q) {
    const bool live = !P.is_inf() && !Q.is_inf();
    const Fq2 b3 = twist_b3();
    G2Proj T{Q.x, Q.y, Fq2::one()};
    Fq12 f = Fq12::one();
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        f = fq12_sqr_ni(f);
        f = mul_line(f, dbl_step(T, b3), P, live);
        if (ate_bit(i)) f = mul_line(f, add_step(T, Q), P, live);
    }
    G2A Q1, Q2;
    twist_frobenius_pair(Q, Q1, Q2);
    f = mul_line(f, add_step(T, Q1), P, live);
    return mul_line(f, add_step(T, Q2), P, live);
}

// ---- final exponentiation with the exact exponent (q^12 - 1) / r = (q^6 - 1)(q^2 + 1) * (q^4 - q^2 + 1) / r ----
ZK_HD Fq12 final_exp_easy(const Fq12& f) {
    const Fq12 t = fq12_mul_ni(f.conj(), f.inv());   // f^(q^6 - 1): in the cyclotomic subgroup from here on
    return fq12_mul_ni(t.frobenius(2), t);            // ^(q^2 + 1)
}
// g^((q^4 - q^2 + 1) / r) for g in the cyclotomic subgroup: left-to-right square-and-multiply over the fixed exponent
ZK_HD Fq12 final_exp_hard(const Fq12& g) {
    Fq12 acc = g;
    for (int i = HARD_EXP_BITS - 2; i >= 0; --i) {
        acc = fq12_cyc_sqr_ni(acc);
        if ((HARD_EXP[i >> 5] >> (i & 31)) & 1) acc = fq12_mul_ni(acc, g);
    }
    return acc;
}
ZK_HD Fq12 final_exp_exact(const Fq12& f) { return final_exp_hard(final_exp_easy(f)); }

}  // namespace zk
