// babyjub.hpp -- Baby Jubjub on the host: the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over the BN254 scalar field Fr with
// a = 168700, d = 168696 (circomlib, iden3, Semaphore).  The identity is (0, 1); Base8 generates the subgroup of prime order l
// (251 bits), Generator the whole group of order 8 l, Base8 = 8 Generator.  a is a square and d is not, so the addition law is complete:
// no denominator vanishes for any two curve points, the ones of low order included, and nothing here has a special case.
//
// Points are computed in projective coordinates (X : Y : Z), x = X / Z, y = Y / Z, with add-2008-bbjlp and dbl-2008-bbjlp for general a:
//   add   A = Z1 Z2, B = A^2, C = X1 X2, D = Y1 Y2, E = C D, H = (X1 + Y1)(X2 + Y2), F = B - d E, G = B + d E,
//         X3 = (A F)(H - C - D), Y3 = (A G)(D - a C), Z3 = F G                          13 multiplications, 12 when Z2 = 1
//   dbl   B = (X + Y)^2, C = X^2, D = Y^2, E = a C, F = E + D, H = Z^2, J = F - 2 H,
//         X3 = (B - C - D) J, Y3 = F (E - D), Z3 = F J                                   8 multiplications
// Z3 of a sum is (1 - t)(1 + t) Z1^2 Z2^2 with t = d x1 x2 y1 y2, never 0 on curve points.  The same code compiles for the device
// (babyjub.hip).  Header-only; the host part is free of device code, so tests/cpp/babyjub_host.hip compiles it alone under the
// sanitizers.
#pragma once
#include <vector>
#include "witgen_tape.hpp"

namespace zk {

constexpr uint32_t BABYJUB_A = 168700, BABYJUB_D = 168696;
// canonical words, least significant first
static const uint64_t BABYJUB_BASE8[8] = {0x2893f3f6bb957051ull, 0x2ab8d8010534e0b6ull, 0x4eacb2e09d6277c1ull, 0x0bb77a6ad63e739bull,
                                          0x4b3c257a872d7d8bull, 0xfce0051fb9e13377ull, 0x25572e1cd16bf9edull, 0x25797203f7a0b249ull};
static const uint64_t BABYJUB_GENERATOR[8] = {0x40f41a59f4d4b45eull, 0xb494b1255b1162bbull, 0x38bcba38f25645adull, 0x023343e3445b673dull,
                                              0x50f87d64fc000001ull, 0x4a0cfa121e6e5c24ull, 0x6e14116da0605617ull, 0x0c19139cb84c680aull};
static const uint64_t BABYJUB_ORDER[4] = {0x677297dc392126f1ull, 0xab3eedb83920ee0aull, 0x370a08b6d0302b0bull, 0x060c89ce5c263405ull};

// coordinates in Montgomery form
struct BjAffine { Fr x, y; };
struct BjPoint {
    Fr X, Y, Z;
    ZK_HD static BjPoint identity() { return BjPoint{Fr::zero(), Fr::one(), Fr::one()}; }
};

// a and d in Montgomery form travel as arguments: the device keeps them in scalar registers
struct BjConsts { Fr a, d; };
static inline BjConsts babyjub_consts() { return BjConsts{Fr::from_u32(BABYJUB_A), Fr::from_u32(BABYJUB_D)}; }

ZK_HD bool bj_on_curve(const BjConsts& k, const Fr& x, const Fr& y) {
    const Fr u = x.sqr(), v = y.sqr();
    return k.a * u + v == Fr::one() + k.d * (u * v);
}
ZK_HD BjPoint bj_add(const BjConsts& k, const BjPoint& p, const BjPoint& q) {
    const Fr A = p.Z * q.Z, B = A.sqr(), C = p.X * q.X, D = p.Y * q.Y;
    const Fr E = k.d * (C * D), H = (p.X + p.Y) * (q.X + q.Y);
    const Fr F = B - E, G = B + E;
    return BjPoint{(A * F) * (H - C - D), (A * G) * (D - k.a * C), F * G};
}
// q affine: Z2 = 1
ZK_HD BjPoint bj_add_mixed(const BjConsts& k, const BjPoint& p, const Fr& x2, const Fr& y2) {
    const Fr B = p.Z.sqr(), C = p.X * x2, D = p.Y * y2;
    const Fr E = k.d * (C * D), H = (p.X + p.Y) * (x2 + y2);
    const Fr F = B - E, G = B + E;
    return BjPoint{(p.Z * F) * (H - C - D), (p.Z * G) * (D - k.a * C), F * G};
}
ZK_HD BjPoint bj_dbl(const BjConsts& k, const BjPoint& p) {
    const Fr B = (p.X + p.Y).sqr(), C = p.X.sqr(), D = p.Y.sqr(), E = k.a * C;
    const Fr F = E + D, J = F - p.Z.sqr().dbl();
    return BjPoint{(B - C - D) * J, F * (E - D), F * J};
}
ZK_HD BjAffine bj_to_affine(const BjPoint& p) {
    const Fr zi = p.Z.inv();
    return BjAffine{p.X * zi, p.Y * zi};
}

// [scalar] p for any integer below 2^256 (8 words of 32 bits, least significant first), most significant bit first
static inline BjPoint babyjub_mul(const BjConsts& k, const uint32_t scalar[8], const BjAffine& p) {
    BjPoint acc = BjPoint::identity();
    for (int i = 255; i >= 0; --i) {
        acc = bj_dbl(k, acc);
        if ((scalar[i >> 5] >> (i & 31)) & 1) acc = bj_add_mixed(k, acc, p.x, p.y);
    }
    return acc;
}
static inline BjAffine babyjub_base8() {
    return BjAffine{Fr::from_canonical(fr_from_words(BABYJUB_BASE8)), Fr::from_canonical(fr_from_words(BABYJUB_BASE8 + 4))};
}

// The table of the fixed-base kernel and of zk_builder_babyjub_mul_fixed: entry (k, j) = j 2^(window k) Base8, affine, Montgomery form,
// for k < windows and j < 2^window; j = 0 is the identity.
static inline std::vector<BjAffine> babyjub_window_table(unsigned window, unsigned windows) {
    const BjConsts k = babyjub_consts();
    std::vector<BjAffine> t;
    t.reserve((size_t)windows << window);
    BjAffine base = babyjub_base8();
    for (unsigned w = 0; w < windows; ++w) {
        BjPoint acc = BjPoint::identity();
        for (unsigned j = 0; j < (1u << window); ++j) {
            t.push_back(bj_to_affine(acc));
            acc = bj_add_mixed(k, acc, base.x, base.y);
        }
        base = bj_to_affine(acc);   // 2^window times the window's base
    }
    return t;
}

// ---- the context-free entry points of include/zkgpu.h ------------------------------------------
// 8 canonical words -> a point; ZK_ERR_RANGE for a coordinate >= r and, with `check`, for a point off the curve
static inline int babyjub_read(const uint64_t* w, BjAffine& out, bool check = true) {
    const Fr x = fr_from_words(w), y = fr_from_words(w + 4);
    if (!x.raw_in_range() || !y.raw_in_range()) return ZK_ERR_RANGE;
    out = BjAffine{Fr::from_canonical(x), Fr::from_canonical(y)};
    if (check && !bj_on_curve(babyjub_consts(), out.x, out.y)) return ZK_ERR_RANGE;
    return ZK_OK;
}
static inline void babyjub_write(const BjAffine& p, uint64_t* w) {
    fr_to_words(p.x.to_canonical(), w);
    fr_to_words(p.y.to_canonical(), w + 4);
}
static inline int babyjub_params_words(uint64_t* a, uint64_t* d, uint64_t* order, uint64_t* base8, uint64_t* generator) {
    if (a) { a[0] = BABYJUB_A; a[1] = a[2] = a[3] = 0; }
    if (d) { d[0] = BABYJUB_D; d[1] = d[2] = d[3] = 0; }
    for (int i = 0; i < 4; ++i) if (order) order[i] = BABYJUB_ORDER[i];
    for (int i = 0; i < 8; ++i) {
        if (base8) base8[i] = BABYJUB_BASE8[i];
        if (generator) generator[i] = BABYJUB_GENERATOR[i];
    }
    return ZK_OK;
}
// 1: on the curve, 0: off it
static inline int babyjub_on_curve_words(const uint64_t* p) {
    if (!p) return ZK_ERR_ARG;
    BjAffine a;
    const int rc = babyjub_read(p, a, false);
    if (rc != ZK_OK) return rc;
    return bj_on_curve(babyjub_consts(), a.x, a.y) ? 1 : 0;
}
static inline int babyjub_add_words(const uint64_t* p, const uint64_t* q, uint64_t* out) {
    if (!p || !q || !out) return ZK_ERR_ARG;
    BjAffine a, b;
    for (int pass = 0; pass < 2; ++pass) {   // a coordinate >= r in either operand comes before a point off the curve
        int rc = babyjub_read(p, a, pass != 0);
        if (rc == ZK_OK) rc = babyjub_read(q, b, pass != 0);
        if (rc != ZK_OK) return rc;
    }
    babyjub_write(bj_to_affine(bj_add_mixed(babyjub_consts(), BjPoint{a.x, a.y, Fr::one()}, b.x, b.y)), out);
    return ZK_OK;
}
static inline int babyjub_mul_words(const uint64_t* scalar, const uint64_t* p, uint64_t* out) {
    if (!scalar || !out) return ZK_ERR_ARG;
    BjAffine a = babyjub_base8();
    if (p) {
        const int rc = babyjub_read(p, a);
        if (rc != ZK_OK) return rc;
    }
    uint32_t s[8];
    for (int i = 0; i < 4; ++i) { s[2 * i] = (uint32_t)scalar[i]; s[2 * i + 1] = (uint32_t)(scalar[i] >> 32); }
    babyjub_write(bj_to_affine(babyjub_mul(babyjub_consts(), s, a)), out);
    return ZK_OK;
}

}  // namespace zk
