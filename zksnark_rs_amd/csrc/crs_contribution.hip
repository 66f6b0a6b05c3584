// crs_contribution.hip -- the host side of a delta contribution (crs_contribute.hip has the device side): the one scalar of
// k_g1_scale prepared once (GLV split, width-4 non-adjacent forms), and the contribution record -- a Schnorr proof of knowledge of
// the factor d with delta' = d delta, bound to a caller's 32-byte tag:
//   T = k delta_before,  c = SHA-256("ZKCONTRv1\0" | tag | delta_before | delta_after | T) as a big-endian integer mod r,
//   z = k + c d mod r;   accepted iff z delta_before = T + c delta_after.
// Nothing in this file needs a context or a device (as vk.hip); tests/cpp/crs_contribution_host.hip compiles it alone for the host
// under the sanitizers.
#include <random>
#include "crs_contribution.hpp"
#include "pairing.cuh"
#include "sha256.hpp"

namespace zk {

// ---- k = k1 + k2 lambda: gbasis.hip's glv_split on the host, with nearest rounding (constants derived and checked by tools/glv_constants.py) ----
namespace {
const uint32_t H_GLV_G1[5] = {0x00ff6565u, 0x5398fd03u, 0xa773d2d2u, 0x4ccef014u, 0x00000002u};   // floor(2^256 b2 / r)
const uint32_t H_GLV_G2[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u};                             // floor(2^256 (-b1) / r)
const uint32_t H_GLV_A1[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};
const uint32_t H_GLV_NB1[2] = {0x94d213e3u, 0x89d32568u};                                          // -b1 = a2
const uint32_t H_GLV_B2[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};

// out[0 .. no) = words skip .. of a[0 .. na) * b[0 .. nb); with `round`, of the product plus half a unit of word `skip` (nearest)
void mp_mul_host(const uint32_t* a, int na, const uint32_t* b, int nb, int skip, uint32_t* out, int no, bool round = false) {
    uint32_t prod[16] = {0};
    for (int i = 0; i < na; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < nb; ++j) {
            c += (uint64_t)a[i] * b[j] + prod[i + j];
            prod[i + j] = (uint32_t)c;
            c >>= 32;
        }
        prod[i + nb] = (uint32_t)c;
    }
    if (round) {
        uint64_t c = 0x80000000u;
        for (int i = skip - 1; i < na + nb && c; ++i) { c += prod[i]; prod[i] = (uint32_t)c; c >>= 32; }
    }
    for (int i = 0; i < no; ++i) out[i] = skip + i < na + nb ? prod[skip + i] : 0;
}
}  // namespace

void glv_split_host(const uint32_t k[8], uint32_t k1[5], bool& neg1, uint32_t k2[5], bool& neg2) {
    uint32_t c1[5], c2[3], t1[6], t2[6], t3[6], t4[6], r1[6], r2[6];
    // gbasis.hip takes the floors; here the quotients are rounded to NEAREST, c_i = floor(k g_i / 2^256 + 1 / 2): both halves then come
    // out with either sign and |k1|, |k2| < 2^127 + 2^65 (half the basis vectors' sum, plus the roundings' error of at most one)
    mp_mul_host(k, 8, H_GLV_G1, 5, 8, c1, 5, true);   // c1 < 2^128
    mp_mul_host(k, 8, H_GLV_G2, 3, 8, c2, 3, true);   // c2 < 2^65
    // modulo 2^192 (the results fit 129 signed bits):  k1 = k - c1 a1 - c2 a2,  k2 = c1 (-b1) - c2 b2,  a2 = -b1
    mp_mul_host(c1, 5, H_GLV_A1, 4, 0, t1, 6);
    mp_mul_host(c2, 3, H_GLV_NB1, 2, 0, t2, 6);
    mp_mul_host(c1, 5, H_GLV_NB1, 2, 0, t3, 6);
    mp_mul_host(c2, 3, H_GLV_B2, 4, 0, t4, 6);
    int64_t br = 0;
    for (int i = 0; i < 6; ++i) { const int64_t v = (int64_t)k[i] - t1[i] - t2[i] + br; r1[i] = (uint32_t)v; br = v >> 32; }
    br = 0;
    for (int i = 0; i < 6; ++i) { const int64_t v = (int64_t)t3[i] - t4[i] + br; r2[i] = (uint32_t)v; br = v >> 32; }
    neg1 = (r1[5] >> 31) != 0;
    neg2 = (r2[5] >> 31) != 0;
    uint64_t c = neg1 ? 1 : 0;
    for (int i = 0; i < 6; ++i) { c += neg1 ? (uint32_t)~r1[i] : r1[i]; if (i < 5) k1[i] = (uint32_t)c; else ZK_REQUIRE((uint32_t)c == 0, ZK_ERR_SIZE, "glv_split: |k1| >= 2^160"); c >>= 32; }
    c = neg2 ? 1 : 0;
    for (int i = 0; i < 6; ++i) { c += neg2 ? (uint32_t)~r2[i] : r2[i]; if (i < 5) k2[i] = (uint32_t)c; else ZK_REQUIRE((uint32_t)c == 0, ZK_ERR_SIZE, "glv_split: |k2| >= 2^160"); c >>= 32; }
}

// width-4 non-adjacent form of the magnitude m (5 words), digits negated when `neg`: while m != 0, an odd m gives the digit
// m mods 16 in [-7, 7] (odd) and m -= digit, which clears the low four bits; then m /= 2.  Returns the number of digits written.
static int wnaf4(const uint32_t m5[5], bool neg, int8_t* digits) {
    uint32_t m[6] = {m5[0], m5[1], m5[2], m5[3], m5[4], 0};
    int len = 0;
    for (int i = 0; i < SC_DIGITS; ++i) digits[i] = 0;
    auto nonzero = [&] { return (m[0] | m[1] | m[2] | m[3] | m[4] | m[5]) != 0; };
    for (int i = 0; nonzero(); ++i) {
        ZK_REQUIRE(i < SC_DIGITS, ZK_ERR_SIZE, "scalar_recode: more digits than the kernel takes");
        if (m[0] & 1) {
            int d = (int)(m[0] & 15u);
            if (d >= 8) d -= 16;
            digits[i] = (int8_t)(neg ? -d : d);
            // m -= d: d > 0 clears the low bits in place; d < 0 adds |d| with a carry
            if (d > 0) m[0] -= (uint32_t)d;
            else {
                uint64_t c = (uint64_t)(-d);
                for (int w = 0; w < 6 && c; ++w) { c += m[w]; m[w] = (uint32_t)c; c >>= 32; }
            }
            len = i + 1;
        }
        for (int w = 0; w < 5; ++w) m[w] = (m[w] >> 1) | (m[w + 1] << 31);
        m[5] >>= 1;
    }
    return len;
}

void scalar_recode(const uint32_t k[8], ScaleDigits& out) {
    uint32_t k1[5], k2[5];
    bool n1, n2;
    glv_split_host(k, k1, n1, k2, n2);
    const int l1 = wnaf4(k1, n1, out.d1), l2 = wnaf4(k2, n2, out.d2);
    out.top = (l1 > l2 ? l1 : l2) - 1;
    wipe(k1, sizeof(k1));
    wipe(k2, sizeof(k2));
}

void wipe(void* p, size_t bytes) {
    volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
    for (size_t i = 0; i < bytes; ++i) v[i] = 0;
}

Fr draw_scalar_nonzero() {
    std::random_device rd;
    for (;;) {
        Fr x;
        for (int i = 0; i < 8; ++i) x.l[i] = (uint32_t)rd();
        while (!x.raw_in_range()) {           // 2^256 < 6 r
            uint64_t borrow = 0;
            for (int i = 0; i < 8; ++i) {
                const uint64_t d = (uint64_t)x.l[i] - FrParams::P[i] - borrow;
                x.l[i] = (uint32_t)d;
                borrow = (d >> 32) & 1;
            }
        }
        if (!x.is_zero()) return x;
    }
}

// ---- the record ----
namespace {

Fr fr_words(const uint64_t* w) {
    Fr x;
    for (int i = 0; i < 4; ++i) { x.l[2 * i] = (uint32_t)w[i]; x.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return x;
}
void fr_to_words(const Fr& x, uint64_t* w) {
    for (int i = 0; i < 4; ++i) w[i] = (uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32);
}
void g1_to_words(const G1A& p, uint64_t* w) {   // Montgomery -> canonical words; infinity = zeros
    const Fq x = p.x.to_canonical(), y = p.y.to_canonical();
    for (int i = 0; i < 4; ++i) {
        w[i] = (uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32);
        w[4 + i] = (uint64_t)y.l[2 * i] | ((uint64_t)y.l[2 * i + 1] << 32);
    }
}
// a point enters the hash as its 64 bytes: the eight canonical little-endian words, x then y
void hash_point(Sha256& h, const uint64_t* w) {
    uint8_t b[64];
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) b[8 * i + j] = (uint8_t)(w[i] >> (8 * j));
    h.update(b, 64);
}
Fr challenge_of(const uint8_t tag[32], const uint64_t* before, const uint64_t* after, const uint64_t* commit) {
    static const uint8_t zero_tag[32] = {0};
    Sha256 h;
    h.update("ZKCONTRv1", 10);   // with its terminating zero
    h.update(tag ? tag : zero_tag, 32);
    hash_point(h, before);
    hash_point(h, after);
    hash_point(h, commit);
    uint8_t dg[32];
    h.finish(dg);
    Fr c;   // big-endian integer -> little-endian words, reduced mod r (2^256 < 6 r)
    for (int i = 0; i < 8; ++i)
        c.l[i] = ((uint32_t)dg[28 - 4 * i] << 24) | ((uint32_t)dg[29 - 4 * i] << 16) | ((uint32_t)dg[30 - 4 * i] << 8) | dg[31 - 4 * i];
    while (!c.raw_in_range()) {
        uint64_t borrow = 0;
        for (int i = 0; i < 8; ++i) {
            const uint64_t d = (uint64_t)c.l[i] - FrParams::P[i] - borrow;
            c.l[i] = (uint32_t)d;
            borrow = (d >> 32) & 1;
        }
    }
    return c;
}
G1A g1_mul_host(const G1A& p, const Fr& k_can) { return jac_to_affine(jac_mul_words(G1J::from_affine(p), k_can.l)); }

}  // namespace

// false: delta_before is out of range, off the curve or infinity.  d and the nonce are canonical and below r (the caller checked).
bool contribution_prove(const uint64_t delta_before[8], const Fr& d_can, const Fr& nonce_can, const uint8_t tag[32], zk_crs_contribution* out) {
    G1A before;
    if (!rd_g1(delta_before, before) || before.is_inf()) return false;
    zk_crs_contribution c;
    std::memcpy(c.delta_before_g1, delta_before, sizeof(c.delta_before_g1));
    g1_to_words(g1_mul_host(before, d_can), c.delta_after_g1);
    g1_to_words(g1_mul_host(before, nonce_can), c.commit_g1);
    const Fr ch = challenge_of(tag, c.delta_before_g1, c.delta_after_g1, c.commit_g1);
    Fr z = (Fr::from_canonical(nonce_can) + Fr::from_canonical(ch) * Fr::from_canonical(d_can)).to_canonical();
    fr_to_words(z, c.response);
    wipe(&z, sizeof(z));
    *out = c;
    return true;
}

bool contribution_verify(const zk_crs_contribution& c, const uint8_t tag[32]) {
    G1A before, after, commit;
    if (!rd_g1(c.delta_before_g1, before) || !rd_g1(c.delta_after_g1, after) || !rd_g1(c.commit_g1, commit)) return false;
    if (before.is_inf() || after.is_inf()) return false;
    const Fr z = fr_words(c.response);
    if (!z.raw_in_range()) return false;
    const Fr ch = challenge_of(tag, c.delta_before_g1, c.delta_after_g1, c.commit_g1);
    const G1A lhs = g1_mul_host(before, z);
    const G1A rhs = jac_to_affine(jac_add(G1J::from_affine(commit), jac_mul_words(G1J::from_affine(after), ch.l)));
    return lhs.x == rhs.x && lhs.y == rhs.y;
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_crs_contribution_prove(const uint64_t delta_before_g1[8], const uint64_t d[4], const uint64_t nonce[4], const uint8_t tag[32],
                              zk_crs_contribution* out) {
    if (!delta_before_g1 || !d || !out) return ZK_ERR_ARG;
    Fr dc = fr_words(d);
    if (!dc.raw_in_range()) return ZK_ERR_RANGE;
    if (dc.is_zero()) return ZK_ERR_DIV_BY_ZERO;
    Fr k;
    if (nonce) {
        k = fr_words(nonce);
        if (!k.raw_in_range()) return ZK_ERR_RANGE;
    } else {
        k = draw_scalar_nonzero();
    }
    const bool ok = contribution_prove(delta_before_g1, dc, k, tag, out);
    wipe(&dc, sizeof(dc));
    wipe(&k, sizeof(k));
    return ok ? ZK_OK : ZK_ERR_RANGE;
}

int zk_crs_contribution_verify(const zk_crs_contribution* c, const uint8_t tag[32], int* ok) {
    if (!c || !ok) return ZK_ERR_ARG;
    *ok = contribution_verify(*c, tag) ? 1 : 0;
    return ZK_OK;
}

}  // extern "C"
