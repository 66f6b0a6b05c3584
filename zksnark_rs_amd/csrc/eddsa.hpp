// eddsa.hpp -- EdDSA-Poseidon on Baby Jubjub on the host (include/zkgpu.h, "EdDSA-Poseidon", states the scheme): the challenge hash H6,
// Poseidon of width 6 (poseidon.hpp: poseidon_params_t6), arithmetic mod the subgroup order l, key derivation, signing and
// verification.  With A = [k] Base8:
//   sign      rho = H6(n, M, 0, 0, 0) mod l, R8 = [rho] Base8, hm = H6(R8.x, R8.y, A.x, A.y, M), S = (rho + 8 hm k) mod l
//   verify    [S] Base8 = R8 + [8] ([hm] A), hm as the full integer below r; the two sides stay projective and are compared by cross
//             multiplication, so nothing is inverted
// 8 hm can reach 2^257 and is never a scalar: [hm] A is doubled three times.  Arithmetic mod l is written plainly: a 256 x 256 -> 512
// bit schoolbook product and a reduction by shift and subtract, one bit at a time.  Header-only and free of device code, like
// babyjub.hpp: tests/cpp/eddsa_host.hip compiles it alone under the sanitizers.  No context.
#pragma once
#include "babyjub.hpp"
#include "poseidon.hpp"

namespace zk {

// ---- integers of 4 and 8 words of 64 bits, least significant first --------------------------------
static inline bool u256_less(const uint64_t* a, const uint64_t* b) {
    for (int i = 3; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
static inline bool u256_is_zero(const uint64_t* a) { return !(a[0] | a[1] | a[2] | a[3]); }
// x mod l for x of 512 bits: the remainder stays below l < 2^251, so doubling it and adding a bit fits 4 words
static inline void eddsa_mod_l(const uint64_t x[8], uint64_t out[4]) {
    uint64_t rem[4] = {0, 0, 0, 0};
    for (int bit = 511; bit >= 0; --bit) {
        for (int i = 3; i > 0; --i) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
        rem[0] = (rem[0] << 1) | ((x[bit >> 6] >> (bit & 63)) & 1);
        if (!u256_less(rem, BABYJUB_ORDER)) {
            unsigned __int128 borrow = 0;
            for (int i = 0; i < 4; ++i) {
                const unsigned __int128 d = (unsigned __int128)rem[i] - BABYJUB_ORDER[i] - borrow;
                rem[i] = (uint64_t)d;
                borrow = (uint64_t)(d >> 64) & 1;
            }
        }
    }
    for (int i = 0; i < 4; ++i) out[i] = rem[i];
}
static inline void u256_mul(const uint64_t a[4], const uint64_t b[4], uint64_t out[8]) {
    for (int i = 0; i < 8; ++i) out[i] = 0;
    for (int i = 0; i < 4; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; ++j) {
            const unsigned __int128 t = (unsigned __int128)a[i] * b[j] + out[i + j] + carry;
            out[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        out[i + 4] = carry;
    }
}
// (rho + 8 h k) mod l for rho, k < l and any h of 256 bits: h is reduced first, so 8 (h mod l) k + rho < 2^506
static inline void eddsa_response(const uint64_t rho[4], const uint64_t h[4], const uint64_t k[4], uint64_t out[4]) {
    uint64_t wide[8] = {h[0], h[1], h[2], h[3], 0, 0, 0, 0}, h1[4], prod[8];
    eddsa_mod_l(wide, h1);
    u256_mul(h1, k, prod);
    for (int i = 7; i > 0; --i) prod[i] = (prod[i] << 3) | (prod[i - 1] >> 61);
    prod[0] <<= 3;
    unsigned __int128 carry = 0;
    for (int i = 0; i < 8; ++i) {
        const unsigned __int128 t = (unsigned __int128)prod[i] + (i < 4 ? rho[i] : 0) + carry;
        prod[i] = (uint64_t)t;
        carry = t >> 64;
    }
    eddsa_mod_l(prod, out);
}
// zeroes memory in a way the optimiser keeps
static inline void eddsa_wipe(void* p, size_t bytes) {
    volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
    for (size_t i = 0; i < bytes; ++i) v[i] = 0;
}

// ---- H6 ----------------------------------------------------------------------------------------------
static inline Fr eddsa_h6(const Fr in[5]) { return poseidon_hash_mont(poseidon_params_t6(), in); }
// canonical words below r -> Montgomery form; false for a word pattern >= r
static inline bool eddsa_read(const uint64_t* w, Fr& out) {
    const Fr x = fr_from_words(w);
    if (!x.raw_in_range()) return false;
    out = Fr::from_canonical(x);
    return true;
}
static inline void u256_to_u32(const uint64_t* w, uint32_t s[8]) {
    for (int i = 0; i < 4; ++i) { s[2 * i] = (uint32_t)w[i]; s[2 * i + 1] = (uint32_t)(w[i] >> 32); }
}

// ---- the context-free entry points of include/zkgpu.h ------------------------------------------------
// H6(R8.x, R8.y, A.x, A.y, M): a range check and no curve check
static inline int eddsa_challenge_words(const uint64_t* r8, const uint64_t* a, const uint64_t* msg, uint64_t* out) {
    if (!r8 || !a || !msg || !out) return ZK_ERR_ARG;
    Fr in[5];
    if (!eddsa_read(r8, in[0]) || !eddsa_read(r8 + 4, in[1]) || !eddsa_read(a, in[2]) || !eddsa_read(a + 4, in[3]) || !eddsa_read(msg, in[4]))
        return ZK_ERR_RANGE;
    fr_to_words(eddsa_h6(in).to_canonical(), out);
    return ZK_OK;
}
static inline bool eddsa_key_ok(const uint64_t* k) { return !u256_is_zero(k) && u256_less(k, BABYJUB_ORDER); }
static inline int eddsa_public_key_words(const uint64_t* k, uint64_t* out) {
    if (!k || !out) return ZK_ERR_ARG;
    if (!eddsa_key_ok(k)) return ZK_ERR_RANGE;
    uint32_t s[8];
    u256_to_u32(k, s);
    babyjub_write(bj_to_affine(babyjub_mul(babyjub_consts(), s, babyjub_base8())), out);
    eddsa_wipe(s, sizeof(s));
    return ZK_OK;
}
static inline int eddsa_sign_words(const uint64_t* k, const uint64_t* nonce_key, const uint64_t* msg, uint64_t* r8_out, uint64_t* s_out) {
    if (!k || !nonce_key || !msg || !r8_out || !s_out) return ZK_ERR_ARG;
    Fr in[5] = {Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero(), Fr::zero()}, m;
    if (!eddsa_key_ok(k) || !eddsa_read(nonce_key, in[0]) || !eddsa_read(msg, m)) {
        eddsa_wipe(in, sizeof(in));
        return ZK_ERR_RANGE;
    }
    in[1] = m;
    const BjConsts c = babyjub_consts();
    const BjAffine base = babyjub_base8();
    uint64_t wide[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rho[4], h[4];
    uint32_t s[8];
    fr_to_words(eddsa_h6(in).to_canonical(), wide);
    eddsa_mod_l(wide, rho);
    u256_to_u32(rho, s);
    const BjAffine r8 = bj_to_affine(babyjub_mul(c, s, base));
    u256_to_u32(k, s);
    const BjAffine a = bj_to_affine(babyjub_mul(c, s, base));
    const Fr ch[5] = {r8.x, r8.y, a.x, a.y, m};
    fr_to_words(eddsa_h6(ch).to_canonical(), h);
    eddsa_response(rho, h, k, s_out);
    babyjub_write(r8, r8_out);
    eddsa_wipe(in, sizeof(in));
    eddsa_wipe(wide, sizeof(wide));
    eddsa_wipe(rho, sizeof(rho));
    eddsa_wipe(s, sizeof(s));
    return ZK_OK;
}
// the verdict of one signature: ZK_EDDSA_*, the lowest applicable
static inline int eddsa_status(const uint64_t* a, const uint64_t* msg, const uint64_t* r8, const uint64_t* s) {
    Fr ax, ay, rx, ry, m, sv;
    if (!eddsa_read(a, ax) || !eddsa_read(a + 4, ay) || !eddsa_read(r8, rx) || !eddsa_read(r8 + 4, ry) || !eddsa_read(msg, m) || !eddsa_read(s, sv))
        return ZK_EDDSA_RANGE;
    const BjConsts c = babyjub_consts();
    if (!bj_on_curve(c, ax, ay)) return ZK_EDDSA_KEY_OFF_CURVE;
    if (!bj_on_curve(c, rx, ry)) return ZK_EDDSA_R_OFF_CURVE;
    if (!u256_less(s, BABYJUB_ORDER)) return ZK_EDDSA_S_RANGE;
    const Fr ch[5] = {rx, ry, ax, ay, m};
    uint64_t h[4];
    fr_to_words(eddsa_h6(ch).to_canonical(), h);
    uint32_t w[8];
    u256_to_u32(h, w);
    BjPoint right = babyjub_mul(c, w, BjAffine{ax, ay});
    for (int i = 0; i < 3; ++i) right = bj_dbl(c, right);
    right = bj_add_mixed(c, right, rx, ry);
    u256_to_u32(s, w);
    const BjPoint left = babyjub_mul(c, w, babyjub_base8());
    return left.X * right.Z == right.X * left.Z && left.Y * right.Z == right.Y * left.Z ? ZK_EDDSA_VALID : ZK_EDDSA_MISMATCH;
}
static inline int eddsa_verify_words(const uint64_t* a, const uint64_t* msg, const uint64_t* r8, const uint64_t* s, int* status) {
    if (!a || !msg || !r8 || !s || !status) return ZK_ERR_ARG;
    *status = eddsa_status(a, msg, r8, s);
    return ZK_OK;
}
// the parameters of width 6 as canonical words: 408 round constants, 36 matrix entries (the test hook behind zk_eddsa_challenge's
// constants; not part of the C ABI)
static inline void eddsa_h6_params_words(uint64_t* round_constants, uint64_t* mds) {
    const PoseidonParams& p = poseidon_params_t6();
    for (size_t i = 0; i < p.c.size(); ++i) fr_to_words(p.c[i].to_canonical(), round_constants + 4 * i);
    for (size_t i = 0; i < p.m.size(); ++i) fr_to_words(p.m[i].to_canonical(), mds + 4 * i);
}

}  // namespace zk
