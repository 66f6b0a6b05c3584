// eddsa_modl.hpp -- arithmetic mod the order l of Base8 (251 bits) on limbs of 32 bits, least significant first, for the signing
// kernels of eddsa.hip: every function is ZK_HD, so tests/cpp/eddsa_modl_check.hip runs the same text on the host and in a kernel.
//   modl_reduce_r      x mod l for x < 8 l -- every x < r, since 7 l < r < 8 l: three conditional subtractions, of 4 l, 2 l and l
//   modl_reduce_wide   x mod l for x < 2^512 by Barrett's reduction (Handbook of Applied Cryptography 14.42 with b = 2^32, k = 8):
//                      q3 = floor(floor(x / b^7) mu / b^9) with mu = floor(b^16 / l) satisfies q - 2 <= q3 <= q for q = floor(x / l), so
//                      x - q3 l lies in [0, 3 l) and two conditional subtractions of l finish.  3 l < 2^253 < b^8, so the difference is
//                      taken mod b^8 and nothing above limb 7 of q3 l is computed.
//   modl_response      (rho + 8 (h mod l) k) mod l for h < 8 l and any rho, k below 2^256: 8 (h mod l) k + rho < 2^510 + 2^256 < 2^512
// Nothing here branches on or indexes by a value: a conditional subtraction computes the difference and selects limb by limb, and every
// loop has constant bounds.  The constants come from modl_consts() at compile time: l is typed once below (the words of BABYJUB_ORDER),
// 2 l and 4 l are shifts of it and mu comes from a long division; tests/test_eddsa_modl.py holds all four against Python integers.
#pragma once
#include "ff.cuh"

namespace zk {

struct ModlConsts {
    uint32_t l[8], l2[8], l4[8];   // l, 2 l, 4 l
    uint32_t mu[9];                // floor(2^512 / l), 262 bits
};
constexpr ModlConsts modl_consts() {
    constexpr uint32_t L[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
    ModlConsts c{};
    for (int i = 0; i < 8; ++i) {
        c.l[i] = L[i];
        c.l2[i] = (L[i] << 1) | (i ? L[i - 1] >> 31 : 0u);
        c.l4[i] = (L[i] << 2) | (i ? L[i - 1] >> 30 : 0u);
    }
    // 2^512 / l, one bit at a time: the remainder stays below l, so twice it plus one fits 9 limbs with room to spare
    uint32_t rem[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int bit = 512; bit >= 0; --bit) {
        for (int i = 8; i > 0; --i) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 31);
        rem[0] = (rem[0] << 1) | (bit == 512 ? 1u : 0u);
        uint32_t d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t borrow = 0;
        for (int i = 0; i < 9; ++i) {
            const uint64_t t = (uint64_t)rem[i] - (i < 8 ? L[i] : 0u) - borrow;
            d[i] = (uint32_t)t;
            borrow = t >> 63;
        }
        if (!borrow) {
            for (int i = 0; i < 9; ++i) rem[i] = d[i];
            if (bit < 288) c.mu[bit >> 5] |= 1u << (bit & 31);
        }
    }
    return c;
}
static_assert(modl_consts().l[7] >> 26 == 1 && modl_consts().l4[7] >> 28 == 1, "l has 251 bits: 4 l fits 8 limbs");
static_assert(modl_consts().mu[8] >> 5 == 1, "floor(2^512 / l) has 262 bits");

// x = x - m where x >= m, x otherwise: the same instructions either way
ZK_HD void modl_cond_sub(uint32_t (&x)[8], const uint32_t (&m)[8]) {
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)x[i] - m[i] - borrow;
        d[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = borrow ? x[i] : d[i];
}
// x < 8 l -> x mod l
ZK_HD void modl_reduce_r(uint32_t (&x)[8]) {
    constexpr ModlConsts C = modl_consts();
    modl_cond_sub(x, C.l4);
    modl_cond_sub(x, C.l2);
    modl_cond_sub(x, C.l);
}
// x < 2^512 -> x mod l
ZK_HD void modl_reduce_wide(const uint32_t (&x)[16], uint32_t (&out)[8]) {
    constexpr ModlConsts C = modl_consts();
    uint32_t q2[18];                // floor(x / b^7) mu: 9 x 9 limbs
#pragma unroll
    for (int i = 0; i < 18; ++i) q2[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint64_t t = (uint64_t)x[7 + i] * C.mu[j] + q2[i + j] + carry;
            q2[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        q2[i + 9] = (uint32_t)carry;
    }
    uint32_t p[8];                  // q3 l mod b^8, q3 = limbs 9..17 of q2 (limb 17 multiplies b^8 and drops out)
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8 - i; ++j) {
            const uint64_t t = (uint64_t)q2[9 + i] * C.l[j] + p[i + j] + carry;
            p[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = (uint64_t)x[i] - p[i] - borrow;
        out[i] = (uint32_t)t;
        borrow = (uint32_t)(t >> 63);
    }
    modl_cond_sub(out, C.l);
    modl_cond_sub(out, C.l);
}
// (rho + 8 (h mod l) k) mod l, h < 8 l
ZK_HD void modl_response(const uint32_t (&rho)[8], const uint32_t (&h)[8], const uint32_t (&k)[8], uint32_t (&out)[8]) {
    uint32_t h1[8], x[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) h1[i] = h[i];
    modl_reduce_r(h1);
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t t = (uint64_t)h1[i] * k[j] + x[i + j] + carry;
            x[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        x[i + 8] = (uint32_t)carry;
    }
#pragma unroll
    for (int i = 15; i > 0; --i) x[i] = (x[i] << 3) | (x[i - 1] >> 29);
    x[0] <<= 3;
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint64_t t = (uint64_t)x[i] + (i < 8 ? rho[i] : 0u) + carry;
        x[i] = (uint32_t)t;
        carry = t >> 32;
    }
    modl_reduce_wide(x, out);
}

}  // namespace zk
