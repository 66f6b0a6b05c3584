// mul_each_recode.hpp -- the scalar side of k_mul_each (powers.hip), host and device code alike so that the host can test
// it (zk_lazy29_batch op ZK_LAZY_REGULAR_RECODE, tests/test_powers_recode_host.py).
//
//   split    k = k1 + k2 lambda, the quotients rounded to NEAREST as crs_contribution.hip's glv_split_host does (same constants,
//            tools/glv_constants.py): |k1|, |k2| < 2^127 + 2^65.  No branch, no table: every lane of a wave does the same work.
//   recode   a REGULAR signed fixed-window form of each magnitude m: ND digits of width W, EVERY digit odd and non-zero, so every
//            lane adds at the same ND positions and only the table index and the sign differ.  For an odd m < 2^(W ND)
//                b = (m + 2^(W ND) - 1) / 2 = (m >> 1) | 2^(W ND - 1),   b = sum_i b_i 2^(W i), 0 <= b_i < 2^W,
//                d_i = 2 b_i - (2^W - 1):   sum_i d_i 2^(W i) = 2 b - (2^(W ND) - 1) = m,   d_i odd, |d_i| <= 2^W - 1.
//            The digits are therefore the windows of b itself: the top bit of a window is the digit's sign (1: positive), the other
//            W - 1 bits are the index (|d_i| - 1) / 2 into the table of odd multiples -- complemented for a negative digit.  Nothing
//            is stored per digit: b sits in NW words, left-aligned, and every step takes the top window and shifts.
//   even, 0  an even magnitude (zero included) is recoded as m + 1; `even` tells the caller to subtract the point once at the end.
#pragma once
#include <stdint.h>
#include "ff.cuh"

namespace zk {

// the window widths of k_mul_each (powers.hip; DESIGN 4n has the reasons): G1 and G2
constexpr int ME_W_G1 = 4, ME_W_G2 = 3;

template <int W>
struct RegularRecode {
    static constexpr int ND = W == 4 ? 32 : (129 + W - 1) / W;   // digits a half: W ND >= 128 bits (W = 4: exactly 128)
    static constexpr int NW = (W * ND + 31) / 32;                // words of b
    static constexpr int PRE = 32 * NW - W * ND;                 // b is kept shifted left by this much: its top window tops the top word
};

namespace me_detail {
// out[0 .. NO) = words skip .. of a[0 .. NA) * b[0 .. NB); with `round`, of the product plus half a unit of word `skip`
template <int NA, int NB, int NO>
ZK_HD void mp_mul(const uint32_t* a, const uint32_t* b, int skip, bool round, uint32_t* out) {
    uint32_t prod[NA + NB];
#pragma unroll
    for (int i = 0; i < NA + NB; ++i) prod[i] = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            c += (uint64_t)a[i] * b[j] + prod[i + j];
            prod[i + j] = (uint32_t)c;
            c >>= 32;
        }
        prod[i + NB] = (uint32_t)c;
    }
    if (round) {
        uint64_t c = 0x80000000u;
#pragma unroll
        for (int i = 0; i < NA + NB; ++i)
            if (i >= skip - 1) { c += prod[i]; prod[i] = (uint32_t)c; c >>= 32; }
    }
#pragma unroll
    for (int i = 0; i < NO; ++i) out[i] = skip + i < NA + NB ? prod[skip + i] : 0;
}
}  // namespace me_detail

// |k1|, |k2| (5 words each; word 4 is zero for every k < r) and their signs.  k: canonical, 8 words.
ZK_HD void glv_split_nearest(const uint32_t* k, uint32_t* k1, bool& neg1, uint32_t* k2, bool& neg2) {
    const uint32_t g1[5] = {0x00ff6565u, 0x5398fd03u, 0xa773d2d2u, 0x4ccef014u, 0x00000002u};   // floor(2^256 b2 / r)
    const uint32_t g2[3] = {0xc7e0b3d7u, 0xd91d232eu, 0x00000002u};                             // floor(2^256 (-b1) / r)
    const uint32_t a1[4] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u};
    const uint32_t nb1[2] = {0x94d213e3u, 0x89d32568u};                                          // -b1 = a2
    const uint32_t b2[4] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u};
    uint32_t kw[8], c1[5], c2[3], t1[6], t2[6], t3[6], t4[6], r1[6], r2[6];
#pragma unroll
    for (int i = 0; i < 8; ++i) kw[i] = k[i];
    me_detail::mp_mul<8, 5, 5>(kw, g1, 8, true, c1);   // c1 = floor(k g1 / 2^256 + 1/2) < 2^128
    me_detail::mp_mul<8, 3, 3>(kw, g2, 8, true, c2);   // c2 < 2^65
    // modulo 2^192 (the results fit 129 signed bits):  k1 = k - c1 a1 - c2 a2,  k2 = c1 (-b1) - c2 b2,  a2 = -b1
    me_detail::mp_mul<5, 4, 6>(c1, a1, 0, false, t1);
    me_detail::mp_mul<3, 2, 6>(c2, nb1, 0, false, t2);
    me_detail::mp_mul<5, 2, 6>(c1, nb1, 0, false, t3);
    me_detail::mp_mul<3, 4, 6>(c2, b2, 0, false, t4);
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { const int64_t v = (int64_t)kw[i] - t1[i] - t2[i] + br; r1[i] = (uint32_t)v; br = v >> 32; }
    br = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { const int64_t v = (int64_t)t3[i] - t4[i] + br; r2[i] = (uint32_t)v; br = v >> 32; }
    neg1 = (r1[5] >> 31) != 0;
    neg2 = (r2[5] >> 31) != 0;
    uint64_t c = neg1 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { c += neg1 ? (uint32_t)~r1[i] : r1[i]; if (i < 5) k1[i] = (uint32_t)c; c >>= 32; }
    c = neg2 ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) { c += neg2 ? (uint32_t)~r2[i] : r2[i]; if (i < 5) k2[i] = (uint32_t)c; c >>= 32; }
}

// b of the magnitude m (5 words, below 2^(W ND)), left-aligned in RegularRecode<W>::NW words; even: m + 1 was recoded in m's place
template <int W>
ZK_HD void regular_recode(const uint32_t* m, uint32_t* b, bool& even) {
    typedef RegularRecode<W> RR;
    even = !(m[0] & 1);
    uint32_t v[6];   // (m | 1) >> 1, then the top bit 2^(W ND - 1)
#pragma unroll
    for (int i = 0; i < 5; ++i) v[i] = i < 4 ? (m[i] >> 1) | (m[i + 1] << 31) : m[i] >> 1;
    v[5] = 0;
    v[(W * RR::ND - 1) >> 5] |= 1u << ((W * RR::ND - 1) & 31);
#pragma unroll
    for (int i = RR::NW - 1; i >= 0; --i)
        b[i] = RR::PRE ? (v[i] << RR::PRE) | (i ? v[i - 1] >> (32 - RR::PRE) : 0u) : v[i];
}

// the next digit, most significant first: index (|d| - 1) / 2 and sign; b moves up by one window
template <int W>
ZK_HD void regular_next(uint32_t* b, uint32_t& index, bool& negative) {
    typedef RegularRecode<W> RR;
    const uint32_t win = b[RR::NW - 1] >> (32 - W);
    negative = !(win >> (W - 1));
    const uint32_t low = win & ((1u << (W - 1)) - 1);
    index = negative ? ((1u << (W - 1)) - 1) - low : low;
#pragma unroll
    for (int i = RR::NW - 1; i >= 0; --i) b[i] = (b[i] << W) | (i ? b[i - 1] >> (32 - W) : 0u);
}

}  // namespace zk
