// babyjub_dev.cuh -- what babyjub.hip and eddsa.hip share on the device: the per-context state with the window table of Base8, the
// loads and stores of canonical words, the fixed-base walk over the table, the Fermat inversion and the selection among four register
// entries.
#pragma once
#include "common.hpp"
#include "babyjub.hpp"

namespace zk {

static constexpr unsigned BABYJUB_BLOCK = 256;
static constexpr unsigned BABYJUB_FIXED_WINDOW = ZK_BABYJUB_FIXED_WINDOW, BABYJUB_FIXED_WINDOWS = 256 / BABYJUB_FIXED_WINDOW;
static constexpr unsigned BABYJUB_VAR_WINDOW = ZK_BABYJUB_VAR_WINDOW;
static_assert(BABYJUB_FIXED_WINDOW == 4 && BABYJUB_VAR_WINDOW == 2, "the kernels' shifts and selections are written for these windows");

struct BabyjubState {
    DevBuf<BjAffine> table;               // [window][digit]: j 16^k Base8, affine, Montgomery form
    DevBuf<unsigned long long> flag;      // [0] range, [1] curve
};
// babyjub.hip: the context's state, made on first use, and its table, built on the host and uploaded on first use
BabyjubState& babyjub_state(zk_ctx* ctx);
const BjAffine* babyjub_table(zk_ctx* ctx, BabyjubState& st);

// 4 words of 64 bits behind an 8-byte aligned pointer -> 8 limbs
__device__ __forceinline__ void bj_load_words(const uint64_t* __restrict__ w, uint32_t (&l)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t v = w[i];
        l[2 * i] = (uint32_t)v;
        l[2 * i + 1] = (uint32_t)(v >> 32);
    }
}
__device__ __forceinline__ Fr bj_load_raw(const uint64_t* __restrict__ w) {
    Fr x;
    bj_load_words(w, x.l);
    return x;
}
__device__ __forceinline__ void bj_store(const Fr& v, uint64_t* __restrict__ w) {
    const Fr c = v.to_canonical();
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint64_t)c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32);
}
// x^(r - 2): the exponent is the same in every lane and is shifted through scalar registers, so the branch is uniform
__device__ __forceinline__ Fr bj_inv(const Fr& x) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = FrParams::P[i];
    e[0] -= 2;
    Fr acc = Fr::one();
#pragma unroll 1
    for (int i = 0; i < 256; ++i) {
        acc = acc.sqr();
        if (e[7] >> 31) acc = acc * x;
#pragma unroll
        for (int w = 7; w > 0; --w) e[w] = (e[w] << 1) | (e[w - 1] >> 31);
        e[0] <<= 1;
    }
    return acc;
}
// [s] Base8 over the context's table, from the least significant window of 4 bits: 63 mixed additions, no doubling.  s is consumed.
__device__ __forceinline__ BjPoint bj_mul_fixed(const BjAffine* __restrict__ table, const BjConsts& k, uint32_t (&s)[8]) {
    BjPoint acc = BjPoint::identity();
#pragma unroll 1
    for (unsigned w = 0; w < BABYJUB_FIXED_WINDOWS; ++w) {
        const BjAffine e = table[w * (1u << BABYJUB_FIXED_WINDOW) + (s[0] & 15)];
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] = (s[i] >> 4) | (s[i + 1] << 28);
        s[7] >>= 4;
        if (w == 0) { acc.X = e.x; acc.Y = e.y; }          // the first window is the accumulator itself (w is uniform)
        else acc = bj_add_mixed(k, acc, e.x, e.y);
    }
    return acc;
}
__device__ __forceinline__ Fr bj_pick(unsigned digit, const Fr& e0, const Fr& e1, const Fr& e2, const Fr& e3) {
    Fr o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t lo = digit & 1 ? e1.l[i] : e0.l[i], hi = digit & 1 ? e3.l[i] : e2.l[i];
        o.l[i] = digit & 2 ? hi : lo;
    }
    return o;
}

}  // namespace zk
