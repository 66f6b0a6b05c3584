// eddsa.hip -- EdDSA-Poseidon (eddsa.hpp) on the device: zk_eddsa_verify_batch, one signature per lane, a verdict per signature and no
// affine point, so nothing is inverted.  Two launches:
//   k_eddsa_challenge   the checks that need no curve arithmetic -- a word pattern >= r, A and R8 on the curve, S < l -- folded into a
//                       status word (the lowest code wins); hm = H6(R8.x, R8.y, A.x, A.y, M) by the permutation of width 6, the state of
//                       six elements in registers, M times the state one row at a time, the constants read at indices that are the
//                       same in every lane; hm goes to a context buffer (32 bytes a signature), and S | hm << 251 to d_bits_out.
//   k_eddsa_curve       [hm] A by the 2-bit register windows of k_babyjub_mul_var (127 windows: hm < 2^254), three doublings, + R8; then
//                       [S] Base8 by the 63 mixed additions of k_babyjub_mul_fixed over the context's table; then X1 Z2 = X2 Z1 and
//                       Y1 Z2 = Y2 Z1.  The status of the first launch overrides the comparison.
// The hash is a launch of its own because the curve kernel alone needs 240 VGPRs at two waves a SIMD (the variable-base loop holds P,
// 2 P, 3 P, the accumulator and the scalar) and the permutation of width 6 holds twelve elements through its mix (180 VGPRs on its own):
// fused, the kernel would pass 256 VGPRs and fall to one wave a SIMD (DESIGN 4r has the register figures).  Every lane runs the same
// instruction stream whatever its data: no lane returns early on a defect, a lane with a point off the curve walks the formulas on
// whatever values come out -- all of it register arithmetic, the table index is four bits of S -- and nothing depends on its Z being
// non-zero, since its status is already set.
#include <utility>
#include "babyjub_dev.cuh"
#include "eddsa.hpp"

namespace zk {

static constexpr unsigned EDDSA_T = 6, EDDSA_ROUNDS = POSEIDON_RF + POSEIDON_RP_T6;
static constexpr unsigned EDDSA_POINT_WORDS = 20, EDDSA_BITS_WORDS = 8;   // words of 64 bits an instance: the fields; a row of bits

struct EddsaState {
    DevBuf<Fr> par;            // C (EDDSA_ROUNDS x 6) then M (6 x 6, row-major), Montgomery form
    DevBuf<uint64_t> hm;       // count x 4 canonical words, grow-only
};

// s < l, by the borrow of s - l over limbs of 32 bits
__device__ __forceinline__ bool eddsa_below_l(const uint32_t (&s)[8]) {
    constexpr uint32_t L[8] = {0x392126f1u, 0x677297dcu, 0x3920ee0au, 0xab3eedb8u, 0xd0302b0bu, 0x370a08b6u, 0x5c263405u, 0x060c89ceu};
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)s[i] - L[i] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    return borrow != 0;
}

// The state is indexed through index sequences only, as in poseidon.hip: every index is a compile-time constant.
template <unsigned N>
using EddsaSeq = std::make_integer_sequence<unsigned, N>;
template <unsigned... J>
__device__ __forceinline__ Fr eddsa_row(const Fr (&s)[EDDSA_T], const Fr* __restrict__ row, std::integer_sequence<unsigned, J...>) {
    Fr acc = row[0] * s[0];
    ((acc = acc + row[J + 1] * s[J + 1]), ...);
    return acc;
}
__device__ __forceinline__ Fr eddsa_pow5(const Fr& x) {
    const Fr x2 = x.sqr();
    return x2.sqr() * x;
}
// one round: constants, S-boxes on all elements or on element 0, then M: the new state is built row by row beside the old one.  M is
// the same in every round, and left to itself the compiler keeps all 36 entries (288 registers) across the loop; the empty asm makes
// the pointer opaque once a round, so the entries are fetched again by scalar loads and 2 t elements are what stays live.
template <bool FULL, unsigned... I>
__device__ __forceinline__ void eddsa_round(Fr (&s)[EDDSA_T], const Fr* __restrict__ c, const Fr* m, std::integer_sequence<unsigned, I...>) {
    asm volatile("" : "+s"(m));
    ((s[I] = s[I] + c[I]), ...);
    if (FULL) ((s[I] = eddsa_pow5(s[I])), ...);
    else s[0] = eddsa_pow5(s[0]);
    Fr n[EDDSA_T];
    ((n[I] = eddsa_row(s, m + I * EDDSA_T, EddsaSeq<EDDSA_T - 1>())), ...);
    ((s[I] = n[I]), ...);
}

// grid: ceil(count / BABYJUB_BLOCK) blocks, lane j owns signature j.  bits: nullptr, or rows of bits_stride words of 64 bits.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_eddsa_challenge(const Fr* __restrict__ par, BjConsts k, const uint64_t* __restrict__ points, const uint64_t* __restrict__ sigs, size_t count,
                  uint64_t* __restrict__ hm_out, uint32_t* __restrict__ status, uint64_t* __restrict__ bits, size_t bits_stride) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t* __restrict__ in = points + EDDSA_POINT_WORDS * j;
    Fr s[EDDSA_T];
    const Fr sig = bj_load_raw(sigs + 4 * j);
    const Fr ax = bj_load_raw(in), ay = bj_load_raw(in + 4), rx = bj_load_raw(in + 8), ry = bj_load_raw(in + 12), msg = bj_load_raw(in + 16);
    const bool range = sig.raw_in_range() && ax.raw_in_range() && ay.raw_in_range() && rx.raw_in_range() && ry.raw_in_range() && msg.raw_in_range();
    s[0] = Fr::zero();
    s[1] = Fr::from_canonical(rx); s[2] = Fr::from_canonical(ry);
    s[3] = Fr::from_canonical(ax); s[4] = Fr::from_canonical(ay);
    s[5] = Fr::from_canonical(msg);
    uint32_t st = ZK_EDDSA_VALID;
    st = eddsa_below_l(sig.l) ? st : ZK_EDDSA_S_RANGE;
    st = bj_on_curve(k, s[1], s[2]) ? st : ZK_EDDSA_R_OFF_CURVE;
    st = bj_on_curve(k, s[3], s[4]) ? st : ZK_EDDSA_KEY_OFF_CURVE;
    st = range ? st : ZK_EDDSA_RANGE;
    status[j] = st;

    const Fr* __restrict__ c = par;
    const Fr* __restrict__ m = par + (size_t)EDDSA_ROUNDS * EDDSA_T;
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += EDDSA_T) eddsa_round<true>(s, c, m, EddsaSeq<EDDSA_T>());
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RP_T6; ++r, c += EDDSA_T) eddsa_round<false>(s, c, m, EddsaSeq<EDDSA_T>());
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += EDDSA_T) eddsa_round<true>(s, c, m, EddsaSeq<EDDSA_T>());
    const Fr d = s[0].to_canonical();
#pragma unroll
    for (int i = 0; i < 4; ++i) hm_out[4 * j + i] = (uint64_t)d.l[2 * i] | ((uint64_t)d.l[2 * i + 1] << 32);
    if (bits) {
        // 251 bits of S, then 254 bits of hm: 505 bits in 16 limbs, all zero for a word pattern >= r
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 7; ++i) w[i] = sig.l[i];
        w[7] = (sig.l[7] & 0x07ffffffu) | (d.l[0] << 27);
#pragma unroll
        for (int i = 0; i < 7; ++i) w[8 + i] = (d.l[i] >> 5) | (d.l[i + 1] << 27);
        w[15] = d.l[7] >> 5;
        uint64_t* __restrict__ row = bits + j * bits_stride;
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = range ? (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32) : 0;
    }
}

// grid as above.  status: what k_eddsa_challenge wrote; VALID becomes the verdict of the equation.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_eddsa_curve(const BjAffine* __restrict__ table, BjConsts k, const uint64_t* __restrict__ points, const uint64_t* __restrict__ sigs,
              const uint64_t* __restrict__ hm, size_t count, uint32_t* __restrict__ status) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t* __restrict__ in = points + EDDSA_POINT_WORDS * j;
    const Fr one = Fr::one(), zero = Fr::zero();
    uint32_t s[8];
    bj_load_words(hm + 4 * j, s);
#pragma unroll
    for (int i = 7; i > 0; --i) s[i] = (s[i] << 2) | (s[i - 1] >> 30);   // hm < 2^254: the walk starts at bit 253
    s[0] <<= 2;
    BjPoint right = BjPoint::identity();
    {
        const BjPoint p1{Fr::from_canonical(bj_load_raw(in)), Fr::from_canonical(bj_load_raw(in + 4)), one};
        const BjPoint p2 = bj_dbl(k, p1);
        const BjPoint p3 = bj_add_mixed(k, p2, p1.X, p1.Y);
#pragma unroll 1
        for (unsigned w = 0; w < 254 / BABYJUB_VAR_WINDOW; ++w) {
            const unsigned digit = s[7] >> 30;
#pragma unroll
            for (int i = 7; i > 0; --i) s[i] = (s[i] << 2) | (s[i - 1] >> 30);
            s[0] <<= 2;
            right = bj_dbl(k, bj_dbl(k, right));
            const BjPoint e{bj_pick(digit, zero, p1.X, p2.X, p3.X), bj_pick(digit, one, p1.Y, p2.Y, p3.Y), bj_pick(digit, one, one, p2.Z, p3.Z)};
            right = bj_add(k, right, e);
        }
    }
    right = bj_dbl(k, bj_dbl(k, bj_dbl(k, right)));                       // [8] ([hm] A): 8 hm is never a scalar
    right = bj_add_mixed(k, right, Fr::from_canonical(bj_load_raw(in + 8)), Fr::from_canonical(bj_load_raw(in + 12)));
    bj_load_words(sigs + 4 * j, s);
    BjPoint left = BjPoint::identity();
#pragma unroll 1
    for (unsigned w = 0; w < BABYJUB_FIXED_WINDOWS; ++w) {
        const BjAffine e = table[w * (1u << BABYJUB_FIXED_WINDOW) + (s[0] & 15)];
#pragma unroll
        for (int i = 0; i < 7; ++i) s[i] = (s[i] >> 4) | (s[i + 1] << 28);
        s[7] >>= 4;
        if (w == 0) { left.X = e.x; left.Y = e.y; }                       // the first window is the accumulator itself (w is uniform)
        else left = bj_add_mixed(k, left, e.x, e.y);
    }
    const bool equal = left.X * right.Z == right.X * left.Z && left.Y * right.Z == right.Y * left.Z;
    const uint32_t before = status[j];
    status[j] = before != ZK_EDDSA_VALID ? before : equal ? ZK_EDDSA_VALID : ZK_EDDSA_MISMATCH;
}

static EddsaState& eddsa_state(zk_ctx* ctx) {
    if (!ctx->eddsa) ctx->eddsa = std::make_shared<EddsaState>();
    EddsaState& st = *ctx->eddsa;
    if (!st.par.p) {
        const PoseidonParams& p = poseidon_params_t6();
        std::vector<Fr> host(p.c);
        host.insert(host.end(), p.m.begin(), p.m.end());
        DevBuf<Fr> buf(host.size());
        ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));   // `host` goes away
        st.par = std::move(buf);
    }
    return st;
}

static void eddsa_verify_batch(zk_ctx* ctx, const uint64_t* d_points, const uint64_t* d_s, size_t count, uint32_t* d_status, uint64_t* d_bits,
                               size_t bits_stride_words) {
    ZK_REQUIRE(count <= ((size_t)1 << 31) * BABYJUB_BLOCK, ZK_ERR_SIZE, "eddsa: too many signatures for one call");
    EddsaState& st = eddsa_state(ctx);
    const BjAffine* table = babyjub_table(ctx, babyjub_state(ctx));
    st.hm.ensure(4 * count);
    const dim3 grid(ceil_div(count, BABYJUB_BLOCK)), block(BABYJUB_BLOCK);
    const BjConsts k = babyjub_consts();
    {
        ProfScope ps(ctx, "eddsa_challenge", (double)count * (224.0 + (d_bits ? 64.0 : 0.0)));
        hipLaunchKernelGGL(k_eddsa_challenge, grid, block, 0, ctx->stream, st.par.p, k, d_points, d_s, count, st.hm.p, d_status, d_bits, bits_stride_words);
        ZK_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "eddsa_curve", (double)count * 232.0);
        hipLaunchKernelGGL(k_eddsa_curve, grid, block, 0, ctx->stream, table, k, d_points, d_s, st.hm.p, count, d_status);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_eddsa_verify_batch(zk_ctx* ctx, const void* d_points_msg, const void* d_s, size_t count, void* d_status, void* d_bits_out,
                          size_t bits_stride_bytes) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(!d_bits_out || (bits_stride_bytes >= 8 * EDDSA_BITS_WORDS && bits_stride_bytes % 8 == 0), ZK_ERR_ARG,
                   "eddsa: bits_stride_bytes must be a multiple of 8 and at least 64, got " + std::to_string(bits_stride_bytes));
        if (count == 0) return;
        ZK_REQUIRE(d_points_msg && d_s && d_status, ZK_ERR_ARG, "eddsa: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_points_msg | (uintptr_t)d_s | (uintptr_t)d_bits_out) % 8 == 0 && (uintptr_t)d_status % 4 == 0, ZK_ERR_ARG,
                   "eddsa: the device pointers must be 8-byte aligned (d_status: 4-byte)");
        eddsa_verify_batch(ctx, (const uint64_t*)d_points_msg, (const uint64_t*)d_s, count, (uint32_t*)d_status, (uint64_t*)d_bits_out,
                           bits_stride_bytes / 8);
    });
}

}  // extern "C"
