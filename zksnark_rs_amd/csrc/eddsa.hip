// eddsa.hip -- EdDSA-Poseidon (eddsa.hpp) on the device: zk_eddsa_verify_batch and, below, zk_eddsa_sign_batch.  Verification: one
// signature per lane, a verdict per signature and no affine point, so nothing is inverted.  Two launches:
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
//
// zk_eddsa_sign_batch, one instance (k, n, M) per lane, three launches:
//   k_eddsa_sign_nonce      the range checks (0 < k < l, n < r, M < r), the lowest offender recorded by atomicMin, and
//                           rho = H6(n, M, 0, 0, 0) mod l into a context buffer.  The host reads the flag and refuses before any launch
//                           that writes an output.
//   k_eddsa_sign_points     A = [k] Base8 and R8 = [rho] Base8 by the walk of k_babyjub_mul_fixed, ONE Fermat inversion of Z_A Z_R for
//                           both, the row (A.x, A.y, R8.x, R8.y, M).
//   k_eddsa_sign_response   hm = H6 over the row by the permutation of k_eddsa_challenge, S = (rho + 8 (hm mod l) k) mod l by
//                           eddsa_modl.hpp, S and the bit row; zeros over rho.
// The first launch stands alone because the checks must be complete before an output is written.  The other two would fit one kernel
// (184 VGPRs, no scratch) and are split all the same: the response kernel runs at 166 VGPRs, three waves a SIMD, the fused form at two,
// and measured 1 % slower at 2^20 instances (DESIGN 4s has the figures).  rho lives in the context buffer between the launches only;
// k is read from the caller's array by each launch and kept nowhere.
#include <utility>
#include "babyjub_dev.cuh"
#include "eddsa.hpp"
#include "eddsa_modl.hpp"

namespace zk {

static constexpr unsigned EDDSA_T = 6, EDDSA_ROUNDS = POSEIDON_RF + POSEIDON_RP_T6;
static constexpr unsigned EDDSA_POINT_WORDS = 20, EDDSA_BITS_WORDS = 8;   // words of 64 bits an instance: the fields; a row of bits

struct EddsaState {
    DevBuf<Fr> par;            // C (EDDSA_ROUNDS x 6) then M (6 x 6, row-major), Montgomery form
    DevBuf<uint64_t> hm;       // count x 4 canonical words, grow-only
    DevBuf<uint64_t> rho;      // signing: count x 4 words, grow-only; secret between the launches of a call, zero afterwards
    DevBuf<unsigned long long> flag;   // signing: the lowest input out of range
};
static constexpr unsigned long long EDDSA_NO_ERROR = ~0ull;

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

// the permutation of width 6 over the state in registers; par: C (EDDSA_ROUNDS x 6) then M
__device__ __forceinline__ void eddsa_permute(Fr (&s)[EDDSA_T], const Fr* __restrict__ par) {
    const Fr* __restrict__ c = par;
    const Fr* __restrict__ m = par + (size_t)EDDSA_ROUNDS * EDDSA_T;
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += EDDSA_T) eddsa_round<true>(s, c, m, EddsaSeq<EDDSA_T>());
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RP_T6; ++r, c += EDDSA_T) eddsa_round<false>(s, c, m, EddsaSeq<EDDSA_T>());
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += EDDSA_T) eddsa_round<true>(s, c, m, EddsaSeq<EDDSA_T>());
}
// a row of d_bits_out: 251 bits of S, then 254 bits of hm: 505 bits in 16 limbs; all zero where `range` is false
__device__ __forceinline__ void eddsa_store_bits(uint64_t* __restrict__ row, const uint32_t (&sig)[8], const uint32_t (&hm)[8], bool range) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 7; ++i) w[i] = sig[i];
    w[7] = (sig[7] & 0x07ffffffu) | (hm[0] << 27);
#pragma unroll
    for (int i = 0; i < 7; ++i) w[8 + i] = (hm[i] >> 5) | (hm[i + 1] << 27);
    w[15] = hm[7] >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) row[i] = range ? (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32) : 0;
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

    eddsa_permute(s, par);
    const Fr d = s[0].to_canonical();
#pragma unroll
    for (int i = 0; i < 4; ++i) hm_out[4 * j + i] = (uint64_t)d.l[2 * i] | ((uint64_t)d.l[2 * i + 1] << 32);
    if (bits) eddsa_store_bits(bits + j * bits_stride, sig.l, d.l, range);   // all zero for a word pattern >= r
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
    const BjPoint left = bj_mul_fixed(table, k, s);
    const bool equal = left.X * right.Z == right.X * left.Z && left.Y * right.Z == right.Y * left.Z;
    const uint32_t before = status[j];
    status[j] = before != ZK_EDDSA_VALID ? before : equal ? ZK_EDDSA_VALID : ZK_EDDSA_MISMATCH;
}

// ---- zk_eddsa_sign_batch: lane j signs instance j ------------------------------------------------------------------------------
// flag: the lowest 4 j + input (0 the key, 1 the nonce key, 2 the message) out of range, by atomicMin; rho_out: H6(n, M, 0, 0, 0) mod l.
// Nothing else is written.  Reporting a refusal is the only branch on an input, and the caller is told of it anyway.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_eddsa_sign_nonce(const Fr* __restrict__ par, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ nonce_keys,
                   const uint64_t* __restrict__ msgs, size_t count, uint64_t* __restrict__ rho_out, unsigned long long* __restrict__ flag) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    uint32_t key[8];
    bj_load_words(keys + 4 * j, key);
    const Fr n = bj_load_raw(nonce_keys + 4 * j), msg = bj_load_raw(msgs + 4 * j);
    const bool key_ok = ((key[0] | key[1] | key[2] | key[3] | key[4] | key[5] | key[6] | key[7]) != 0) & eddsa_below_l(key);
    const unsigned bad = !key_ok ? 0u : !n.raw_in_range() ? 1u : !msg.raw_in_range() ? 2u : 3u;
    if (bad != 3u) atomicMin(flag, 4ull * j + bad);
    Fr s[EDDSA_T];
    s[0] = Fr::zero();
    s[1] = Fr::from_canonical(n); s[2] = Fr::from_canonical(msg);
    s[3] = Fr::zero(); s[4] = Fr::zero(); s[5] = Fr::zero();
    eddsa_permute(s, par);
    Fr d = s[0].to_canonical();
    modl_reduce_r(d.l);
#pragma unroll
    for (int i = 0; i < 4; ++i) rho_out[4 * j + i] = (uint64_t)d.l[2 * i] | ((uint64_t)d.l[2 * i + 1] << 32);
}

// A = [k] Base8 and R8 = [rho] Base8 by the walk of k_babyjub_mul_fixed, both to affine with one inversion, of Z_A Z_R; writes the
// row (A.x, A.y, R8.x, R8.y, M).  The stream is the same in every lane; the table entry is addressed by four bits of k, then of rho.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_eddsa_sign_points(const BjAffine* __restrict__ table, BjConsts k, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ rho,
                    const uint64_t* __restrict__ msgs, size_t count, uint64_t* __restrict__ points_out) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    uint32_t s[8];
    bj_load_words(keys + 4 * j, s);
    const BjPoint a = bj_mul_fixed(table, k, s);
    bj_load_words(rho + 4 * j, s);
    const BjPoint r8 = bj_mul_fixed(table, k, s);
    const Fr zi = bj_inv(a.Z * r8.Z), za = zi * r8.Z, zr = zi * a.Z;
    uint64_t* __restrict__ out = points_out + EDDSA_POINT_WORDS * j;
    bj_store(a.X * za, out);
    bj_store(a.Y * za, out + 4);
    bj_store(r8.X * zr, out + 8);
    bj_store(r8.Y * zr, out + 12);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[16 + i] = msgs[4 * j + i];
}

// hm = H6 over the row just written, S = (rho + 8 (hm mod l) k) mod l; writes S and the bit row, and zeros over rho.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_eddsa_sign_response(const Fr* __restrict__ par, const uint64_t* __restrict__ keys, uint64_t* __restrict__ rho, const uint64_t* __restrict__ points,
                      size_t count, uint64_t* __restrict__ s_out, uint64_t* __restrict__ bits, size_t bits_stride) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t* __restrict__ in = points + EDDSA_POINT_WORDS * j;
    Fr s[EDDSA_T];
    s[0] = Fr::zero();
    s[1] = Fr::from_canonical(bj_load_raw(in + 8)); s[2] = Fr::from_canonical(bj_load_raw(in + 12));
    s[3] = Fr::from_canonical(bj_load_raw(in)); s[4] = Fr::from_canonical(bj_load_raw(in + 4));
    s[5] = Fr::from_canonical(bj_load_raw(in + 16));
    eddsa_permute(s, par);
    const Fr d = s[0].to_canonical();
    uint32_t key[8], nonce[8], sig[8];
    bj_load_words(keys + 4 * j, key);
    bj_load_words(rho + 4 * j, nonce);
    modl_response(nonce, d.l, key, sig);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s_out[4 * j + i] = (uint64_t)sig[2 * i] | ((uint64_t)sig[2 * i + 1] << 32);
        rho[4 * j + i] = 0;
    }
    if (bits) eddsa_store_bits(bits + j * bits_stride, sig, d.l, true);
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

static void eddsa_sign_batch(zk_ctx* ctx, const uint64_t* d_keys, const uint64_t* d_nonce_keys, const uint64_t* d_msgs, size_t count,
                             uint64_t* d_points, uint64_t* d_s, uint64_t* d_bits, size_t bits_stride_words) {
    ZK_REQUIRE(count <= ((size_t)1 << 31) * BABYJUB_BLOCK, ZK_ERR_SIZE, "eddsa: too many signatures for one call");
    EddsaState& st = eddsa_state(ctx);
    const BjAffine* table = babyjub_table(ctx, babyjub_state(ctx));
    st.rho.ensure(4 * count);
    if (!st.flag.p) st.flag.alloc(1);
    const dim3 grid(ceil_div(count, BABYJUB_BLOCK)), block(BABYJUB_BLOCK);
    const BjConsts k = babyjub_consts();
    unsigned long long bad = EDDSA_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(st.flag.p, &EDDSA_NO_ERROR, sizeof(bad), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "eddsa_sign_nonce", (double)count * 128.0);
        hipLaunchKernelGGL(k_eddsa_sign_nonce, grid, block, 0, ctx->stream, st.par.p, d_keys, d_nonce_keys, d_msgs, count, st.rho.p, st.flag.p);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipMemcpyAsync(&bad, st.flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    if (bad != EDDSA_NO_ERROR) {
        ZK_HIP(hipMemsetAsync(st.rho.p, 0, 32 * count, ctx->stream));   // a refused call leaves no nonce behind
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        ctx->resolve_profile();
        const std::string at = " of instance " + std::to_string(bad / 4);
        ZK_REQUIRE(bad % 4 != 0, ZK_ERR_RANGE, "eddsa: the key" + at + " is 0 or not below l");
        ZK_REQUIRE(bad % 4 != 1, ZK_ERR_RANGE, "eddsa: the nonce key" + at + " is not below r");
        ZK_REQUIRE(false, ZK_ERR_RANGE, "eddsa: the message" + at + " is not below r");
    }
    {
        ProfScope ps(ctx, "eddsa_sign_points", (double)count * 256.0);
        hipLaunchKernelGGL(k_eddsa_sign_points, grid, block, 0, ctx->stream, table, k, d_keys, st.rho.p, d_msgs, count, d_points);
        ZK_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "eddsa_sign_response", (double)count * (288.0 + (d_bits ? 64.0 : 0.0)));
        hipLaunchKernelGGL(k_eddsa_sign_response, grid, block, 0, ctx->stream, st.par.p, d_keys, st.rho.p, d_points, count, d_s, d_bits, bits_stride_words);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_eddsa_sign_batch(zk_ctx* ctx, const void* d_keys, const void* d_nonce_keys, const void* d_msgs, size_t count, void* d_points_msg_out,
                        void* d_s_out, void* d_bits_out, size_t bits_stride_bytes) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(!d_bits_out || (bits_stride_bytes >= 8 * EDDSA_BITS_WORDS && bits_stride_bytes % 8 == 0), ZK_ERR_ARG,
                   "eddsa: bits_stride_bytes must be a multiple of 8 and at least 64, got " + std::to_string(bits_stride_bytes));
        if (count == 0) return;
        ZK_REQUIRE(d_keys && d_nonce_keys && d_msgs && d_points_msg_out && d_s_out, ZK_ERR_ARG, "eddsa: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_keys | (uintptr_t)d_nonce_keys | (uintptr_t)d_msgs | (uintptr_t)d_points_msg_out | (uintptr_t)d_s_out |
                    (uintptr_t)d_bits_out) % 8 == 0,
                   ZK_ERR_ARG, "eddsa: the device pointers must be 8-byte aligned");
        eddsa_sign_batch(ctx, (const uint64_t*)d_keys, (const uint64_t*)d_nonce_keys, (const uint64_t*)d_msgs, count, (uint64_t*)d_points_msg_out,
                         (uint64_t*)d_s_out, (uint64_t*)d_bits_out, bits_stride_bytes / 8);
    });
}

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
