// babyjub.hip -- Baby Jubjub (babyjub.hpp) on the device: zk_babyjub_mul_batch, one scalar multiplication per lane, the point in
// projective coordinates in registers, one Fermat inversion per lane back to affine.
//   k_babyjub_mul_fixed   [s] Base8.  A per-context table holds j 16^k Base8 for the 64 windows k of 4 bits and j < 16, affine, Montgomery
//                         form (64 KiB, built on the host at first use).  A lane walks its scalar from the least significant window, reads
//                         the entry of its digit (a per-lane index into the window's 16 entries, 64 bytes) and adds it with the mixed
//                         addition: 63 additions of 12 multiplications, no doubling.  Digit 0 reads the identity like any other entry.
//   k_babyjub_mul_var     [s] P.  The lane keeps P, 2 P, 3 P in registers and walks its scalar from the most significant window of 2 bits:
//                         two doublings, then the addition of the entry its digit selects among (0 : 1 : 1), P, 2 P, 3 P -- by v_cndmask on
//                         every limb, not by an address.  128 (2 x 8 + 13) + 20 = 3732 multiplications.  No LDS: a table of 16 projective
//                         entries a lane is 96 KiB a wave and leaves one wave a CU.
//   k_babyjub_check       variable base only, before anything is written: flag[0] = the lowest instance with a coordinate >= r, flag[1] =
//                         the lowest instance off the curve (atomicMin, the arrangement of k_poseidon_update_check).
// Every lane executes the same instruction stream whatever its scalar and point: the loops have fixed trip counts, the scalar is shifted
// through registers with constant indices, digits select by index or by v_cndmask, and the addition law is complete, so no value is a
// special case.  The inversion walks the public exponent r - 2 held in scalar registers.
#include "babyjub_dev.cuh"

namespace zk {

static constexpr unsigned long long BABYJUB_NO_ERROR = ~0ull;

__device__ __forceinline__ void bj_store_affine(const BjPoint& p, uint64_t* __restrict__ out) {
    const Fr zi = bj_inv(p.Z);
    bj_store(p.X * zi, out);
    bj_store(p.Y * zi, out + 4);
}

// grid: ceil(count / BABYJUB_BLOCK) blocks, lane j owns instance j.  out_stride: words of 64 bits between two results, >= 8.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_babyjub_mul_fixed(const BjAffine* __restrict__ table, BjConsts k, const uint64_t* __restrict__ scalars, size_t count, uint64_t* __restrict__ out,
                    size_t out_stride) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    uint32_t s[8];
    bj_load_words(scalars + 4 * j, s);
    const BjPoint acc = bj_mul_fixed(table, k, s);
    bj_store_affine(acc, out + j * out_stride);
}

// grid as above.  points: count x 8 canonical words, checked by k_babyjub_check before this launch.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_babyjub_mul_var(BjConsts k, const uint64_t* __restrict__ scalars, const uint64_t* __restrict__ points, size_t count, uint64_t* __restrict__ out,
                  size_t out_stride) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    uint32_t s[8];
    bj_load_words(scalars + 4 * j, s);
    const Fr one = Fr::one(), zero = Fr::zero();
    const BjPoint p1{Fr::from_canonical(bj_load_raw(points + 8 * j)), Fr::from_canonical(bj_load_raw(points + 8 * j + 4)), one};
    const BjPoint p2 = bj_dbl(k, p1);
    const BjPoint p3 = bj_add_mixed(k, p2, p1.X, p1.Y);
    BjPoint acc = BjPoint::identity();
#pragma unroll 1
    for (unsigned w = 0; w < 256 / BABYJUB_VAR_WINDOW; ++w) {
        const unsigned digit = s[7] >> 30;
#pragma unroll
        for (int i = 7; i > 0; --i) s[i] = (s[i] << 2) | (s[i - 1] >> 30);
        s[0] <<= 2;
        acc = bj_dbl(k, bj_dbl(k, acc));
        const BjPoint e{bj_pick(digit, zero, p1.X, p2.X, p3.X), bj_pick(digit, one, p1.Y, p2.Y, p3.Y), bj_pick(digit, one, one, p2.Z, p3.Z)};
        acc = bj_add(k, acc, e);
    }
    bj_store_affine(acc, out + j * out_stride);
}

// grid as above.  Writes the flags only.
__global__ void __launch_bounds__(BABYJUB_BLOCK)
k_babyjub_check(BjConsts k, const uint64_t* __restrict__ points, size_t count, unsigned long long* __restrict__ flags) {
    const size_t j = (size_t)blockIdx.x * BABYJUB_BLOCK + threadIdx.x;
    if (j >= count) return;
    const Fr x = bj_load_raw(points + 8 * j), y = bj_load_raw(points + 8 * j + 4);
    if (!x.raw_in_range() || !y.raw_in_range()) atomicMin(flags, (unsigned long long)j);
    else if (!bj_on_curve(k, Fr::from_canonical(x), Fr::from_canonical(y))) atomicMin(flags + 1, (unsigned long long)j);
}

BabyjubState& babyjub_state(zk_ctx* ctx) {
    if (!ctx->babyjub) ctx->babyjub = std::make_shared<BabyjubState>();
    BabyjubState& st = *ctx->babyjub;
    if (!st.flag.p) st.flag.alloc(2);
    return st;
}
const BjAffine* babyjub_table(zk_ctx* ctx, BabyjubState& st) {
    if (!st.table.p) {
        const std::vector<BjAffine> host = babyjub_window_table(BABYJUB_FIXED_WINDOW, BABYJUB_FIXED_WINDOWS);
        DevBuf<BjAffine> buf(host.size());
        ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(BjAffine), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));   // `host` goes away
        st.table = std::move(buf);
    }
    return st.table.p;
}

static void babyjub_mul_batch(zk_ctx* ctx, const uint64_t* d_scalars, const uint64_t* d_points, size_t count, uint64_t* d_out, size_t stride) {
    BabyjubState& st = babyjub_state(ctx);
    ZK_REQUIRE(count <= ((size_t)1 << 31) * BABYJUB_BLOCK, ZK_ERR_SIZE, "babyjub: too many points for one call");
    const dim3 grid(ceil_div(count, BABYJUB_BLOCK)), block(BABYJUB_BLOCK);
    const BjConsts k = babyjub_consts();
    if (!d_points) {
        const BjAffine* table = babyjub_table(ctx, st);
        ProfScope ps(ctx, "babyjub_mul_fixed", (double)count * 96.0);
        hipLaunchKernelGGL(k_babyjub_mul_fixed, grid, block, 0, ctx->stream, table, k, d_scalars, count, d_out, stride);
        ZK_HIP(hipGetLastError());
    } else {
        static const unsigned long long none[2] = {BABYJUB_NO_ERROR, BABYJUB_NO_ERROR};
        unsigned long long bad[2] = {BABYJUB_NO_ERROR, BABYJUB_NO_ERROR};
        ZK_HIP(hipMemcpyAsync(st.flag.p, none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_babyjub_check, grid, block, 0, ctx->stream, k, d_points, count, st.flag.p);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(bad, st.flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        ZK_REQUIRE(bad[0] == BABYJUB_NO_ERROR, ZK_ERR_RANGE, "babyjub: coordinate >= r in instance " + std::to_string(bad[0]));
        ZK_REQUIRE(bad[1] == BABYJUB_NO_ERROR, ZK_ERR_RANGE, "babyjub: point not on the curve in instance " + std::to_string(bad[1]));
        ProfScope ps(ctx, "babyjub_mul_var", (double)count * 160.0);
        hipLaunchKernelGGL(k_babyjub_mul_var, grid, block, 0, ctx->stream, k, d_scalars, d_points, count, d_out, stride);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_babyjub_mul_batch(zk_ctx* ctx, const void* d_scalars, const void* d_points, size_t count, void* d_out, size_t out_stride_words) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(out_stride_words == 0 || out_stride_words >= 8, ZK_ERR_ARG,
                   "babyjub: out_stride_words must be 0 or at least 8, got " + std::to_string(out_stride_words));
        if (count == 0) return;
        ZK_REQUIRE(d_scalars && d_out, ZK_ERR_ARG, "babyjub: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_scalars | (uintptr_t)d_points | (uintptr_t)d_out) % 8 == 0, ZK_ERR_ARG,
                   "babyjub: the device pointers must be 8-byte aligned");
        babyjub_mul_batch(ctx, (const uint64_t*)d_scalars, (const uint64_t*)d_points, count, (uint64_t*)d_out, out_stride_words ? out_stride_words : 8);
    });
}

}  // extern "C"
