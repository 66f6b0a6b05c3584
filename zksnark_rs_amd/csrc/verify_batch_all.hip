// verify_batch_all.hip -- zk_verify_batch_all: one verdict for a whole batch of proofs over one CRS, by a random linear
// combination with the caller's secret multipliers z_j (verify_all.cuh states the equation).
//
// Per chunk of proofs (on the call's own stream, nothing synchronised until the end):
//   k_vba_lane     one lane per proof: decode, z_j A_j and z_j C_j, ml(-z_j A_j, B_j) with B's lines on the fly
//   k_vba_reduce   the lanes' (Miller value, C sum, decode flag) multiplied / added / ANDed: LDS within a block, then again over
//                  the blocks' results until one is left; k_vba_fold takes it into the call-wide accumulator
//   k_vba_columns  t_i over the chunk, i = 1..k (Fr), per tile of rows; k_vba_colsum adds the tiles into the call-wide t_i
// Once per call:
//   k_vba_ts       T_S = sum_{i=0..k} t_i sum_gamma_i, one lane per column, LDS tree, then k_vba_reduce
//   k_vba_finish   the fixed-argument pairs (t_0 alpha, beta), (T_S, gamma), (T_C, delta), the exact final exponentiation,
//                  compared with 1 and ANDed with the decode flags
// The host checks z, the inputs' range and the CRS points, computes t_0, t_0 alpha and the lines of beta, gamma and delta.
#define ZK_MUL_OUTLINE 1
#include "pipeline.hpp"
#include "verify_all.cuh"
#include "verify_batch.hpp"

namespace zk {

static constexpr int VBA_BLOCK = 64;
static constexpr int VBA_ROWS = 256;   // rows of a column-sum tile

// z: 2 words per proof; zm: z_j in Montgomery form for the column sums
__global__ void __launch_bounds__(VBA_BLOCK) k_vba_lane(const uint8_t* proofs, const uint64_t* z, size_t n, VbaAcc* out, Fr* zm) {
    const size_t j = (size_t)blockIdx.x * VBA_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t zw[4] = {(uint32_t)z[2 * j], (uint32_t)(z[2 * j] >> 32), (uint32_t)z[2 * j + 1], (uint32_t)(z[2 * j + 1] >> 32)};
    out[j] = vba_lane(proofs + j * ZK_PROOF_BYTES, zw);
    zm[j] = vba_z_mont(zw);
}

// the block's VBA_BLOCK values combined in LDS; thread 0 writes the result.  Every thread of the block calls it.
__device__ void vba_block_reduce(VbaAcc v, VbaAcc* out) {
    __shared__ VbaAcc lds[VBA_BLOCK];
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = VBA_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] = vba_combine(lds[threadIdx.x], lds[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = lds[0];
}

__global__ void __launch_bounds__(VBA_BLOCK) k_vba_reduce(const VbaAcc* in, size_t n, VbaAcc* out) {
    const size_t j = (size_t)blockIdx.x * VBA_BLOCK + threadIdx.x;
    vba_block_reduce(j < n ? in[j] : vba_identity(), out + blockIdx.x);
}

__global__ void __launch_bounds__(VBA_BLOCK) k_vba_fold(VbaAcc* acc, const VbaAcc* part) { *acc = vba_combine(*acc, *part); }

// part[b k + i] = sum of z_j x_ji over the rows j of tile b (grid: tiles x ceil(k / VBA_BLOCK)); x: m rows of k canonical inputs
__global__ void __launch_bounds__(VBA_BLOCK) k_vba_columns(const uint64_t* x, size_t k, const Fr* zm, size_t m, Fr* part) {
    const size_t i = (size_t)blockIdx.y * VBA_BLOCK + threadIdx.x;
    if (i >= k) return;
    const size_t j0 = (size_t)blockIdx.x * VBA_ROWS, j1 = j0 + VBA_ROWS < m ? j0 + VBA_ROWS : m;
    Fr acc = Fr::zero();
    for (size_t j = j0; j < j1; ++j) acc = acc + vba_zx(zm[j], x + (j * k + i) * 4);
    part[blockIdx.x * k + i] = acc;
}

// t[i] += sum over the nb tiles of part[b k + i]
__global__ void __launch_bounds__(VBA_BLOCK) k_vba_colsum(const Fr* part, size_t nb, size_t k, Fr* t) {
    const size_t i = (size_t)blockIdx.x * VBA_BLOCK + threadIdx.x;
    if (i >= k) return;
    Fr acc = t[i];
    for (size_t b = 0; b < nb; ++b) acc = acc + part[b * k + i];
    t[i] = acc;
}

// t: the k + 1 column sums (canonical), sg: the k + 1 bases; one block result per VBA_BLOCK columns
__global__ void __launch_bounds__(VBA_BLOCK) k_vba_ts(const Fr* t, size_t n, const G1A* sg, VbaAcc* out) {
    const size_t i = (size_t)blockIdx.x * VBA_BLOCK + threadIdx.x;
    VbaAcc v = vba_identity();
    if (i < n) v.c = vba_ts_term(t[i], sg[i]);
    vba_block_reduce(v, out + blockIdx.x);
}

__global__ void __launch_bounds__(VBA_BLOCK) k_vba_finish(const VbaAcc* acc, const VbaAcc* ts, const VbaFixed* fx, int* ok) {
    *ok = vba_finish(*acc, ts->c, *fx) ? 1 : 0;
}

}  // namespace zk

using namespace zk;

// every z_j != 0 and the inputs zk_verify reads < r, before anything is launched; t_0 = sum z_j < n 2^128 < r (no reduction)
void zk::vba_check(const uint64_t* z, const uint64_t* inputs, size_t n_inputs, size_t k, size_t n_proofs, uint64_t t0[4]) {
    t0[0] = t0[1] = t0[2] = t0[3] = 0;
    for (size_t j = 0; j < n_proofs; ++j) {
        ZK_REQUIRE(z[2 * j] | z[2 * j + 1], ZK_ERR_ARG, "verify_batch_all: a multiplier z_j is 0");
        unsigned __int128 s = (unsigned __int128)t0[0] + z[2 * j];
        t0[0] = (uint64_t)s;
        s = (unsigned __int128)t0[1] + z[2 * j + 1] + (uint64_t)(s >> 64);
        t0[1] = (uint64_t)s;
        t0[2] += (uint64_t)(s >> 64);
    }
    vb_check_inputs(inputs, n_inputs, k, n_proofs, "verify_batch_all: input >= r");
}

// zk_verify_batch_all over the verification constants (d_sg, alpha; fx: the lines of beta, gamma, delta)
void zk::verify_batch_all_run(zk_ctx* ctx, const VerifyConsts& vc, VbaFixed& fx, const uint64_t t0[4], const uint64_t* inputs, size_t n_inputs,
                              const uint8_t* proofs, size_t n_proofs, const uint64_t* z, int* ok) {
    VerifyBatchState& st = vb_state(ctx);
    hipStream_t s = st.stream;
    const size_t k = std::min(vc.l, n_inputs);
    // once per call: t_0 alpha, and t = (t_0, 0, ..., 0)
    uint32_t t0w[8];
    for (int h = 0; h < 4; ++h) { t0w[2 * h] = (uint32_t)t0[h]; t0w[2 * h + 1] = (uint32_t)(t0[h] >> 32); }
    fx.t0_alpha = jac_to_affine(g1_mul_bits(vc.alpha, t0w, 256));
    std::vector<Fr> h_t(k + 1, Fr::zero());
    for (int h = 0; h < 8; ++h) h_t[0].l[h] = t0w[h];
    const VbaAcc h_acc = vba_identity();

    // one arena: the call's constants and accumulators, then the arrays of one chunk
    const size_t m_max = std::min(n_proofs, (size_t)ZK_VERIFY_BATCH_CHUNK);
    const size_t n_part = ceil_div(m_max, VBA_BLOCK), n_tiles = ceil_div(m_max, VBA_ROWS), n_ts = ceil_div(k + 1, VBA_BLOCK);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_fx = 0, o_acc = o_fx + up(sizeof(VbaFixed)), o_t = o_acc + up(sizeof(VbaAcc)), o_ok = o_t + up((k + 1) * sizeof(Fr));
    const size_t o_proofs = o_ok + up(sizeof(int)), o_z = o_proofs + up(m_max * ZK_PROOF_BYTES), o_x = o_z + up(m_max * 16);
    const size_t o_lane = o_x + up(m_max * k * 32), o_part = o_lane + up(m_max * sizeof(VbaAcc)), o_zm = o_part + up(n_part * sizeof(VbaAcc));
    const size_t o_cols = o_zm + up(m_max * sizeof(Fr)), o_tsa = o_cols + up(n_tiles * k * sizeof(Fr)), o_tsb = o_tsa + up(n_ts * sizeof(VbaAcc));
    const size_t total = o_tsb + up(n_ts * sizeof(VbaAcc));
    if (st.arena.n < total) {
        if (st.arena.p) st.retired.push_back(std::move(st.arena));
        st.arena.alloc(total);
    }
    uint8_t* base = st.arena.p;
    VbaFixed* d_fx = (VbaFixed*)(base + o_fx);
    VbaAcc *d_acc = (VbaAcc*)(base + o_acc), *d_lane = (VbaAcc*)(base + o_lane), *d_part = (VbaAcc*)(base + o_part);
    VbaAcc *d_tsa = (VbaAcc*)(base + o_tsa), *d_tsb = (VbaAcc*)(base + o_tsb);
    Fr *d_t = (Fr*)(base + o_t), *d_zm = (Fr*)(base + o_zm), *d_cols = (Fr*)(base + o_cols);
    int* d_ok = (int*)(base + o_ok);
    uint8_t* d_proofs = base + o_proofs;
    uint64_t *d_z = (uint64_t*)(base + o_z), *d_x = (uint64_t*)(base + o_x);
    ZK_HIP(hipMemcpyAsync(d_fx, &fx, sizeof(VbaFixed), hipMemcpyHostToDevice, s));
    ZK_HIP(hipMemcpyAsync(d_acc, &h_acc, sizeof(VbaAcc), hipMemcpyHostToDevice, s));
    ZK_HIP(hipMemcpyAsync(d_t, h_t.data(), (k + 1) * sizeof(Fr), hipMemcpyHostToDevice, s));

    // n values at a, combined VBA_BLOCK at a time, ping-ponging with b, until one is left; returns where it is
    auto reduce = [&](VbaAcc* a, VbaAcc* b, size_t n) {
        while (n > 1) {
            const unsigned g = ceil_div(n, VBA_BLOCK);
            hipLaunchKernelGGL(k_vba_reduce, dim3(g), dim3(VBA_BLOCK), 0, s, a, n, b);
            ZK_HIP(hipGetLastError());
            std::swap(a, b);
            n = g;
        }
        return a;
    };
    for (size_t j0 = 0; j0 < n_proofs; j0 += m_max) {
        const size_t m = std::min(m_max, n_proofs - j0);
        ZK_HIP(hipMemcpyAsync(d_proofs, proofs + j0 * ZK_PROOF_BYTES, m * ZK_PROOF_BYTES, hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d_z, z + 2 * j0, m * 16, hipMemcpyHostToDevice, s));
        if (k)   // only the first k inputs of a row are read (zip truncation)
            ZK_HIP(hipMemcpy2DAsync(d_x, k * 32, inputs + j0 * n_inputs * 4, n_inputs * 32, k * 32, m, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_vba_lane, dim3(ceil_div(m, VBA_BLOCK)), dim3(VBA_BLOCK), 0, s, d_proofs, d_z, m, d_lane, d_zm);
        ZK_HIP(hipGetLastError());
        const VbaAcc* r = reduce(d_lane, d_part, m);
        hipLaunchKernelGGL(k_vba_fold, dim3(1), dim3(1), 0, s, d_acc, r);
        ZK_HIP(hipGetLastError());
        if (k) {
            hipLaunchKernelGGL(k_vba_columns, dim3(ceil_div(m, VBA_ROWS), ceil_div(k, VBA_BLOCK)), dim3(VBA_BLOCK), 0, s, d_x, k, d_zm, m, d_cols);
            ZK_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_vba_colsum, dim3(ceil_div(k, VBA_BLOCK)), dim3(VBA_BLOCK), 0, s, d_cols, (size_t)ceil_div(m, VBA_ROWS), k, d_t + 1);
            ZK_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_vba_ts, dim3(n_ts), dim3(VBA_BLOCK), 0, s, d_t, k + 1, vc.d_sg, d_tsa);
    ZK_HIP(hipGetLastError());
    const VbaAcc* ts = reduce(d_tsa, d_tsb, n_ts);
    hipLaunchKernelGGL(k_vba_finish, dim3(1), dim3(1), 0, s, d_acc, ts, d_fx, d_ok);
    ZK_HIP(hipGetLastError());
    int verdict = 0;
    ZK_HIP(hipMemcpyAsync(&verdict, d_ok, sizeof(int), hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    *ok = verdict;
}

extern "C" int zk_verify_batch_all(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                                   size_t n_proofs, const uint64_t* z, int* ok) {
    if (!ctx || !crs || !proofs || !z || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    *ok = 0;
    if (n_proofs == 0) {
        *ok = 1;
        return ZK_OK;
    }
    return guarded(ctx, [&] {
        const size_t l = crs->input, k = std::min(l, n_inputs);
        uint64_t t0[4];
        vba_check(z, inputs, n_inputs, k, n_proofs, t0);
        hipStream_t s = vb_state(ctx).stream;

        // the CRS points, copied on this stream and re-checked as zk_verify_batch does
        G1A h_alpha;
        G2A h_beta, h_gamma, h_delta;
        std::vector<G1A> h_sg(k + 1);
        ZK_HIP(hipMemcpyAsync(&h_alpha, crs->alpha1.p, sizeof(G1A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_beta, crs->beta2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_gamma, crs->gamma2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_delta, crs->delta2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(h_sg.data(), crs->sum_gamma1.p, (k + 1) * sizeof(G1A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
        G1A alpha;
        G2A beta, gamma, delta;
        ZK_REQUIRE(check_g1(h_alpha, alpha) && check_g2(h_beta, beta) && check_g2(h_gamma, gamma) && check_g2(h_delta, delta), ZK_ERR_ARG,
                   "verify_batch_all: CRS point not on the curve or outside G2");
        for (size_t i = 0; i <= k; ++i) {
            G1A g;
            ZK_REQUIRE(check_g1(h_sg[i], g), ZK_ERR_ARG, "verify_batch_all: CRS point not on the curve");
        }
        // once per call: the lines of beta, gamma and delta
        auto h_fx = std::make_unique<VbaFixed>();
        const G2A* qs[3] = {&beta, &gamma, &delta};
        for (int q = 0; q < 3; ++q) {
            ml_lines(*qs[q], h_fx->lines[q]);
            h_fx->finite[q] = qs[q]->is_inf() ? 0 : 1;
        }
        VerifyConsts vc;
        vc.l = l;
        vc.d_sg = crs->sum_gamma1.p;
        vc.alpha = alpha;
        verify_batch_all_run(ctx, vc, *h_fx, t0, inputs, n_inputs, proofs, n_proofs, z, ok);
    });
}
