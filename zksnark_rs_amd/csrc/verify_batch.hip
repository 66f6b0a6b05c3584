// verify_batch.hip -- zk_verify_batch: zk_verify for many proofs over one CRS, one lane per proof on the GPU.
//
// Per proof j (four kernels, per-proof state in HBM between them):
//   k_vb_decode   the 259 bytes through the decoder zk_verify uses (pairing.cuh dec_g1 / dec_g2, [r]B == infinity included)
//   k_vb_inputs   S_j = sum_gamma_0 + sum_{i=1..k} x_ji sum_gamma_i, k = min(l, n_inputs): one shared doubling per bit, a mixed
//                 addition per set bit (complete formulas, ec.cuh), then affine
//   k_vb_miller   f_j = ml(S_j, gamma) ml(C_j, delta) ml(-A_j, B_j) with one shared squaring per step, gamma's and delta's lines
//                 precomputed once per call (fixed argument), B's computed on the fly; times c = ml(alpha, beta), also once per call
//   k_vb_final    ok_j = decoded_j && final_exp_exact(f_j) == 1
// The host checks the inputs' range and the CRS points exactly as zk_verify does, computes c and the fixed lines, uploads bytes
// and inputs and reads the verdicts back.  Everything runs on the call's own stream.
// zk_verify_batch_compressed is the same call over 128-byte proofs: a chunk is decompressed on the device (proof_codec.hip) into
// the 259-byte strings k_vb_decode reads; a string that does not decompress arrives there as 0xFF bytes and is refused by tag.
#define ZK_MUL_OUTLINE 1
#include "pipeline.hpp"
#include "pairing.cuh"
#include "verify_batch.hpp"

namespace zk {

static constexpr int VB_BLOCK = 64;

__global__ void __launch_bounds__(VB_BLOCK) k_vb_decode(const uint8_t* proofs, size_t n, G1A* A, G2A* B, G1A* C, int* decoded) {
    const size_t j = (size_t)blockIdx.x * VB_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint8_t* p = proofs + j * ZK_PROOF_BYTES;
    G1A a = G1A::infinity(), c = G1A::infinity();
    G2A b = G2A::infinity();
    const bool ok = dec_g1(p, a) && dec_g2(p + 65, b) && dec_g1(p + 194, c);
    A[j] = a;
    B[j] = b;
    C[j] = c;
    decoded[j] = ok ? 1 : 0;
}

// x: n rows of k canonical inputs (4 words each), all < r (checked on the host); sg: the k + 1 bases, Montgomery
__global__ void __launch_bounds__(VB_BLOCK) k_vb_inputs(const uint64_t* x, size_t k, const G1A* sg, size_t n, G1A* S) {
    const size_t j = (size_t)blockIdx.x * VB_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint64_t* xj = x + j * k * 4;
    G1J acc = G1J::infinity();
    if (k) {
        for (int b = 253; b >= 0; --b) {   // inputs < r < 2^254
            acc = jac_dbl_ni(acc);
            for (size_t i = 0; i < k; ++i)
                if ((xj[4 * i + (b >> 6)] >> (b & 63)) & 1) acc = jac_madd_ni(acc, sg[i + 1]);
        }
    }
    S[j] = jac_to_affine(jac_madd_ni(acc, sg[0]));
}

// lines: gamma's ATE_LINES lines, then delta's; c: ml(alpha, beta)
__global__ void __launch_bounds__(VB_BLOCK) k_vb_miller(const G1A* S, const G1A* A, const G2A* B, const G1A* C, size_t n,
                                                        const Line* lines, const Fq12* c, Fq12* F) {
    const size_t j = (size_t)blockIdx.x * VB_BLOCK + threadIdx.x;
    if (j >= n) return;
    const G1A s = S[j], a = A[j].neg(), cc = C[j];
    const G2A q = B[j];
    const bool live_s = !s.is_inf(), live_c = !cc.is_inf(), live_ab = !a.is_inf() && !q.is_inf();
    const Line* lg = lines;
    const Line* ld = lines + ATE_LINES;
    const Fq2 b3 = twist_b3();
    G2Proj T{q.x, q.y, Fq2::one()};
    Fq12 f = Fq12::one();
    int m = 0;
    for (int i = ATE_LOOP_BITS - 2; i >= 0; --i) {
        f = fq12_sqr_ni(f);
        f = mul_line(f, lg[m], s, live_s);
        f = mul_line(f, ld[m], cc, live_c);
        f = mul_line(f, dbl_step(T, b3), a, live_ab);
        ++m;
        if (ate_bit(i)) {
            f = mul_line(f, lg[m], s, live_s);
            f = mul_line(f, ld[m], cc, live_c);
            f = mul_line(f, add_step(T, q), a, live_ab);
            ++m;
        }
    }
    G2A q1, q2;
    twist_frobenius_pair(q, q1, q2);
    f = mul_line(f, lg[m], s, live_s);
    f = mul_line(f, ld[m], cc, live_c);
    f = mul_line(f, add_step(T, q1), a, live_ab);
    ++m;
    f = mul_line(f, lg[m], s, live_s);
    f = mul_line(f, ld[m], cc, live_c);
    f = mul_line(f, add_step(T, q2), a, live_ab);
    F[j] = fq12_mul_ni(f, *c);
}

__global__ void __launch_bounds__(VB_BLOCK) k_vb_final(const Fq12* F, const int* decoded, size_t n, int* ok) {
    const size_t j = (size_t)blockIdx.x * VB_BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool one = final_exp_exact(F[j]) == Fq12::one();
    ok[j] = (decoded[j] && one) ? 1 : 0;
}

}  // namespace zk

using namespace zk;

void zk::vb_launch_inputs(const uint64_t* d_x, size_t k, const G1A* d_sg, size_t m, G1A* d_S, hipStream_t s) {
    hipLaunchKernelGGL(k_vb_inputs, dim3(ceil_div(m, VB_BLOCK)), dim3(VB_BLOCK), 0, s, d_x, k, d_sg, m, d_S);
    ZK_HIP(hipGetLastError());
}

// the chunks of zk_verify_batch and zk_verify_batch_compressed over the verification constants: `proofs` holds n_proofs strings of
// 259 bytes, or of 128 when `compressed`; a chunk of the latter is uploaded as it is and decompressed into d_proofs on the device.
void zk::verify_batch_run(zk_ctx* ctx, const VerifyConsts& vc, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                          size_t n_proofs, int* ok, bool compressed) {
    VerifyBatchState& st = vb_state(ctx);
    hipStream_t s = st.stream;
    const size_t k = std::min(vc.l, n_inputs);
    const bool resident = vc.d_lines != nullptr;

    // one arena: the constants unless they are resident, then the per-proof arrays of one chunk
    const size_t m_max = std::min(n_proofs, (size_t)ZK_VERIFY_BATCH_CHUNK);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_lines = 0, o_c = o_lines + (resident ? 0 : up(2 * ATE_LINES * sizeof(Line))), o_proofs = o_c + (resident ? 0 : up(sizeof(Fq12)));
    const size_t o_x = o_proofs + up(m_max * ZK_PROOF_BYTES), o_A = o_x + up(m_max * k * 32), o_B = o_A + up(m_max * sizeof(G1A));
    const size_t o_C = o_B + up(m_max * sizeof(G2A)), o_S = o_C + up(m_max * sizeof(G1A)), o_F = o_S + up(m_max * sizeof(G1A));
    const size_t o_dec = o_F + up(m_max * sizeof(Fq12)), o_ok = o_dec + up(m_max * sizeof(int));
    // the 128-byte strings of a chunk, behind everything zk_verify_batch itself lays out
    const size_t o_cin = o_ok + up(m_max * sizeof(int)), total = o_cin + (compressed ? up(m_max * ZK_PROOF_COMPRESSED_BYTES) : 0);
    if (st.arena.n < total) {
        if (st.arena.p) st.retired.push_back(std::move(st.arena));
        st.arena.alloc(total);
    }
    uint8_t* base = st.arena.p;
    const Line* d_lines = resident ? vc.d_lines : (const Line*)(base + o_lines);
    const Fq12* d_c = resident ? vc.d_c : (const Fq12*)(base + o_c);
    uint8_t* d_proofs = base + o_proofs;
    uint64_t* d_x = (uint64_t*)(base + o_x);
    G1A *d_A = (G1A*)(base + o_A), *d_C = (G1A*)(base + o_C), *d_S = (G1A*)(base + o_S);
    G2A* d_B = (G2A*)(base + o_B);
    Fq12* d_F = (Fq12*)(base + o_F);
    int *d_dec = (int*)(base + o_dec), *d_ok = (int*)(base + o_ok);
    if (!resident) {
        ZK_HIP(hipMemcpyAsync(base + o_lines, vc.h_lines, 2 * ATE_LINES * sizeof(Line), hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(base + o_c, vc.h_c, sizeof(Fq12), hipMemcpyHostToDevice, s));
    }

    std::vector<uint64_t> packed;
    for (size_t j0 = 0; j0 < n_proofs; j0 += m_max) {
        const size_t m = std::min(m_max, n_proofs - j0);
        const unsigned grid = ceil_div(m, VB_BLOCK);
        if (compressed) {
            uint8_t* d_cin = base + o_cin;
            ZK_HIP(hipMemcpyAsync(d_cin, proofs + j0 * ZK_PROOF_COMPRESSED_BYTES, m * ZK_PROOF_COMPRESSED_BYTES, hipMemcpyHostToDevice, s));
            pc_launch_decompress(d_cin, m, d_proofs, s);
        } else {
            ZK_HIP(hipMemcpyAsync(d_proofs, proofs + j0 * ZK_PROOF_BYTES, m * ZK_PROOF_BYTES, hipMemcpyHostToDevice, s));
        }
        if (k) {
            const uint64_t* src = inputs + j0 * n_inputs * 4;
            if (k != n_inputs) {   // only the first k inputs of a row are read (zip truncation)
                packed.resize(m * k * 4);
                for (size_t j = 0; j < m; ++j) std::memcpy(&packed[j * k * 4], src + j * n_inputs * 4, k * 32);
                src = packed.data();
            }
            ZK_HIP(hipMemcpyAsync(d_x, src, m * k * 32, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_vb_decode, dim3(grid), dim3(VB_BLOCK), 0, s, d_proofs, m, d_A, d_B, d_C, d_dec);
        ZK_HIP(hipGetLastError());
        if (vc.d_tab) vk_launch_inputs(d_x, k, vc.d_sg, vc.d_tab, m, d_S, s);
        else vb_launch_inputs(d_x, k, vc.d_sg, m, d_S, s);
        hipLaunchKernelGGL(k_vb_miller, dim3(grid), dim3(VB_BLOCK), 0, s, d_S, d_A, d_B, d_C, m, d_lines, d_c, d_F);
        ZK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_vb_final, dim3(grid), dim3(VB_BLOCK), 0, s, d_F, d_dec, m, d_ok);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(ok + j0, d_ok, m * sizeof(int), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));   // also keeps `packed` and the arena's chunk arrays free for the next chunk
    }
}

// the body of zk_verify_batch and zk_verify_batch_compressed: the constants of a CRS, made per call.  The error rules of the
// compressed call are zk_verify_batch's exactly, texts included: its zk_last_error also reads "verify_batch: ...", on purpose.
static int verify_batch_impl(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                             size_t n_proofs, int* ok, bool compressed) {
    if (!ctx || !crs) return ZK_ERR_ARG;
    if (n_proofs == 0) return ZK_OK;
    if (!proofs || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    std::fill(ok, ok + n_proofs, 0);
    return guarded(ctx, [&] {
        const size_t l = crs->input, k = std::min(l, n_inputs);
        vb_check_inputs(inputs, n_inputs, k, n_proofs, "verify_batch: input >= r");
        hipStream_t s = vb_state(ctx).stream;

        // the CRS points verify reads, copied on this stream (not through crs_download, which runs on the proving stream)
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
                   "verify_batch: CRS point not on the curve or outside G2");
        for (size_t i = 0; i <= k; ++i) {
            G1A g;
            ZK_REQUIRE(check_g1(h_sg[i], g), ZK_ERR_ARG, "verify_batch: CRS point not on the curve");
        }
        // once per call: c = ml(alpha, beta) and the lines of gamma and delta
        std::vector<Line> h_lines(2 * ATE_LINES);
        ml_lines(gamma, h_lines.data());
        ml_lines(delta, h_lines.data() + ATE_LINES);
        const Fq12 h_c = ml_proj(alpha, beta);
        VerifyConsts vc;
        vc.l = l;
        vc.d_sg = crs->sum_gamma1.p;
        vc.h_lines = h_lines.data();
        vc.h_c = &h_c;
        verify_batch_run(ctx, vc, inputs, n_inputs, proofs, n_proofs, ok, compressed);
    });
}

extern "C" int zk_verify_batch(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                               size_t n_proofs, int* ok) {
    return verify_batch_impl(ctx, crs, inputs, n_inputs, proofs, n_proofs, ok, false);
}
extern "C" int zk_verify_batch_compressed(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                                          size_t n_proofs, int* ok) {
    return verify_batch_impl(ctx, crs, inputs, n_inputs, proofs, n_proofs, ok, true);
}
