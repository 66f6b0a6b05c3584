// proof_codec.hip -- the compressed 128-byte proof form: zk_proof_compress / zk_proof_decompress on the host, their batch forms
// on the GPU, and the launcher zk_verify_batch_compressed decompresses a chunk with (verify_batch.hip).  The arithmetic is
// point_codec.cuh, the same routines on both sides.
//
// Decompression is two launches, so that no wave mixes the one-exponentiation G1 chain with the three-exponentiation G2 chain
// (a mixed wave would run both one after the other):
//   k_pc_decompress_g1   one lane per G1 block, 2 per proof (A and C): 32 -> 65 bytes
//   k_pc_decompress_g2   one lane per G2 block: 64 -> 129 bytes
// Every lane runs the same fixed exponent chains whatever its flag or validity and selects at the end, so one malformed proof
// does not serialise its wave.  A block that is no valid encoding is written as 0xFF bytes; k_pc_finish then turns a proof with
// such a block into 259 x 0xFF and writes the verdict (zk_verify_batch_compressed skips it: k_vb_decode refuses tag 0xFF).
//   k_pc_compress        one lane per proof, no square roots: tag, range, curve and sign
// The batch calls run on the verify stream and the grow-only arena of verify_batch.hpp, ZK_VERIFY_BATCH_CHUNK proofs at a
// time, and synchronise only that stream.
#define ZK_MUL_OUTLINE 1
#include "pipeline.hpp"
#include "point_codec.cuh"
#include "verify_batch.hpp"

namespace zk {

static constexpr int PC_BLOCK = 64;
static_assert(ZK_PROOF_COMPRESSED_BYTES == 128 && ZK_PROOF_BYTES == 259, "block offsets below");

__global__ void __launch_bounds__(PC_BLOCK) k_pc_decompress_g1(const uint8_t* in, size_t n, uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= 2 * n) return;
    const size_t j = i >> 1;
    const bool c = i & 1;
    decompress_g1_block(in + j * ZK_PROOF_COMPRESSED_BYTES + (c ? 96 : 0), out + j * ZK_PROOF_BYTES + (c ? 194 : 0));
}
__global__ void __launch_bounds__(PC_BLOCK) k_pc_decompress_g2(const uint8_t* in, size_t n, uint8_t* out) {
    const size_t j = (size_t)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (j >= n) return;
    decompress_g2_block(in + j * ZK_PROOF_COMPRESSED_BYTES + 32, out + j * ZK_PROOF_BYTES + 65);
}
__global__ void __launch_bounds__(PC_BLOCK) k_pc_finish(uint8_t* out, size_t n, int* ok) {
    const size_t j = (size_t)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (j >= n) return;
    uint8_t* p = out + j * ZK_PROOF_BYTES;
    const bool good = p[0] != 0xff && p[65] != 0xff && p[194] != 0xff;
    if (!good) fill_bytes(p, ZK_PROOF_BYTES, 0xff);
    ok[j] = good ? 1 : 0;
}
__global__ void __launch_bounds__(PC_BLOCK) k_pc_compress(const uint8_t* in, size_t n, uint8_t* out, int* ok) {
    const size_t j = (size_t)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (j >= n) return;
    ok[j] = proof_compress(in + j * ZK_PROOF_BYTES, out + j * ZK_PROOF_COMPRESSED_BYTES) ? 1 : 0;
}

void pc_launch_decompress(const uint8_t* d_in, size_t m, uint8_t* d_proofs, hipStream_t s) {
    hipLaunchKernelGGL(k_pc_decompress_g1, dim3(ceil_div(2 * m, PC_BLOCK)), dim3(PC_BLOCK), 0, s, d_in, m, d_proofs);
    ZK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pc_decompress_g2, dim3(ceil_div(m, PC_BLOCK)), dim3(PC_BLOCK), 0, s, d_in, m, d_proofs);
    ZK_HIP(hipGetLastError());
}

// n entries of in_bytes each -> n entries of out_bytes each and n verdicts, a chunk at a time through the verify arena
static int codec_batch(zk_ctx* ctx, const uint8_t* in, size_t in_bytes, size_t n, uint8_t* out, size_t out_bytes, int* ok, bool compress) {
    if (!ctx) return ZK_ERR_ARG;
    if (n == 0) return ZK_OK;
    if (!in || !out || !ok) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        if (!ctx->verify_batch) ctx->verify_batch = std::make_shared<VerifyBatchState>();
        VerifyBatchState& st = *ctx->verify_batch;
        if (!st.stream) ZK_HIP(hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking));
        hipStream_t s = st.stream;
        const size_t m_max = std::min(n, (size_t)ZK_VERIFY_BATCH_CHUNK);
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_in = 0, o_out = o_in + up(m_max * in_bytes), o_ok = o_out + up(m_max * out_bytes), total = o_ok + up(m_max * sizeof(int));
        if (st.arena.n < total) {
            if (st.arena.p) st.retired.push_back(std::move(st.arena));
            st.arena.alloc(total);
        }
        uint8_t *d_in = st.arena.p + o_in, *d_out = st.arena.p + o_out;
        int* d_ok = (int*)(st.arena.p + o_ok);
        for (size_t j0 = 0; j0 < n; j0 += m_max) {
            const size_t m = std::min(m_max, n - j0);
            const unsigned grid = ceil_div(m, PC_BLOCK);
            ZK_HIP(hipMemcpyAsync(d_in, in + j0 * in_bytes, m * in_bytes, hipMemcpyHostToDevice, s));
            if (compress) {
                hipLaunchKernelGGL(k_pc_compress, dim3(grid), dim3(PC_BLOCK), 0, s, d_in, m, d_out, d_ok);
                ZK_HIP(hipGetLastError());
            } else {
                pc_launch_decompress(d_in, m, d_out, s);
                hipLaunchKernelGGL(k_pc_finish, dim3(grid), dim3(PC_BLOCK), 0, s, d_out, m, d_ok);
                ZK_HIP(hipGetLastError());
            }
            ZK_HIP(hipMemcpyAsync(out + j0 * out_bytes, d_out, m * out_bytes, hipMemcpyDeviceToHost, s));
            ZK_HIP(hipMemcpyAsync(ok + j0, d_ok, m * sizeof(int), hipMemcpyDeviceToHost, s));
            ZK_HIP(hipStreamSynchronize(s));   // the arena's chunk arrays are free for the next chunk
        }
    });
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_proof_compress(const uint8_t proof[ZK_PROOF_BYTES], uint8_t out[ZK_PROOF_COMPRESSED_BYTES]) {
    if (!proof || !out) return ZK_ERR_ARG;
    return proof_compress(proof, out) ? ZK_OK : ZK_ERR_RANGE;
}
int zk_proof_decompress(const uint8_t in[ZK_PROOF_COMPRESSED_BYTES], uint8_t proof_out[ZK_PROOF_BYTES]) {
    if (!in || !proof_out) return ZK_ERR_ARG;
    return proof_decompress(in, proof_out) ? ZK_OK : ZK_ERR_RANGE;
}
int zk_proof_compress_batch(zk_ctx* ctx, const uint8_t* proofs, size_t n, uint8_t* out, int* ok) {
    return codec_batch(ctx, proofs, ZK_PROOF_BYTES, n, out, ZK_PROOF_COMPRESSED_BYTES, ok, true);
}
int zk_proof_decompress_batch(zk_ctx* ctx, const uint8_t* in, size_t n, uint8_t* proofs_out, int* ok) {
    return codec_batch(ctx, in, ZK_PROOF_COMPRESSED_BYTES, n, proofs_out, ZK_PROOF_BYTES, ok, false);
}

}  // extern "C"
