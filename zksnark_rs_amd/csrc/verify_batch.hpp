// verify_batch.hpp -- what zk_verify_batch (verify_batch.hip), zk_verify_batch_all (verify_batch_all.hip) and the batch forms of
// the proof codec (proof_codec.hip) share: the call's stream and grow-only arena kept by the context, and the re-check of the
// CRS points through zk_verify's readers.
#pragma once
#include "common.hpp"
#include "pairing.cuh"
#include "vk.hpp"

namespace zk {

// the call's stream and device buffers, kept by the context; a buffer that has to grow is parked until the context goes,
// because hipFree would wait for every stream of the device (an outstanding proof included)
struct VerifyBatchState {
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> arena;
    std::vector<DevBuf<uint8_t>> retired;
    std::vector<std::shared_ptr<VkBinding>> keys;   // verifying keys bound to this context (vk.hpp): their buffers go with it
    ~VerifyBatchState() {
        for (auto& b : keys) {
            b->alive = false;
            b->consts.release();
            b->tables.release();
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// the context's state with its stream made
static inline VerifyBatchState& vb_state(zk_ctx* ctx) {
    if (!ctx->verify_batch) ctx->verify_batch = std::make_shared<VerifyBatchState>();
    VerifyBatchState& st = *ctx->verify_batch;
    if (!st.stream) ZK_HIP(hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking));
    return st;
}

// The verification constants: what the batch kernels read of a CRS or of a key.  The CRS forms fill them per call (host values,
// which the call uploads into its arena); the key forms take the device pointers from the key's binding.
struct VerifyConsts {
    size_t l = 0;
    const G1A* d_sg = nullptr;       // device: the l + 1 bases, Montgomery
    const Line* h_lines = nullptr;   // host: gamma's ATE_LINES lines, then delta's        } uploaded per call when
    const Fq12* h_c = nullptr;       // host: ml(alpha, beta)                              } d_lines is null
    const Line* d_lines = nullptr;   // device: the same, resident
    const Fq12* d_c = nullptr;
    const G1A* d_tab = nullptr;      // device: the input-sum tables of a key (vk_batch.hip), null = k_vb_inputs
    G1A alpha = G1A::infinity();     // host, zk_verify_batch_all: t_0 alpha
};

// the inputs zk_verify reads, before anything is launched: `text` is thrown with ZK_ERR_RANGE for an input >= r
static inline void vb_check_inputs(const uint64_t* inputs, size_t n_inputs, size_t k, size_t n_proofs, const char* text) {
    for (size_t j = 0; j < n_proofs; ++j)
        for (size_t i = 0; i < k; ++i) {
            Fr x;
            const uint64_t* w = inputs + (j * n_inputs + i) * 4;
            for (int h = 0; h < 4; ++h) { x.l[2 * h] = (uint32_t)w[h]; x.l[2 * h + 1] = (uint32_t)(w[h] >> 32); }
            ZK_REQUIRE(x.raw_in_range(), ZK_ERR_RANGE, text);
        }
}

// verify_batch.hip: the chunks of zk_verify_batch(_compressed) over the constants; inputs checked by the caller
void verify_batch_run(zk_ctx* ctx, const VerifyConsts& vc, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                      size_t n_proofs, int* ok, bool compressed);
// verify_batch.hip: S[j] for m rows of k packed inputs at d_x by k_vb_inputs
void vb_launch_inputs(const uint64_t* d_x, size_t k, const G1A* d_sg, size_t m, G1A* d_S, hipStream_t s);
// vk_batch.hip: the same from a key's tables by k_vk_inputs
void vk_launch_inputs(const uint64_t* d_x, size_t k, const G1A* d_sg, const G1A* d_tab, size_t m, G1A* d_S, hipStream_t s);
// verify_batch_all.hip: z and the inputs checked, t_0 = sum z_j (4 words); then the call over the constants.  fx: the lines of
// beta, gamma, delta and the finite flags; its t0_alpha is filled here
void vba_check(const uint64_t* z, const uint64_t* inputs, size_t n_inputs, size_t k, size_t n_proofs, uint64_t t0[4]);
void verify_batch_all_run(zk_ctx* ctx, const VerifyConsts& vc, VbaFixed& fx, const uint64_t t0[4], const uint64_t* inputs, size_t n_inputs,
                          const uint8_t* proofs, size_t n_proofs, const uint64_t* z, int* ok);

// proof_codec.hip: d_proofs[259 j ..) = the 259-byte form of d_in[128 j ..) for j < m, by the two decompress kernels on stream s.
// A block that is no valid encoding comes out as 0xFF bytes, which no decoder of the 259-byte form accepts.
void pc_launch_decompress(const uint8_t* d_in, size_t m, uint8_t* d_proofs, hipStream_t s);

static inline void words_of(const Fq& x, uint64_t* w) {
    const Fq c = x.to_canonical();
    for (int i = 0; i < 4; ++i) w[i] = (uint64_t)c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32);
}
// a device-resident (Montgomery) CRS point through zk_verify's reader: the same checks, the same point
static inline bool check_g1(const G1A& p, G1A& out) {
    uint64_t w[8];
    words_of(p.x, w); words_of(p.y, w + 4);
    return rd_g1(w, out);
}
static inline bool check_g2(const G2A& p, G2A& out) {
    uint64_t w[16];
    words_of(p.x.c0, w); words_of(p.x.c1, w + 4); words_of(p.y.c0, w + 8); words_of(p.y.c1, w + 12);
    return rd_g2(w, out);
}

}  // namespace zk
