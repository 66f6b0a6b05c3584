// vk.hpp -- the verifying key (zk_vk): the five points and the l + 1 bases groth16::verify reads (groth16/mod.rs:299-320), with what
// depends only on them computed once.  The object is host data (vk.hip); a batch call binds it to ONE context (vk_batch.hip).
//
// Lifetime of the device side: a VkBinding is shared by the key and by the context's VerifyBatchState.  The buffers belong to the
// context -- whichever of zk_vk_free / zk_ctx_destroy comes first, the other finds the binding marked and touches no device memory:
//   zk_ctx_destroy first: ~VerifyBatchState frees the buffers and clears `alive`; the key stays usable on the host, a later batch
//                         call answers ZK_ERR_ARG.
//   zk_vk_free first:     the buffers move to the state's retired list (no hipFree under a live ticket) and go with the context.
//                         Nothing drains that list earlier: a context that binds and frees many keys holds their device memory
//                         (constants + tables, 15.4 MB at l = 257) until it is destroyed.
#pragma once
#include "common.hpp"
#include "verify_all.cuh"

namespace zk {

constexpr int VK_WINDOW_BITS = 4;                                   // unsigned digits of the input-sum tables
constexpr int VK_WINDOWS = 256 / VK_WINDOW_BITS;                    // inputs < r < 2^254: the top window holds 2 bits
constexpr int VK_ENTRIES = (1 << VK_WINDOW_BITS) - 1;               // d = 1 .. 2^w - 1 (digit 0 is skipped)
static inline size_t vk_table_bytes(size_t l) { return l * VK_WINDOWS * VK_ENTRIES * sizeof(G1A); }

struct VkBinding {
    zk_ctx* ctx = nullptr;      // compared only while `alive`
    bool alive = true;
    DevBuf<uint8_t> consts;     // gamma's and delta's lines | c = ml(alpha, beta) | the l + 1 bases (Montgomery)
    size_t o_c = 0, o_sg = 0;
    DevBuf<uint8_t> tables;     // T[i][s][d]: vk_batch.hip k_vk_table; empty until a call may use them
    bool tables_refused = false;   // their allocation failed once: k_vb_inputs serves this key (never an error, never a verdict's matter)
    void (*retire)(VkBinding&) = nullptr;   // vk_batch.hip: hands the buffers to the context's retired list
};

}  // namespace zk

struct zk_vk {
    size_t input = 0;
    std::vector<uint64_t> words;        // the payload of the byte form: alpha | beta | gamma | delta | sum_gamma[0..l], canonical
    zk::G1A alpha;
    zk::G2A beta, gamma, delta;         // through rd_g1 / rd_g2: Montgomery, on the curve, in G2
    std::vector<zk::G1A> sg;
    std::unique_ptr<zk::VbaFixed> fx;   // lines of beta, gamma, delta and which is finite (t0_alpha is per call)
    zk::Fq12 c;                         // ml_proj(alpha, beta)
    std::shared_ptr<zk::VkBinding> binding;
    const uint64_t* sg_words() const { return words.data() + 56; }
};

namespace zk {
constexpr size_t VK_HEAD_BYTES = 24;
static inline size_t vk_payload_words(size_t l) { return 56 + 8 * (l + 1); }
}  // namespace zk
