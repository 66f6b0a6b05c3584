// verify_host.hpp -- the part of groth16::verify (groth16/mod.rs:299-320) that zk_verify (verify.hip, points from a CRS) and
// zk_vk_verify (vk.hip, points from a verifying key) share: the proof through the decoder, the inputs' range, and
// S = sum_{i <= min(l, n_inputs)} (1, inputs...)_i sum_gamma_i.  Host code; nothing here needs a device.
#pragma once
#include "common.hpp"
#include "pairing.cuh"

namespace zk {

// sg_words: the l + 1 bases as canonical words (8 each), read through rd_g1 as they are met.  Returns false for a malformed or
// off-curve proof (rejected before anything else is looked at); throws ZK_ERR_ARG for a base off the curve, ZK_ERR_RANGE for an
// input >= r.
static inline bool verify_decode_sum(const uint64_t* sg_words, size_t l, const uint64_t* inputs, size_t n_inputs, const uint8_t* proof,
                                     G1A& A, G2A& B, G1A& C, G1A& S) {
    if (!dec_g1(proof, A) || !dec_g2(proof + 65, B) || !dec_g1(proof + 194, C)) return false;   // malformed / off-curve proof: rejected
    // sum_term = sum_{i<=l} (1, inputs...)_i * sum_gamma_i  (zip truncates, mod.rs:308-314)
    G1J sum = G1J::infinity();
    for (size_t i = 0; i <= l && i < n_inputs + 1; ++i) {
        G1A g;
        ZK_REQUIRE(rd_g1(sg_words + 8 * i, g), ZK_ERR_ARG, "verify: CRS point not on the curve");
        Fr k;
        if (i == 0) { k = Fr::zero(); k.l[0] = 1; }
        else {
            k = Fr::zero();
            for (int w = 0; w < 4; ++w) { k.l[2 * w] = (uint32_t)inputs[4 * (i - 1) + w]; k.l[2 * w + 1] = (uint32_t)(inputs[4 * (i - 1) + w] >> 32); }
            ZK_REQUIRE(k.raw_in_range(), ZK_ERR_RANGE, "verify: input >= r");
        }
        sum = jac_add(sum, jac_mul_words(G1J::from_affine(g), k.l));
    }
    S = jac_to_affine(sum);
    return true;
}

}  // namespace zk
