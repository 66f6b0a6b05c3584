// verify_batch.hpp -- what zk_verify_batch (verify_batch.hip), zk_verify_batch_all (verify_batch_all.hip) and the batch forms of
// the proof codec (proof_codec.hip) share: the call's stream and grow-only arena kept by the context, and the re-check of the
// CRS points through zk_verify's readers.
#pragma once
#include "common.hpp"
#include "pairing.cuh"

namespace zk {

// the call's stream and device buffers, kept by the context; a buffer that has to grow is parked until the context goes,
// because hipFree would wait for every stream of the device (an outstanding proof included)
struct VerifyBatchState {
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> arena;
    std::vector<DevBuf<uint8_t>> retired;
    ~VerifyBatchState() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

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
