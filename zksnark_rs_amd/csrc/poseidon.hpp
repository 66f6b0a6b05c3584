// poseidon.hpp -- Poseidon over the BN254 scalar field on the host: the parameters, generated in code, and the permutation over the
// host Fr.  S-box x^5, state width t = arity + 1 in {2, 3, 5}, R_F = 8 full rounds around R_P = 56 / 57 / 60 partial ones: circomlib's
// parameter sets.  hash(inputs): state = [0, inputs...]; per round add C[round * t + i] to element i, raise every element (full round)
// or element 0 (partial round) to the fifth power, multiply by M; the digest is element 0 after the last round.
//
// The constants come from the Poseidon paper's Grain LFSR.  80 bits of state, seeded most significant bit first with 01 | 0000 |
// n = 254 (12 bits) | t (12) | R_F (10) | R_P (10) | thirty 1s; one step shifts in b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0; 160 steps are
// discarded; the stream is self-shrinking (steps come in pairs, and a pair that starts with 1 yields its second bit); an element is
// 254 stream bits, most significant first.  The round constants are the first (R_F + R_P) t elements below r (others are rejected),
// then x_0..x_{t-1}, y_0..y_{t-1} are 2t more, each reduced mod r and all redrawn if two are equal or some x_i + y_j = 0, and
// M[i][j] = 1 / (x_i + y_j).  The paper's script also redraws M when a security test fails; for these three widths the first draw is
// the published one (tests/test_poseidon.py holds C, M and digests against the published values), which is why no other width is
// offered.  Width 6 (five inputs, R_P = 60) is the EdDSA challenge hash of eddsa.hpp and is INTERNAL: poseidon_params_t6() hands it to
// zk_eddsa_*, the gadget of zk_builder_eddsa_verify and eddsa.hip, while poseidon_rp(), which gates the public calls, still answers
// 0 for arity 5.  Its first draw gives hash(1, 2, 3, 4, 5) = 0x0dab9449...eeb123c0, the digest circomlibjs and go-iden3-crypto publish
// (tests/test_eddsa.py), so the first draw is the published one for this width too.
// Header-only and free of device code: tests/cpp/poseidon_host.hip compiles it alone under the sanitizers.
#pragma once
#include <memory>
#include <mutex>
#include <vector>
#include "witgen_tape.hpp"

namespace zk {

constexpr unsigned POSEIDON_RF = 8;
constexpr unsigned POSEIDON_MAX_T = 6;
constexpr unsigned POSEIDON_RP_T6 = 60;
// 0: the arity is not offered
static inline unsigned poseidon_rp(size_t arity) { return arity == 1 ? 56 : arity == 2 ? 57 : arity == 4 ? 60 : 0; }

struct PoseidonParams {
    unsigned t = 0, rf = POSEIDON_RF, rp = 0;
    std::vector<Fr> c;   // (rf + rp) * t round constants, Montgomery form
    std::vector<Fr> m;   // t * t, row-major: m[i * t + j] = M[i][j], Montgomery form
    unsigned rounds() const { return rf + rp; }
};

struct PoseidonGrain {
    bool b[80];
    unsigned at = 0;   // b[(at + k) % 80] is bit k of the register
    PoseidonGrain(unsigned t, unsigned rf, unsigned rp) {
        unsigned n = 0;
        auto put = [&](unsigned value, unsigned width) {
            for (unsigned i = 0; i < width; ++i) b[n++] = (value >> (width - 1 - i)) & 1;
        };
        put(1, 2); put(0, 4); put(254, 12); put(t, 12); put(rf, 10); put(rp, 10);
        for (unsigned i = 0; i < 30; ++i) b[n++] = true;
        for (unsigned i = 0; i < 160; ++i) step();
    }
    bool bit(unsigned k) const { return b[(at + k) % 80]; }
    bool step() {
        const bool fresh = bit(62) ^ bit(51) ^ bit(38) ^ bit(23) ^ bit(13) ^ bit(0);
        b[at] = fresh;             // the oldest bit leaves, the new one is bit 79
        at = (at + 1) % 80;
        return fresh;
    }
    bool next_bit() {
        for (;;) {
            const bool first = step(), second = step();
            if (first) return second;
        }
    }
    // 254 bits, most significant first, as raw (canonical) limbs; may be >= r
    Fr next_element() {
        Fr x = Fr::zero();
        for (int k = 253; k >= 0; --k)
            if (next_bit()) x.l[k >> 5] |= 1u << (k & 31);
        return x;
    }
};

static inline PoseidonParams poseidon_generate(size_t arity, unsigned rp) {
    PoseidonParams p;
    p.t = (unsigned)arity + 1;
    p.rp = rp;
    const unsigned t = p.t;
    PoseidonGrain g(t, p.rf, p.rp);
    while (p.c.size() < (size_t)p.rounds() * t) {
        const Fr x = g.next_element();
        if (x.raw_in_range()) p.c.push_back(Fr::from_canonical(x));
    }
    std::vector<Fr> xy(2 * t);
    for (;;) {
        for (Fr& e : xy) e = Fr::from_canonical(Fr::reduce_once(g.next_element(), 0));   // an element is < 2^254 < 2 r
        bool good = true;
        for (unsigned i = 0; i < 2 * t; ++i)
            for (unsigned j = i + 1; j < 2 * t; ++j) good = good && xy[i] != xy[j];
        for (unsigned i = 0; i < t; ++i)
            for (unsigned j = 0; j < t; ++j) good = good && !(xy[i] + xy[t + j]).is_zero();
        if (good) break;
    }
    p.m.resize((size_t)t * t);
    for (unsigned i = 0; i < t; ++i)
        for (unsigned j = 0; j < t; ++j) p.m[i * t + j] = (xy[i] + xy[t + j]).inv();
    return p;
}

// the parameters of one arity, made on first use; nullptr for an arity that is not offered
inline const PoseidonParams* poseidon_params(size_t arity) {
    static std::mutex mu;
    static std::unique_ptr<PoseidonParams> made[POSEIDON_MAX_T];
    if (!poseidon_rp(arity)) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!made[arity]) made[arity].reset(new PoseidonParams(poseidon_generate(arity, poseidon_rp(arity))));
    return made[arity].get();
}

// width 6, for eddsa.hpp and the EdDSA gadget only
inline const PoseidonParams& poseidon_params_t6() {
    static const PoseidonParams made = poseidon_generate(5, POSEIDON_RP_T6);
    return made;
}

static inline Fr poseidon_pow5(const Fr& x) {
    const Fr x2 = x * x;
    return x2 * x2 * x;
}

// state: t elements in Montgomery form
static inline void poseidon_permute(const PoseidonParams& p, Fr* state) {
    const unsigned t = p.t;
    Fr next[POSEIDON_MAX_T];
    for (unsigned rnd = 0; rnd < p.rounds(); ++rnd) {
        for (unsigned i = 0; i < t; ++i) state[i] = state[i] + p.c[(size_t)rnd * t + i];
        const bool full = rnd < p.rf / 2 || rnd >= p.rf / 2 + p.rp;
        for (unsigned i = 0; i < (full ? t : 1u); ++i) state[i] = poseidon_pow5(state[i]);
        for (unsigned i = 0; i < t; ++i) {
            Fr acc = Fr::zero();
            for (unsigned j = 0; j < t; ++j) acc = acc + p.m[i * t + j] * state[j];
            next[i] = acc;
        }
        for (unsigned i = 0; i < t; ++i) state[i] = next[i];
    }
}

// inputs in Montgomery form -> the digest in Montgomery form
static inline Fr poseidon_hash_mont(const PoseidonParams& p, const Fr* inputs) {
    Fr state[POSEIDON_MAX_T];
    state[0] = Fr::zero();
    for (unsigned i = 1; i < p.t; ++i) state[i] = inputs[i - 1];
    poseidon_permute(p, state);
    return state[0];
}

// z_0 = 0, z_{k + 1} = hash(z_k, z_k): the value of a subtree of height k without a leaf (Montgomery form, depth + 1 entries)
static inline std::vector<Fr> poseidon_zero_hashes(unsigned depth) {
    const PoseidonParams& p = *poseidon_params(2);
    std::vector<Fr> z(depth + 1, Fr::zero());
    for (unsigned k = 0; k < depth; ++k) {
        const Fr pair[2] = {z[k], z[k]};
        z[k + 1] = poseidon_hash_mont(p, pair);
    }
    return z;
}

// ---- the two context-free entry points of include/zkgpu.h ---------------------------------------
static inline int poseidon_hash_words(const uint64_t* inputs, size_t arity, uint64_t out[4]) {
    const PoseidonParams* p = poseidon_params(arity);
    if (!p || !inputs || !out) return ZK_ERR_ARG;
    Fr in[POSEIDON_MAX_T - 1];
    for (size_t i = 0; i < arity; ++i) {
        const Fr x = fr_from_words(inputs + 4 * i);
        if (!x.raw_in_range()) return ZK_ERR_RANGE;
        in[i] = Fr::from_canonical(x);
    }
    fr_to_words(poseidon_hash_mont(*p, in).to_canonical(), out);
    return ZK_OK;
}
static inline int poseidon_params_words(size_t arity, unsigned* rf, unsigned* rp, uint64_t* round_constants, uint64_t* mds) {
    const PoseidonParams* p = poseidon_params(arity);
    if (!p) return ZK_ERR_ARG;
    if (rf) *rf = p->rf;
    if (rp) *rp = p->rp;
    if (round_constants)
        for (size_t i = 0; i < p->c.size(); ++i) fr_to_words(p->c[i].to_canonical(), round_constants + 4 * i);
    if (mds)
        for (size_t i = 0; i < p->m.size(); ++i) fr_to_words(p->m[i].to_canonical(), mds + 4 * i);
    return ZK_OK;
}

}  // namespace zk
