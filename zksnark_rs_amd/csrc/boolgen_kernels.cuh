// boolgen_kernels.cuh -- the bit-sliced kernels that boolgen.hip (boolean circuits) and mixgen.hip (the boolean core of any built
// circuit) both launch; the layout of the state and what each step does is described at the top of boolgen.hip.  The kernels are
// static: each of the two files gets its own code object of them.
#pragma once
#include "pipeline.hpp"
#include "circuit.hpp"

namespace zk {

static constexpr unsigned BG_EVAL_THREADS = 1024;
static constexpr unsigned BG_LOAD_WAVES = 4;
static constexpr unsigned BG_EXPAND_THREADS = 256;
static constexpr size_t BG_MAX_CHUNK_WORDS = 32768;   // a grid dimension of the expansion

// G rule: the largest of 8, 4, 2 words per workgroup that still leaves one workgroup per compute unit, else 1.  More words per
// workgroup read the tape fewer times and make a slot's access G * 8 contiguous bytes; fewer keep every compute unit busy.
static unsigned boolgen_group_words(size_t words, int cu_count) {
    for (unsigned g = 8; g > 1; g /= 2)
        if (words / g >= (size_t)cu_count) return g;
    return 1;
}

// grid: one workgroup per instance word of the chunk; word0 = first word of the chunk (global numbering)
static __global__ void __launch_bounds__(64 * BG_LOAD_WAVES)
k_bool_load(const uint8_t* __restrict__ in, size_t stride, size_t count, size_t word0, const uint32_t* __restrict__ in_wit, unsigned n_in, unsigned m,
            size_t nw, uint64_t* __restrict__ state) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t w = blockIdx.x;
    const size_t j = (word0 + w) * 64 + lane;
    const bool live = j < count;
    if (threadIdx.x == 0) {
        state[w] = ~0ull;                     // index 0: the constant 1
        state[(size_t)m * nw + w] = 0;        // index m: the constant 0
    }
    const unsigned n_bytes = (n_in + 7) / 8;
    for (unsigned k = wave; k < n_bytes; k += BG_LOAD_WAVES) {        // wave-uniform trip count: every lane takes part in every ballot
        const unsigned byte = live ? in[j * stride + k] : 0u;
        const unsigned bits = min(8u, n_in - 8 * k);
        for (unsigned b = 0; b < bits; ++b) {
            const unsigned long long word = __ballot((byte >> b) & 1u);
            if (lane == 0) state[(size_t)in_wit[8 * k + b] * nw + w] = word;
        }
    }
}

// grid: one workgroup per G = 1 << g_log words of the chunk
static __global__ void __launch_bounds__(BG_EVAL_THREADS)
k_bool_eval(const BoolOp* __restrict__ ops, const uint32_t* __restrict__ level_ptr, unsigned levels, unsigned g_log, size_t nw, uint64_t* state) {
    const size_t w_base = (size_t)blockIdx.x << g_log;
    const unsigned g_mask = (1u << g_log) - 1;
    for (unsigned l = 0; l < levels; ++l) {
        const unsigned begin = level_ptr[l], end = level_ptr[l + 1];
        const size_t pairs = (size_t)(end - begin) << g_log;
        for (size_t idx = threadIdx.x; idx < pairs; idx += BG_EVAL_THREADS) {
            const size_t w = w_base + (idx & g_mask);
            if (w < nw) {
                const uint4 raw = reinterpret_cast<const uint4*>(ops)[begin + (idx >> g_log)];   // {dst, a, b, kind}
                const uint64_t a = state[(size_t)raw.y * nw + w], b = state[(size_t)raw.z * nw + w];
                state[(size_t)raw.x * nw + w] = bool_apply(raw.w, a, b);
            }
        }
        __syncthreads();
    }
}

// grid: (ceil(m / threads), words of the chunk)
static __global__ void __launch_bounds__(BG_EXPAND_THREADS)
k_bool_expand(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, unsigned m, uint64_t* __restrict__ out) {
    const unsigned s = blockIdx.x * BG_EXPAND_THREADS + threadIdx.x;
    const size_t w = blockIdx.y;
    const bool mine = s < m;
    const uint64_t word = mine ? state[(size_t)s * nw + w] : 0;
    const size_t j0 = (word0 + w) * 64;
    const unsigned n = (unsigned)min((size_t)64, count - j0);          // j0 < count for every word of a chunk
    if (!mine) return;                                                  // (no barrier and no cross-lane operation follows)
    uint4* o = reinterpret_cast<uint4*>(out + (j0 * m + s) * 4);
    for (unsigned l = 0; l < n; ++l) {
        o[0] = make_uint4((unsigned)((word >> l) & 1), 0, 0, 0);
        o[1] = make_uint4(0, 0, 0, 0);
        o += (size_t)m * 2;
    }
}

// The same bytes with a lane PAIR per wire: the even lane stores {bit, 0}, the odd lane the two zero words, so one wave instruction
// covers 1 KiB contiguous.  grid: (ceil(2 m / threads), words of the chunk)
static __global__ void __launch_bounds__(BG_EXPAND_THREADS)
k_bool_expand_pair(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, unsigned m, uint64_t* __restrict__ out) {
    const unsigned t = blockIdx.x * BG_EXPAND_THREADS + threadIdx.x;
    const unsigned s = t >> 1;
    const size_t w = blockIdx.y;
    if (s >= m) return;                                                 // (no barrier and no cross-lane operation follows)
    const uint64_t word = (t & 1) ? 0 : state[(size_t)s * nw + w];      // the odd lane writes zeros whatever the bit
    const size_t j0 = (word0 + w) * 64;
    const unsigned n = (unsigned)min((size_t)64, count - j0);
    uint4* o = reinterpret_cast<uint4*>(out + j0 * m * 4) + t;
    for (unsigned l = 0; l < n; ++l) {
        *o = make_uint4((unsigned)((word >> l) & 1), 0, 0, 0);
        o += (size_t)m * 2;
    }
}

// The 4 canonical words of a packed wire for instance `lane` of word w: bit i of the value is operand i's bit.  The operand index and
// its state word do not depend on the lane (scalar loads); the four limbs are four named values, no indexed array.
__device__ __forceinline__ uint64_t pack_limb(const uint64_t* __restrict__ state, size_t nw, size_t w, const uint32_t* __restrict__ bits,
                                              unsigned lo, unsigned hi, unsigned lane) {
    uint64_t v = 0;
    for (unsigned e = lo; e < hi; ++e) v |= ((state[(size_t)bits[e] * nw + w] >> lane) & 1) << (e - lo);
    return v;
}
__device__ __forceinline__ void pack_gather(const uint64_t* __restrict__ state, size_t nw, size_t w, const uint32_t* __restrict__ bits,
                                            unsigned begin, unsigned end, unsigned lane, uint4& lo, uint4& hi) {
    const uint64_t l0 = pack_limb(state, nw, w, bits, begin, min(end, begin + 64), lane);
    const uint64_t l1 = pack_limb(state, nw, w, bits, min(end, begin + 64), min(end, begin + 128), lane);
    const uint64_t l2 = pack_limb(state, nw, w, bits, min(end, begin + 128), min(end, begin + 192), lane);
    const uint64_t l3 = pack_limb(state, nw, w, bits, min(end, begin + 192), end, lane);
    lo = make_uint4((unsigned)l0, (unsigned)(l0 >> 32), (unsigned)l1, (unsigned)(l1 >> 32));
    hi = make_uint4((unsigned)l2, (unsigned)(l2 >> 32), (unsigned)l3, (unsigned)(l3 >> 32));
}

// grid: (packs, words of the chunk); one wave, lane = instance.  Lanes behind `count` write nothing; there is no cross-lane operation.
static __global__ void __launch_bounds__(64)
k_bool_expand_packs(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, unsigned m, const uint32_t* __restrict__ pack_out,
                    const uint32_t* __restrict__ pack_ptr, const uint32_t* __restrict__ pack_bits, uint64_t* __restrict__ out) {
    const unsigned p = blockIdx.x, lane = threadIdx.x;
    const size_t w = blockIdx.y;
    uint4 lo, hi;
    pack_gather(state, nw, w, pack_bits, pack_ptr[p], pack_ptr[p + 1], lane, lo, hi);
    const size_t j = (word0 + w) * 64 + lane;
    if (j >= count) return;
    uint4* o = reinterpret_cast<uint4*>(out + (j * m + pack_out[p]) * 4);
    o[0] = lo;
    o[1] = hi;
}

}  // namespace zk
