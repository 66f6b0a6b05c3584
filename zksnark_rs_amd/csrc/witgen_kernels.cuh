// witgen_kernels.cuh -- what the two kernels that run a zk::Tape with one instance per lane share: k_witgen (witgen.hip: the whole
// circuit) and k_mix_tail (mixgen.hip: the field tail behind a bit-sliced core).  The group of 64 instances, the W rule and the run of
// operations are the same; what differs is where an operand comes from, so the run takes the operand fetch as a parameter.
#pragma once
#include "pipeline.hpp"
#include "witgen_tape.hpp"

namespace zk {

static constexpr int WG_LANES = 64;
static constexpr unsigned WG_MAX_WAVES = 4;
static constexpr unsigned long long WG_NO_ERROR = ~0ull;

// The W rule: W = the mean number of operations per level, rounded up to a power of two, at most 4 (and at most the widest level).
// A level of `width` operations costs ceil(width / W) rounds and every level one barrier; waves beyond the mean width would wait at
// barriers most of the time, and parallelism beyond one group comes from the other groups.  A chain (every level 1 wide) gets W = 1.
static unsigned witgen_waves(const Tape& t) {
    const size_t levels = t.levels();
    if (!levels) return 1;
    const size_t mean = (t.ops.size() + levels - 1) / levels;
    unsigned w = 1;
    while (w < mean && w < WG_MAX_WAVES) w *= 2;
    while (w > 1 && w / 2 >= t.max_level_width()) w /= 2;
    return w;
}

// Operations begin, begin + stride, ... < end in this order, each reading what the ones before it in the run (and before the run)
// wrote.  The operands of the next operation are requested BEFORE the current one is computed, so that their memory latency passes
// under a field multiplication instead of in front of it; where the next operation reads the current result (every step of a chain)
// the value is handed over in registers and the early load is dropped.  Without this a dependent chain pays store -> load through
// the cache per operation: 2.8 us per operation measured on the 2^16-gate chain, one wave per group.
// `fetch(x)` is the value of operand word x; `fetch.is_slot(x)` says whether x names a slot of `sc` (a destination always does).
template <class Fetch>
__device__ __forceinline__ void witgen_run_ops(const TapeOp* __restrict__ ops, uint32_t begin, uint32_t end, uint32_t stride, Fr* sc, const Fetch& fetch) {
    if (begin >= end) return;
    TapeOp cur = ops[begin];
    Fr a = fetch(cur.a), b = fetch(cur.b);
    for (uint32_t k = begin; k < end; k += stride) {
        const bool more = k + stride < end;
        TapeOp nxt = cur;
        Fr na = a, nb = b;
        if (more) {
            nxt = ops[k + stride];
            na = fetch(nxt.a);
            nb = fetch(nxt.b);
        }
        const Fr r = cur.kind == TAPE_COPY ? a : cur.kind == TAPE_MUL ? a * b : a + b;
        sc[(size_t)cur.dst * WG_LANES] = r;
        if (fetch.is_slot(nxt.a) && nxt.a == cur.dst) na = r;
        if (fetch.is_slot(nxt.b) && nxt.b == cur.dst) nb = r;
        cur = nxt;
        a = na;
        b = nb;
    }
}

}  // namespace zk
