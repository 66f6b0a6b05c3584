// mixgen.hip -- zk_mixgen_*: the witnesses of ANY built circuit (builder.hpp) for many input sets at once: its boolean core bit-sliced,
// as boolgen.hip runs a boolean circuit, and its field tail as a small field tape with one instance per lane, as witgen.hip runs a
// whole circuit.  zk_builder_finish splits every circuit (circuit.hpp: Mixed): a wire is bit-class if it is a constant, a bit input or
// a boolean gate over bit-class wires, and field-class otherwise; nothing bit-class reads anything field-class.
//   state      boolgen.hip's: uint64 per (witness index, instance word).  Field-class indices own a slot nothing writes.
//   scratch    witgen.hip's, over the TAIL's slots only: value of tail slot s for lane l of word w at ((w * slots + s) * 64 + l)
//   per chunk of words, on the context's stream:
//     k_bool_load, k_bool_eval (the core tape), k_bool_expand[_pair], k_bool_expand_packs (the core packs)   boolgen_kernels.cuh
//     k_mix_tail   one workgroup per word, lane = instance, W waves by witgen_waves' rule on the tail tape: field inputs range-checked
//                  (a word pattern >= r: atomicMin of the instance into a flag), to Montgomery form, to their slots; the tail level by
//                  level through witgen_run_ops (witgen_kernels.cuh) with an operand fetch that knows four forms -- a pooled
//                  constant, a tail slot, a bit-class index ((state word >> lane) & 1 selects Montgomery one or zero: the word is
//                  the same for the whole wave, nothing is multiplied) and a core pack (pack_gather, then to Montgomery form; the
//                  split copies a pack into a temporary at its first reader, so each is gathered once); then every tail slot that is
//                  a witness index to canonical form into out[(j * m + index) * 4].  That overwrites what the expansion wrote there
//                  from the index's never-written state slot -- the arrangement of k_bool_expand_packs: no byte left depends on it.
//   zk_mixgen_eval_fields runs load, core and the tail into scratch only (no expansion, no store), then k_mix_fields gathers the
//                  named wires from state, packs and tail slots.
// Lanes behind `count` take part in every barrier of k_mix_tail and are predicated off every load and store.  The cap
// "boolgen_scratch_kib" covers state plus scratch: a word of 64 instances needs (m + 1) * 8 + tail slots * 64 * 32 bytes.
#include "boolgen_kernels.cuh"
#include "witgen_kernels.cuh"

struct zk_mixgen {
    zk_ctx* ctx = nullptr;
    size_t n_bit = 0, n_field = 0, m = 0, levels = 0;   // levels of the core tape
    size_t slots = 0, n_store = 0, tail_levels = 0;     // tail slots; those that are witness indices (the first n_store)
    unsigned waves = 1;
    size_t scratch_cap = 0;                 // bytes
    unsigned group_words = 0;               // 0 = by rule
    bool expand_pair = false;
    zk::DevBuf<zk::BoolOp> ops;
    zk::DevBuf<uint32_t> level_ptr, bit_in_wit, sel;
    size_t n_packs = 0;                     // core packs
    zk::DevBuf<uint32_t> pack_out, pack_ptr, pack_bits;
    zk::DevBuf<zk::TapeOp> tail_ops;
    zk::DevBuf<uint32_t> tail_level_ptr, slot_wit;
    zk::DevBuf<zk::Fr> consts, scratch;
    zk::DevBuf<uint64_t> state;
    zk::DevBuf<unsigned long long> flag;
    std::vector<uint32_t> ref;              // per witness index: the operand word (circuit.hpp: MIX_*) that names its value
};

namespace zk {

// an operand of the tail tape (circuit.hpp: MIX_*).  The operand word is the same for every lane of a wave, so is the branch taken.
struct MixFetch {
    const Fr* __restrict__ consts;
    const Fr* sc;                           // this lane's scratch: slot s at sc[s * 64]
    const uint64_t* __restrict__ state;
    size_t nw, w;
    const uint32_t* __restrict__ pack_ptr;
    const uint32_t* __restrict__ pack_bits;
    unsigned lane;
    __device__ __forceinline__ bool is_slot(uint32_t x) const { return !(x & MIX_TAG); }
    __device__ __forceinline__ Fr operator()(uint32_t x) const {
        const uint32_t i = x & MIX_INDEX, tag = x & MIX_TAG;
        if (tag == MIX_SLOT) return sc[(size_t)i * WG_LANES];
        if (tag == TAPE_CONST) return consts[i];
        if (tag == MIX_BIT) {
            const bool bit = (state[(size_t)i * nw + w] >> lane) & 1;
            const Fr one = Fr::one();
            Fr r;
#pragma unroll
            for (int k = 0; k < 8; ++k) r.l[k] = bit ? one.l[k] : 0u;
            return r;
        }
        uint4 lo, hi;
        pack_gather(state, nw, w, pack_bits, pack_ptr[i], pack_ptr[i + 1], lane, lo, hi);
        Fr v;
        v.l[0] = lo.x; v.l[1] = lo.y; v.l[2] = lo.z; v.l[3] = lo.w;
        v.l[4] = hi.x; v.l[5] = hi.y; v.l[6] = hi.z; v.l[7] = hi.w;
        return Fr::from_canonical(v);
    }
};

// grid: one workgroup of W waves per instance word of the chunk.  out == nullptr: the tail into scratch only (zk_mixgen_eval_fields).
__global__ void __launch_bounds__(WG_LANES * WG_MAX_WAVES)
k_mix_tail(const TapeOp* __restrict__ ops, const uint32_t* __restrict__ level_ptr, unsigned levels, const Fr* __restrict__ consts,
           const uint32_t* __restrict__ slot_wit, unsigned n_store, const uint64_t* __restrict__ in_fields, unsigned n_field, unsigned m, size_t slots,
           const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, const uint32_t* __restrict__ pack_ptr,
           const uint32_t* __restrict__ pack_bits, Fr* __restrict__ scratch, uint64_t* __restrict__ out, unsigned long long* __restrict__ flag) {
    const unsigned lane = threadIdx.x & (WG_LANES - 1), wave = threadIdx.x / WG_LANES, W = blockDim.x / WG_LANES;
    const size_t w = blockIdx.x;
    const size_t j = (word0 + w) * WG_LANES + lane;                     // instance
    const bool live = j < count;
    Fr* sc = scratch + w * slots * WG_LANES + lane;                     // slot s of this lane: sc[s * 64]

    if (live) {
        const uint64_t* in = in_fields + j * (size_t)n_field * 4;
        for (unsigned i = wave; i < n_field; i += W) {                  // field input i owns tail slot i
            Fr x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t v = in[4 * (size_t)i + k];
                x.l[2 * k] = (uint32_t)v;
                x.l[2 * k + 1] = (uint32_t)(v >> 32);
            }
            if (!x.raw_in_range()) atomicMin(flag, (unsigned long long)j);
            sc[(size_t)i * WG_LANES] = Fr::from_canonical(x);
        }
    }
    if (W > 1) __syncthreads();

    const MixFetch fetch{consts, sc, state, nw, w, pack_ptr, pack_bits, lane};
    if (W == 1) {                       // one wave, program order: the whole tail as one run, no barrier
        if (live) witgen_run_ops(ops, 0, level_ptr[levels], 1, sc, fetch);
    } else {
        for (unsigned l = 0; l < levels; ++l) {
            if (live) witgen_run_ops(ops, level_ptr[l] + wave, level_ptr[l + 1], W, sc, fetch);
            __syncthreads();
        }
    }

    if (live && out) {
        uint64_t* o = out + j * (size_t)m * 4;
        for (unsigned s = wave; s < n_store; s += W) {
            const Fr x = sc[(size_t)s * WG_LANES].to_canonical();
            uint4* dst = reinterpret_cast<uint4*>(o + 4 * (size_t)slot_wit[s]);
            dst[0] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
            dst[1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
        }
    }
}

// grid: (named wires, words of the chunk); one wave, lane = instance: out[(j * n_sel + i) * 4 ..] = the wire that operand word sel[i]
// names, as 4 canonical words.  No barrier and no cross-lane operation: lanes behind `count` leave at once.
__global__ void __launch_bounds__(64)
k_mix_fields(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, const uint32_t* __restrict__ sel, unsigned n_sel,
             const uint32_t* __restrict__ pack_ptr, const uint32_t* __restrict__ pack_bits, const Fr* __restrict__ scratch, size_t slots,
             uint64_t* __restrict__ out) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    const size_t w = blockIdx.y;
    const size_t j = (word0 + w) * 64 + lane;
    if (j >= count) return;
    const uint32_t s = sel[i], at = s & MIX_INDEX;
    uint4 lo, hi;
    if ((s & MIX_TAG) == MIX_PACK) {
        pack_gather(state, nw, w, pack_bits, pack_ptr[at], pack_ptr[at + 1], lane, lo, hi);
    } else if ((s & MIX_TAG) == MIX_BIT) {
        lo = make_uint4((unsigned)((state[(size_t)at * nw + w] >> lane) & 1), 0, 0, 0);
        hi = make_uint4(0, 0, 0, 0);
    } else {
        const Fr x = scratch[(w * slots + at) * WG_LANES + lane].to_canonical();
        lo = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        hi = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    }
    uint4* o = reinterpret_cast<uint4*>(out + (j * n_sel + i) * 4);
    o[0] = lo;
    o[1] = hi;
}

static zk_mixgen* mixgen_create(zk_ctx* ctx, const zk_circuit& c) {
    ZK_REQUIRE(c.built, ZK_ERR_UNSUPPORTED, "mixgen: a parsed program has no boolean core; use zk_witgen_create");
    const Mixed& x = c.built->mix;
    const Tape& t = x.tail;
    const size_t m = c.u.size();
    const long gw = ctx->opt_boolgen_group_words;
    ZK_REQUIRE(gw == 0 || gw == 1 || gw == 2 || gw == 4 || gw == 8, ZK_ERR_ARG, "mixgen: option boolgen_group_words must be 0, 1, 2, 4 or 8");
    std::unique_ptr<zk_mixgen> g(new zk_mixgen());
    g->ctx = ctx;
    g->n_bit = x.bit_in_wit.size(); g->n_field = t.n_in; g->m = m;
    g->levels = x.core_level_ptr.size() - 1;
    g->slots = t.slots; g->n_store = x.slot_wit.size(); g->tail_levels = t.levels();
    g->waves = witgen_waves(t);
    g->scratch_cap = (size_t)std::max<long>(ctx->opt_boolgen_scratch_kib, 0) * 1024;
    g->group_words = (unsigned)gw;
    g->expand_pair = ctx->opt_boolgen_expand_form != 0;
    const size_t word_bytes = (m + 1) * sizeof(uint64_t) + g->slots * WG_LANES * sizeof(Fr);
    ZK_REQUIRE(g->scratch_cap >= word_bytes, ZK_ERR_SIZE,
               "mixgen: one word of 64 instances needs " + std::to_string((word_bytes + 1023) >> 10) +
                   " KiB of state and tail scratch, more than the option boolgen_scratch_kib allows");
    hipStream_t st = ctx->stream;
    auto up = [&](auto& buf, const auto& host) {
        buf.alloc(std::max<size_t>(host.size(), 1));   // never a null array
        if (!host.empty()) ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, st));
    };
    up(g->ops, x.core_ops);
    up(g->level_ptr, x.core_level_ptr);
    up(g->bit_in_wit, x.bit_in_wit);
    g->n_packs = x.cpack_out.size();
    up(g->pack_out, x.cpack_out);
    up(g->pack_ptr, x.cpack_ptr);
    up(g->pack_bits, x.cpack_bits);
    up(g->tail_ops, t.ops);
    const std::vector<uint32_t> lp = t.level_ptr.empty() ? std::vector<uint32_t>{0} : t.level_ptr;
    up(g->tail_level_ptr, lp);
    up(g->slot_wit, x.slot_wit);
    up(g->consts, t.consts);
    g->flag.alloc(1);
    g->ref.resize(m);
    for (size_t i = 0; i < m; ++i) g->ref[i] = MIX_BIT | (uint32_t)i;
    for (size_t p = 0; p < x.cpack_out.size(); ++p) g->ref[x.cpack_out[p]] = MIX_PACK | (uint32_t)p;
    for (size_t s = 0; s < x.slot_wit.size(); ++s) g->ref[x.slot_wit[s]] = MIX_SLOT | (uint32_t)s;
    ZK_HIP(hipStreamSynchronize(st));   // the host vectors may go away with the circuit
    return g.release();
}

// per chunk: load, the core, `expand(word0, words)`, the tail (storing to d_out unless it is null), `gather(word0, words)`; then the
// refusal of a field input >= r, naming the lowest such instance
template <class Expand, class Gather>
static void mixgen_chunks(zk_mixgen& g, const void* d_in, size_t stride, const void* d_fields, size_t count, void* d_out, Expand&& expand,
                          Gather&& gather) {
    zk_ctx* ctx = g.ctx;
    hipStream_t st = ctx->stream;
    const size_t word_bytes = (g.m + 1) * sizeof(uint64_t) + g.slots * WG_LANES * sizeof(Fr);
    const size_t words = (count + 63) / 64;
    const size_t chunk = std::min(std::min(words, g.scratch_cap / word_bytes), BG_MAX_CHUNK_WORDS);   // >= 1: checked at create
    g.state.ensure(chunk * (g.m + 1));
    g.scratch.ensure(std::max<size_t>(chunk * g.slots * WG_LANES, 1));
    const unsigned long long none = WG_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(g.flag.p, &none, sizeof(none), hipMemcpyHostToDevice, st));
    for (size_t w0 = 0; w0 < words; w0 += chunk) {       // same stream: a chunk starts when the one before has left state and scratch
        const size_t nw = std::min(chunk, words - w0);
        const unsigned G = g.group_words ? g.group_words : boolgen_group_words(nw, ctx->cu_count);
        unsigned g_log = 0;
        while ((1u << g_log) < G) ++g_log;
        {
            ProfScope ps(ctx, "mixgen_load", 0.0);
            hipLaunchKernelGGL(k_bool_load, dim3((unsigned)nw), dim3(64 * BG_LOAD_WAVES), 0, st, (const uint8_t*)d_in, stride, count, w0, g.bit_in_wit.p,
                               (unsigned)g.n_bit, (unsigned)g.m, nw, g.state.p);
        }
        if (g.levels) {
            ProfScope ps(ctx, "mixgen_eval", 0.0);
            hipLaunchKernelGGL(k_bool_eval, dim3((unsigned)((nw + G - 1) / G)), dim3(BG_EVAL_THREADS), 0, st, g.ops.p, g.level_ptr.p, (unsigned)g.levels,
                               g_log, nw, g.state.p);
        }
        ZK_HIP(hipGetLastError());
        expand(w0, nw);
        if (g.slots) {
            ProfScope ps(ctx, "mixgen_tail", 0.0);
            hipLaunchKernelGGL(k_mix_tail, dim3((unsigned)nw), dim3(WG_LANES * g.waves), 0, st, g.tail_ops.p, g.tail_level_ptr.p, (unsigned)g.tail_levels,
                               g.consts.p, g.slot_wit.p, (unsigned)g.n_store, (const uint64_t*)d_fields, (unsigned)g.n_field, (unsigned)g.m, g.slots,
                               g.state.p, nw, w0, count, g.pack_ptr.p, g.pack_bits.p, g.scratch.p, (uint64_t*)d_out, g.flag.p);
        }
        ZK_HIP(hipGetLastError());
        gather(w0, nw);
        ZK_HIP(hipGetLastError());
    }
    unsigned long long bad = WG_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(&bad, g.flag.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ctx->resolve_profile();
    ZK_REQUIRE(bad == WG_NO_ERROR, ZK_ERR_RANGE, "mixgen: input value >= r in instance " + std::to_string(bad));
}

static void mixgen_run(zk_mixgen& g, const void* d_in, size_t stride, const void* d_fields, size_t count, void* d_out) {
    zk_ctx* ctx = g.ctx;
    mixgen_chunks(g, d_in, stride, d_fields, count, d_out, [&](size_t w0, size_t nw) {
        const size_t inst = std::min(count - w0 * 64, nw * 64);
        {
            ProfScope ps(ctx, "mixgen_expand", (double)inst * g.m * 32.0);
            if (g.expand_pair)
                hipLaunchKernelGGL(k_bool_expand_pair, dim3(ceil_div(2 * g.m, BG_EXPAND_THREADS), (unsigned)nw), dim3(BG_EXPAND_THREADS), 0, ctx->stream,
                                   g.state.p, nw, w0, count, (unsigned)g.m, (uint64_t*)d_out);
            else
                hipLaunchKernelGGL(k_bool_expand, dim3(ceil_div(g.m, BG_EXPAND_THREADS), (unsigned)nw), dim3(BG_EXPAND_THREADS), 0, ctx->stream, g.state.p,
                                   nw, w0, count, (unsigned)g.m, (uint64_t*)d_out);
        }
        if (g.n_packs) {   // behind the expansion on the same stream: the packed indices' 32 bytes are overwritten
            ProfScope pp(ctx, "mixgen_expand_packs", (double)inst * g.n_packs * 32.0);
            hipLaunchKernelGGL(k_bool_expand_packs, dim3((unsigned)g.n_packs, (unsigned)nw), dim3(64), 0, ctx->stream, g.state.p, nw, w0, count,
                               (unsigned)g.m, g.pack_out.p, g.pack_ptr.p, g.pack_bits.p, (uint64_t*)d_out);
        }
    }, [](size_t, size_t) {});
}

static void mixgen_eval_fields(zk_mixgen& g, const void* d_in, size_t stride, const void* d_fields, size_t count, const uint32_t* wires, size_t n_wires,
                               void* d_out) {
    zk_ctx* ctx = g.ctx;
    std::vector<uint32_t> sel(n_wires);
    for (size_t i = 0; i < n_wires; ++i) sel[i] = g.ref[wires[i]];
    g.sel.ensure(n_wires);
    ZK_HIP(hipMemcpyAsync(g.sel.p, sel.data(), n_wires * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));   // sel is pageable host memory that goes away
    mixgen_chunks(g, d_in, stride, d_fields, count, nullptr, [](size_t, size_t) {}, [&](size_t w0, size_t nw) {
        const size_t inst = std::min(count - w0 * 64, nw * 64);
        ProfScope ps(ctx, "mixgen_fields", (double)inst * n_wires * 32.0);
        hipLaunchKernelGGL(k_mix_fields, dim3((unsigned)n_wires, (unsigned)nw), dim3(64), 0, ctx->stream, g.state.p, nw, w0, count, g.sel.p,
                           (unsigned)n_wires, g.pack_ptr.p, g.pack_bits.p, g.scratch.p, g.slots, (uint64_t*)d_out);
    });
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_mixgen_create(zk_ctx* ctx, const zk_circuit* c, zk_mixgen** out) {
    if (!ctx || !c || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return guarded(ctx, [&] { *out = mixgen_create(ctx, *c); });
}
void zk_mixgen_free(zk_mixgen* g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    delete g;
}
int zk_mixgen_run(zk_mixgen* g, const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count, void* d_weights_out, size_t m) {
    if (!g) return ZK_ERR_ARG;
    return guarded(g->ctx, [&] {
        ZK_REQUIRE(m == g->m, ZK_ERR_ARG, "StructureErr(None, weights buffer size mismatch)");
        ZK_REQUIRE(in_stride_bytes >= (g->n_bit + 7) / 8, ZK_ERR_ARG, "mixgen: in_stride_bytes is shorter than the packed bit inputs of one instance");
        if (count == 0) return;
        ZK_REQUIRE(d_weights_out && (d_in_bits || !g->n_bit) && (d_in_fields || !g->n_field), ZK_ERR_ARG, "mixgen: null device pointer");
        mixgen_run(*g, d_in_bits, in_stride_bytes, d_in_fields, count, d_weights_out);
    });
}
int zk_mixgen_eval_fields(zk_mixgen* g, const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count, const uint32_t* wires,
                          size_t n_wires, void* d_out_words) {
    if (!g) return ZK_ERR_ARG;
    return guarded(g->ctx, [&] {
        ZK_REQUIRE(in_stride_bytes >= (g->n_bit + 7) / 8, ZK_ERR_ARG, "mixgen: in_stride_bytes is shorter than the packed bit inputs of one instance");
        ZK_REQUIRE(wires || !n_wires, ZK_ERR_ARG, "mixgen: null wire list");
        ZK_REQUIRE(n_wires < (1u << 31), ZK_ERR_ARG, "mixgen: too many wires named");
        for (size_t i = 0; i < n_wires; ++i)
            ZK_REQUIRE(wires[i] < g->m, ZK_ERR_ARG, "mixgen: witness index " + std::to_string(wires[i]) + " is not below m");
        if (count == 0 || n_wires == 0) return;
        ZK_REQUIRE(d_out_words && (d_in_bits || !g->n_bit) && (d_in_fields || !g->n_field), ZK_ERR_ARG, "mixgen: null device pointer");
        mixgen_eval_fields(*g, d_in_bits, in_stride_bytes, d_in_fields, count, wires, n_wires, d_out_words);
    });
}

}  // extern "C"
