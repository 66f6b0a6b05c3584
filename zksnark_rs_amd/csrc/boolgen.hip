// boolgen.hip -- zk_boolgen_*: the witnesses of a BOOLEAN built circuit (builder.hpp) for many input sets at once, bit-sliced.
//
// Where k_witgen (witgen.hip) keeps a 32-byte Montgomery slot per wire and instance and pays a 254-bit multiplication per AND, every
// value here is 0 or 1, so a wire is one uint64 per 64 instances and a gate one 64-bit logic operation for all 64 of them.
//   state      uint64 per (witness index, instance word), index-major: state[s * nw + w]; bit l of word w is instance 64 w + l.
//              Index 0 is the constant 1 (all ones), index m the constant 0.
//   load       a transposition (k_bool_load): lane = instance, one wave64 __ballot per input bit is that input's word.  Instances
//              behind `count` in the last word load 0 and are never written out.
//   evaluate   the circuit's boolean tape (one op per sub-circuit, sorted by level), level by level (k_bool_eval): a workgroup owns G
//              consecutive instance words, the (op, word) pairs of a level are strided over its lanes with the word index fastest,
//              so neighbouring lanes touch neighbouring words of one slot; __syncthreads() between levels.  No lane returns early.
//   expand     the bandwidth step (k_bool_expand): (instance, wire) -> 32 bytes, word 0 = the bit, words 1..3 = 0, instance-major:
//              exactly what zk_witgen_run writes.  Lane = wire: it loads its slot's word once and walks the 64 instances; a wave's
//              stores cover 2 KiB contiguous of one instance's witness.
//   pack       zk_boolgen_eval instead of expand (k_bool_pack): the named wires only, packed the way the inputs are.
//   packed wires   (zk_builder_pack: out = sum 2^i b_i over at most 253 bit-valued operands) are no boolean operation and have no state:
//              the value is below 2^253 < r, so its 4 canonical words ARE the operands' bits, gathered (pack_gather) -- no field
//              arithmetic.  k_bool_expand_packs runs behind the expansion on the same stream and overwrites the 32 bytes the
//              expansion wrote for a packed index from its never-written state slot, so no byte that is left depends on that slot;
//              k_bool_pack_fields (zk_boolgen_eval_fields) returns named wires, bits and packed ones alike, as field elements.
// Words run in chunks of as many as the scratch cap holds (option "boolgen_scratch_kib"); every word is independent of the others, so
// the result does not depend on the chunking.  The kernels are in boolgen_kernels.cuh, which mixgen.hip shares: there a circuit that is
// not boolean in every wire runs its boolean core through them and its field tail through k_mix_tail.
#include "boolgen_kernels.cuh"

struct zk_boolgen {
    zk_ctx* ctx = nullptr;
    size_t n_in = 0, m = 0, levels = 0;
    size_t scratch_cap = 0;                 // bytes
    unsigned group_words = 0;               // 0 = by rule
    bool expand_pair = false;
    zk::DevBuf<zk::BoolOp> ops;
    zk::DevBuf<uint32_t> level_ptr, in_wit, sel;
    size_t n_packs = 0;
    zk::DevBuf<uint32_t> pack_out, pack_ptr, pack_bits;      // Built's CSR lists
    std::vector<std::pair<uint32_t, uint32_t>> pack_of;      // (witness index, pack) sorted by index: which named wires are packed
    zk::DevBuf<uint64_t> state;
};

namespace zk {

// grid: one workgroup per word of the chunk; lane = instance
__global__ void __launch_bounds__(64 * BG_LOAD_WAVES)
k_bool_pack(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, const uint32_t* __restrict__ sel, unsigned n_sel,
            uint8_t* __restrict__ out, size_t stride) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t w = blockIdx.x;
    const size_t j = (word0 + w) * 64 + lane;
    const bool live = j < count;
    const unsigned n_bytes = (n_sel + 7) / 8;
    for (unsigned k = wave; k < n_bytes; k += BG_LOAD_WAVES) {
        const unsigned bits = min(8u, n_sel - 8 * k);
        unsigned v = 0;
        for (unsigned b = 0; b < bits; ++b) v |= (unsigned)((state[(size_t)sel[8 * k + b] * nw + w] >> lane) & 1) << b;
        if (live) out[j * stride + k] = (uint8_t)v;
    }
}

constexpr uint32_t BG_SEL_PACKED = 0x80000000u;   // sel entry: this bit | the pack's number, else a state slot (m < 2^31)

// grid: (named wires, words of the chunk); one wave, lane = instance: out[(j * n_sel + i) * 4 ..] = wire sel[i] as 4 canonical words
__global__ void __launch_bounds__(64)
k_bool_pack_fields(const uint64_t* __restrict__ state, size_t nw, size_t word0, size_t count, const uint32_t* __restrict__ sel, unsigned n_sel,
                   const uint32_t* __restrict__ pack_ptr, const uint32_t* __restrict__ pack_bits, uint64_t* __restrict__ out) {
    const unsigned i = blockIdx.x, lane = threadIdx.x;
    const size_t w = blockIdx.y;
    const uint32_t s = sel[i];
    uint4 lo, hi;
    if (s & BG_SEL_PACKED) {
        const unsigned p = s & ~BG_SEL_PACKED;
        pack_gather(state, nw, w, pack_bits, pack_ptr[p], pack_ptr[p + 1], lane, lo, hi);
    } else {
        lo = make_uint4((unsigned)((state[(size_t)s * nw + w] >> lane) & 1), 0, 0, 0);
        hi = make_uint4(0, 0, 0, 0);
    }
    const size_t j = (word0 + w) * 64 + lane;
    if (j >= count) return;
    uint4* o = reinterpret_cast<uint4*>(out + (j * n_sel + i) * 4);
    o[0] = lo;
    o[1] = hi;
}

static zk_boolgen* boolgen_create(zk_ctx* ctx, const zk_circuit& c) {
    ZK_REQUIRE(c.built && c.built->boolean, ZK_ERR_UNSUPPORTED,
               "boolgen: the circuit is not boolean (a parsed program, a field input, a general sub-circuit or a packed wire that is read); "
               "use zk_witgen_create");
    const Built& p = *c.built;
    const size_t m = c.u.size();
    ZK_REQUIRE(m < (1u << 31) && p.bool_ops.size() < (1u << 31), ZK_ERR_SIZE, "boolgen: circuit too large");
    const long gw = ctx->opt_boolgen_group_words;
    ZK_REQUIRE(gw == 0 || gw == 1 || gw == 2 || gw == 4 || gw == 8, ZK_ERR_ARG, "boolgen: option boolgen_group_words must be 0, 1, 2, 4 or 8");
    std::unique_ptr<zk_boolgen> g(new zk_boolgen());
    g->ctx = ctx;
    g->n_in = p.in_wit.size(); g->m = m;
    g->levels = p.bool_level_ptr.empty() ? 0 : p.bool_level_ptr.size() - 1;
    g->scratch_cap = (size_t)std::max<long>(ctx->opt_boolgen_scratch_kib, 0) * 1024;
    g->group_words = (unsigned)gw;
    g->expand_pair = ctx->opt_boolgen_expand_form != 0;
    hipStream_t st = ctx->stream;
    auto up = [&](auto& buf, const auto& host) {
        buf.alloc(std::max<size_t>(host.size(), 1));   // never a null array
        if (!host.empty()) ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, st));
    };
    up(g->ops, p.bool_ops);
    up(g->in_wit, p.in_wit);
    const std::vector<uint32_t> lp = p.bool_level_ptr.empty() ? std::vector<uint32_t>{0} : p.bool_level_ptr;
    up(g->level_ptr, lp);
    g->n_packs = p.pack_out.size();
    ZK_REQUIRE(g->n_packs < (1u << 31), ZK_ERR_SIZE, "boolgen: circuit too large");
    up(g->pack_out, p.pack_out);
    up(g->pack_ptr, p.pack_ptr);
    up(g->pack_bits, p.pack_bits);
    for (size_t k = 0; k < g->n_packs; ++k) g->pack_of.push_back({p.pack_out[k], (uint32_t)k});
    std::sort(g->pack_of.begin(), g->pack_of.end());
    ZK_HIP(hipStreamSynchronize(st));   // the host vectors may go away with the circuit
    return g.release();
}

// load + evaluate per chunk, then `emit(word0, words, nw)` on the chunk's state
template <class Emit>
static void boolgen_chunks(zk_boolgen& g, const void* d_in, size_t stride, size_t count, Emit&& emit) {
    zk_ctx* ctx = g.ctx;
    hipStream_t st = ctx->stream;
    const size_t word_bytes = (g.m + 1) * sizeof(uint64_t);
    const size_t words = (count + 63) / 64;
    const size_t fit = g.scratch_cap / word_bytes;
    ZK_REQUIRE(fit >= 1, ZK_ERR_SIZE, "boolgen: one word of 64 instances needs " + std::to_string((word_bytes + 1023) >> 10) +
                                          " KiB of scratch, more than the option boolgen_scratch_kib allows");
    const size_t chunk = std::min(std::min(words, fit), BG_MAX_CHUNK_WORDS);
    g.state.ensure(chunk * (g.m + 1));
    for (size_t w0 = 0; w0 < words; w0 += chunk) {       // same stream: a chunk starts when the one before has left the state
        const size_t nw = std::min(chunk, words - w0);
        const unsigned G = g.group_words ? g.group_words : boolgen_group_words(nw, ctx->cu_count);
        unsigned g_log = 0;
        while ((1u << g_log) < G) ++g_log;
        {
            ProfScope ps(ctx, "boolgen_load", 0.0);
            hipLaunchKernelGGL(k_bool_load, dim3((unsigned)nw), dim3(64 * BG_LOAD_WAVES), 0, st, (const uint8_t*)d_in, stride, count, w0, g.in_wit.p,
                               (unsigned)g.n_in, (unsigned)g.m, nw, g.state.p);
        }
        if (g.levels) {
            ProfScope ps(ctx, "boolgen_eval", 0.0);
            hipLaunchKernelGGL(k_bool_eval, dim3((unsigned)((nw + G - 1) / G)), dim3(BG_EVAL_THREADS), 0, st, g.ops.p, g.level_ptr.p, (unsigned)g.levels,
                               g_log, nw, g.state.p);
        }
        ZK_HIP(hipGetLastError());
        emit(w0, nw);
        ZK_HIP(hipGetLastError());
    }
    ZK_HIP(hipStreamSynchronize(st));
    ctx->resolve_profile();
}

static void boolgen_run(zk_boolgen& g, const void* d_in, size_t stride, size_t count, void* d_out) {
    zk_ctx* ctx = g.ctx;
    boolgen_chunks(g, d_in, stride, count, [&](size_t w0, size_t nw) {
        const size_t inst = std::min(count - w0 * 64, nw * 64);
        {
            ProfScope ps(ctx, "boolgen_expand", (double)inst * g.m * 32.0);
            if (g.expand_pair)
                hipLaunchKernelGGL(k_bool_expand_pair, dim3(ceil_div(2 * g.m, BG_EXPAND_THREADS), (unsigned)nw), dim3(BG_EXPAND_THREADS), 0, ctx->stream,
                                   g.state.p, nw, w0, count, (unsigned)g.m, (uint64_t*)d_out);
            else
                hipLaunchKernelGGL(k_bool_expand, dim3(ceil_div(g.m, BG_EXPAND_THREADS), (unsigned)nw), dim3(BG_EXPAND_THREADS), 0, ctx->stream, g.state.p,
                                   nw, w0, count, (unsigned)g.m, (uint64_t*)d_out);
        }
        if (g.n_packs) {   // behind the expansion on the same stream: the packed indices' 32 bytes are overwritten
            ProfScope pp(ctx, "boolgen_expand_packs", (double)inst * g.n_packs * 32.0);
            hipLaunchKernelGGL(k_bool_expand_packs, dim3((unsigned)g.n_packs, (unsigned)nw), dim3(64), 0, ctx->stream, g.state.p, nw, w0, count,
                               (unsigned)g.m, g.pack_out.p, g.pack_ptr.p, g.pack_bits.p, (uint64_t*)d_out);
        }
    });
}

// the pack of witness index s, or -1
static long boolgen_pack_of(const zk_boolgen& g, uint32_t s) {
    auto it = std::lower_bound(g.pack_of.begin(), g.pack_of.end(), std::make_pair(s, (uint32_t)0));
    return it != g.pack_of.end() && it->first == s ? (long)it->second : -1;
}

static void boolgen_eval_fields(zk_boolgen& g, const void* d_in, size_t stride, size_t count, const uint32_t* wires, size_t n_wires, void* d_out) {
    zk_ctx* ctx = g.ctx;
    std::vector<uint32_t> sel(n_wires);
    for (size_t i = 0; i < n_wires; ++i) {
        const long p = boolgen_pack_of(g, wires[i]);
        sel[i] = p < 0 ? wires[i] : (BG_SEL_PACKED | (uint32_t)p);
    }
    g.sel.ensure(n_wires);
    ZK_HIP(hipMemcpyAsync(g.sel.p, sel.data(), n_wires * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));   // sel is pageable host memory that goes away
    boolgen_chunks(g, d_in, stride, count, [&](size_t w0, size_t nw) {
        const size_t inst = std::min(count - w0 * 64, nw * 64);
        ProfScope ps(ctx, "boolgen_pack_fields", (double)inst * n_wires * 32.0);
        hipLaunchKernelGGL(k_bool_pack_fields, dim3((unsigned)n_wires, (unsigned)nw), dim3(64), 0, ctx->stream, g.state.p, nw, w0, count, g.sel.p,
                           (unsigned)n_wires, g.pack_ptr.p, g.pack_bits.p, (uint64_t*)d_out);
    });
}

static void boolgen_eval(zk_boolgen& g, const void* d_in, size_t stride, size_t count, const uint32_t* wires, size_t n_wires, void* d_out,
                         size_t out_stride) {
    zk_ctx* ctx = g.ctx;
    g.sel.ensure(std::max<size_t>(n_wires, 1));
    if (n_wires) ZK_HIP(hipMemcpyAsync(g.sel.p, wires, n_wires * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    boolgen_chunks(g, d_in, stride, count, [&](size_t w0, size_t nw) {
        ProfScope ps(ctx, "boolgen_pack", 0.0);
        hipLaunchKernelGGL(k_bool_pack, dim3((unsigned)nw), dim3(64 * BG_LOAD_WAVES), 0, ctx->stream, g.state.p, nw, w0, count, g.sel.p, (unsigned)n_wires,
                           (uint8_t*)d_out, out_stride);
    });
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_boolgen_create(zk_ctx* ctx, const zk_circuit* c, zk_boolgen** out) {
    if (!ctx || !c || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return guarded(ctx, [&] { *out = boolgen_create(ctx, *c); });
}
void zk_boolgen_free(zk_boolgen* g) {
    if (!g) return;
    (void)hipSetDevice(g->ctx->device);
    delete g;
}
int zk_boolgen_run(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, void* d_weights_out, size_t m) {
    if (!g) return ZK_ERR_ARG;
    return guarded(g->ctx, [&] {
        ZK_REQUIRE(m == g->m, ZK_ERR_ARG, "StructureErr(None, weights buffer size mismatch)");
        ZK_REQUIRE(in_stride_bytes >= (g->n_in + 7) / 8, ZK_ERR_ARG, "boolgen: in_stride_bytes is shorter than the packed inputs of one instance");
        if (count == 0) return;
        ZK_REQUIRE(d_weights_out && (d_in_bits || !g->n_in), ZK_ERR_ARG, "boolgen: null device pointer");
        boolgen_run(*g, d_in_bits, in_stride_bytes, count, d_weights_out);
    });
}
int zk_boolgen_eval(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, const uint32_t* wires, size_t n_wires,
                    void* d_out_bits, size_t out_stride_bytes) {
    if (!g) return ZK_ERR_ARG;
    return guarded(g->ctx, [&] {
        ZK_REQUIRE(in_stride_bytes >= (g->n_in + 7) / 8, ZK_ERR_ARG, "boolgen: in_stride_bytes is shorter than the packed inputs of one instance");
        ZK_REQUIRE(out_stride_bytes >= (n_wires + 7) / 8, ZK_ERR_ARG, "boolgen: out_stride_bytes is shorter than the packed wires of one instance");
        ZK_REQUIRE(wires || !n_wires, ZK_ERR_ARG, "boolgen: null wire list");
        ZK_REQUIRE(n_wires < (1u << 31), ZK_ERR_ARG, "boolgen: too many wires named");
        for (size_t i = 0; i < n_wires; ++i)
            ZK_REQUIRE(wires[i] < g->m, ZK_ERR_ARG, "boolgen: witness index " + std::to_string(wires[i]) + " is not below m");
        for (size_t i = 0; i < n_wires; ++i)
            ZK_REQUIRE(boolgen_pack_of(*g, wires[i]) < 0, ZK_ERR_ARG,
                       "boolgen: witness index " + std::to_string(wires[i]) + " is a packed wire, not a bit; use zk_boolgen_eval_fields");
        if (count == 0 || n_wires == 0) return;
        ZK_REQUIRE(d_out_bits && (d_in_bits || !g->n_in), ZK_ERR_ARG, "boolgen: null device pointer");
        boolgen_eval(*g, d_in_bits, in_stride_bytes, count, wires, n_wires, d_out_bits, out_stride_bytes);
    });
}
int zk_boolgen_eval_fields(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, const uint32_t* wires, size_t n_wires,
                           void* d_out_words) {
    if (!g) return ZK_ERR_ARG;
    return guarded(g->ctx, [&] {
        ZK_REQUIRE(in_stride_bytes >= (g->n_in + 7) / 8, ZK_ERR_ARG, "boolgen: in_stride_bytes is shorter than the packed inputs of one instance");
        ZK_REQUIRE(wires || !n_wires, ZK_ERR_ARG, "boolgen: null wire list");
        ZK_REQUIRE(n_wires < (1u << 31), ZK_ERR_ARG, "boolgen: too many wires named");
        for (size_t i = 0; i < n_wires; ++i)
            ZK_REQUIRE(wires[i] < g->m, ZK_ERR_ARG, "boolgen: witness index " + std::to_string(wires[i]) + " is not below m");
        if (count == 0 || n_wires == 0) return;
        ZK_REQUIRE(d_out_words && (d_in_bits || !g->n_in), ZK_ERR_ARG, "boolgen: null device pointer");
        boolgen_eval_fields(*g, d_in_bits, in_stride_bytes, count, wires, n_wires, d_out_words);
    });
}

}  // extern "C"
