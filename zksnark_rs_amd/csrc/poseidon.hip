// poseidon.hip -- Poseidon (poseidon.hpp) on the device: zk_poseidon_hash_batch, one hash per lane, and zk_poseidon_tree_*, a binary
// Merkle tree that stays on the device and hands out authentication paths in the layout zk_mixgen_run reads.
//   k_poseidon<T>       one hash per lane, the state of T elements in registers.  Inputs are canonical words: range-checked (a word
//                       pattern >= r: atomicMin into a flag, the arrangement of k_mix_tail), to Montgomery form on load, the digest to
//                       canonical form on store.  The round constants and M sit in one per-context array (C, then M row-major, Montgomery
//                       form) read through a const __restrict__ pointer at an index that is the same in every lane, in three rolled
//                       loops -- full, partial, full rounds -- so each constant is fetched once per wave, by scalar loads.  No LDS, no
//                       private array indexed at run time: the state is indexed through index sequences only.
//                       The tree uses the same kernel over PAIRS of a level: input element e of the launch is read only while
//                       e < avail, and is `fill` (the zero hash of that level) behind it.
//   k_poseidon_paths    one lane per (instance, slot): slot 0 copies the leaf and writes the direction bytes, slot 1 + k copies the
//                       sibling of level k, or z_k where the tree stores none.
// Per-hash cost for arity 2: 3 (R_F t + R_P) = 243 multiplications in the S-boxes and t^2 (R_F + R_P) = 585 in the mix.
#include <utility>
#include "common.hpp"
#include "poseidon.hpp"

namespace zk {

static constexpr unsigned POSEIDON_BLOCK = 256;
static constexpr unsigned long long POSEIDON_NO_ERROR = ~0ull;

// the per-context device copy of the parameters: par[arity] = C | M, uploaded on first use
struct PoseidonState {
    DevBuf<Fr> par[POSEIDON_MAX_T];
    DevBuf<unsigned long long> flag;
};

// The state is an array indexed through index sequences only: every index is a compile-time constant, so the elements are registers
// whatever the optimizer decides about loops.
template <unsigned N>
using PoseidonSeq = std::make_integer_sequence<unsigned, N>;

__device__ __forceinline__ Fr poseidon_pow5_dev(const Fr& x) {
    const Fr x2 = x.sqr();
    return x2.sqr() * x;
}
template <unsigned T, unsigned... I>
__device__ __forceinline__ void poseidon_add(Fr (&s)[T], const Fr* __restrict__ c, std::integer_sequence<unsigned, I...>) {
    ((s[I] = s[I] + c[I]), ...);
}
template <unsigned T, unsigned... I>
__device__ __forceinline__ void poseidon_sbox_all(Fr (&s)[T], std::integer_sequence<unsigned, I...>) {
    ((s[I] = poseidon_pow5_dev(s[I])), ...);
}
// row i of M times the state; J runs over 0 .. T - 2 and names column J + 1
template <unsigned T, unsigned... J>
__device__ __forceinline__ Fr poseidon_row(const Fr (&s)[T], const Fr* __restrict__ row, std::integer_sequence<unsigned, J...>) {
    Fr acc = row[0] * s[0];
    ((acc = acc + row[J + 1] * s[J + 1]), ...);
    return acc;
}
template <unsigned T, unsigned... I>
__device__ __forceinline__ void poseidon_mix(Fr (&s)[T], const Fr* __restrict__ m, std::integer_sequence<unsigned, I...>) {
    Fr n[T];
    ((n[I] = poseidon_row<T>(s, m + I * T, PoseidonSeq<T - 1>())), ...);
    ((s[I] = n[I]), ...);
}
template <unsigned T>
__device__ __forceinline__ void poseidon_full_round(Fr (&s)[T], const Fr* __restrict__ c, const Fr* __restrict__ m) {
    poseidon_add<T>(s, c, PoseidonSeq<T>());
    poseidon_sbox_all<T>(s, PoseidonSeq<T>());
    poseidon_mix<T>(s, m, PoseidonSeq<T>());
}
template <unsigned T>
__device__ __forceinline__ void poseidon_partial_round(Fr (&s)[T], const Fr* __restrict__ c, const Fr* __restrict__ m) {
    poseidon_add<T>(s, c, PoseidonSeq<T>());
    s[0] = poseidon_pow5_dev(s[0]);
    poseidon_mix<T>(s, m, PoseidonSeq<T>());
}
// one input element: canonical words -> Montgomery form, or `fill` behind `avail`
__device__ __forceinline__ Fr poseidon_load(const uint64_t* __restrict__ in, size_t e, size_t avail, const Fr& fill, unsigned long long* __restrict__ flag,
                                            unsigned long long report) {
    if (e >= avail) return fill;
    const uint4* src = reinterpret_cast<const uint4*>(in + 4 * e);
    const uint4 lo = src[0], hi = src[1];
    Fr x;
    x.l[0] = lo.x; x.l[1] = lo.y; x.l[2] = lo.z; x.l[3] = lo.w;
    x.l[4] = hi.x; x.l[5] = hi.y; x.l[6] = hi.z; x.l[7] = hi.w;
    if (!x.raw_in_range()) atomicMin(flag, report);
    return Fr::from_canonical(x);
}
template <unsigned T, unsigned... I>
__device__ __forceinline__ void poseidon_load_all(Fr (&s)[T], const uint64_t* __restrict__ in, size_t j, size_t avail, const Fr& fill,
                                                  unsigned long long* __restrict__ flag, int flag_elem, std::integer_sequence<unsigned, I...>) {
    s[0] = Fr::zero();
    ((s[I + 1] = poseidon_load(in, j * (T - 1) + I, avail, fill, flag, flag_elem ? j * (T - 1) + I : j)), ...);
}

// grid: ceil(count / POSEIDON_BLOCK) blocks; lane j hashes input elements j (T - 1) .. j (T - 1) + T - 2.  flag_elem != 0: the flag
// records the lowest ELEMENT >= r (the tree: a leaf), else the lowest lane (the batch: an instance).
template <unsigned T>
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon(const Fr* __restrict__ par, unsigned rp, const uint64_t* __restrict__ in, size_t avail, size_t count, Fr fill, uint64_t* __restrict__ out,
           unsigned long long* __restrict__ flag, int flag_elem) {
    const size_t j = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    if (j >= count) return;
    Fr s[T];
    poseidon_load_all<T>(s, in, j, avail, fill, flag, flag_elem, PoseidonSeq<T - 1>());
    const Fr* __restrict__ c = par;
    const Fr* __restrict__ m = par + (size_t)(POSEIDON_RF + rp) * T;
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += T) poseidon_full_round<T>(s, c, m);
#pragma unroll 1
    for (unsigned r = 0; r < rp; ++r, c += T) poseidon_partial_round<T>(s, c, m);
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += T) poseidon_full_round<T>(s, c, m);
    const Fr d = s[0].to_canonical();
    uint4* dst = reinterpret_cast<uint4*>(out + 4 * j);
    dst[0] = make_uint4(d.l[0], d.l[1], d.l[2], d.l[3]);
    dst[1] = make_uint4(d.l[4], d.l[5], d.l[6], d.l[7]);
}

// grid: ceil(count (depth + 1) / POSEIDON_BLOCK) blocks.  meta: per level k its offset into `nodes` (in nodes) at meta[2 k] and its
// stored size at meta[2 k + 1]; zeros: z_0 .. z_depth, canonical.
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon_paths(const uint64_t* __restrict__ nodes, const uint64_t* __restrict__ meta, const uint64_t* __restrict__ zeros, unsigned depth,
                 size_t n_leaves, const uint64_t* __restrict__ indices, size_t count, uint64_t* __restrict__ fields, size_t field_stride,
                 uint8_t* __restrict__ bits, size_t bits_stride, unsigned long long* __restrict__ flag) {
    const size_t id = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    const size_t j = id / (depth + 1);
    const unsigned slot = (unsigned)(id % (depth + 1));
    if (j >= count) return;
    const uint64_t index = indices[j];
    if (index >= n_leaves) {
        if (slot == 0) atomicMin(flag, (unsigned long long)j);
        return;
    }
    const uint64_t* src;
    if (slot == 0) {
        src = nodes + 4 * index;
        for (unsigned k = 0; k < (depth + 7) / 8; ++k) bits[j * bits_stride + k] = (uint8_t)(index >> (8 * k));
    } else {
        const unsigned k = slot - 1;
        const uint64_t sib = (index >> k) ^ 1;
        src = sib < meta[2 * k + 1] ? nodes + 4 * (meta[2 * k] + sib) : zeros + 4 * k;
    }
    uint64_t* dst = fields + j * field_stride + 4 * (size_t)slot;
#pragma unroll
    for (int w = 0; w < 4; ++w) dst[w] = src[w];
}

static PoseidonState& poseidon_state(zk_ctx* ctx, size_t arity, const PoseidonParams& p) {
    if (!ctx->poseidon) ctx->poseidon = std::make_shared<PoseidonState>();
    PoseidonState& st = *ctx->poseidon;
    if (!st.flag.p) st.flag.alloc(1);
    if (!st.par[arity].p) {
        std::vector<Fr> host(p.c);
        host.insert(host.end(), p.m.begin(), p.m.end());
        DevBuf<Fr> buf(host.size());
        ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));   // `host` goes away
        st.par[arity] = std::move(buf);
    }
    return st;
}

static void poseidon_launch(zk_ctx* ctx, size_t arity, const uint64_t* in, size_t avail, size_t count, const Fr& fill, uint64_t* out, int flag_elem) {
    const PoseidonParams& p = *poseidon_params(arity);
    PoseidonState& st = poseidon_state(ctx, arity, p);
    ZK_REQUIRE(count <= ((size_t)1 << 31) * POSEIDON_BLOCK, ZK_ERR_SIZE, "poseidon: too many hashes for one call");
    const dim3 grid(ceil_div(count, POSEIDON_BLOCK)), block(POSEIDON_BLOCK);
    ProfScope ps(ctx, "poseidon", (double)count * (arity + 1) * 32.0);
    switch (arity) {
        case 1: hipLaunchKernelGGL(k_poseidon<2>, grid, block, 0, ctx->stream, st.par[1].p, p.rp, in, avail, count, fill, out, st.flag.p, flag_elem); break;
        case 2: hipLaunchKernelGGL(k_poseidon<3>, grid, block, 0, ctx->stream, st.par[2].p, p.rp, in, avail, count, fill, out, st.flag.p, flag_elem); break;
        default: hipLaunchKernelGGL(k_poseidon<5>, grid, block, 0, ctx->stream, st.par[4].p, p.rp, in, avail, count, fill, out, st.flag.p, flag_elem); break;
    }
    ZK_HIP(hipGetLastError());
}

static void poseidon_flag_reset(zk_ctx* ctx) {
    if (!ctx->poseidon) ctx->poseidon = std::make_shared<PoseidonState>();
    if (!ctx->poseidon->flag.p) ctx->poseidon->flag.alloc(1);
    const unsigned long long none = POSEIDON_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(ctx->poseidon->flag.p, &none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
}
// waits for the stream; the lowest index an earlier launch recorded, or POSEIDON_NO_ERROR
static unsigned long long poseidon_flag_read(zk_ctx* ctx) {
    unsigned long long bad = POSEIDON_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(&bad, ctx->poseidon->flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
    return bad;
}

static void poseidon_hash_batch(zk_ctx* ctx, const void* d_in, size_t arity, size_t count, void* d_out) {
    poseidon_flag_reset(ctx);
    poseidon_launch(ctx, arity, (const uint64_t*)d_in, count * arity, count, Fr::zero(), (uint64_t*)d_out, 0);
    const unsigned long long bad = poseidon_flag_read(ctx);
    ZK_REQUIRE(bad == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon: input value >= r in instance " + std::to_string(bad));
}

}  // namespace zk

struct zk_poseidon_tree {
    zk_ctx* ctx = nullptr;
    size_t n_leaves = 0;
    unsigned depth = 0;
    std::vector<uint64_t> meta;        // per level: offset into nodes (in nodes), stored size
    zk::DevBuf<uint64_t> nodes;        // every level, canonical, 4 words per node
    zk::DevBuf<uint64_t> d_meta, zeros;
    uint64_t root[4] = {0, 0, 0, 0};
};

namespace zk {

static size_t poseidon_level_size(size_t n_leaves, unsigned level) {
    if (level == 0) return n_leaves;
    return std::max<size_t>(1, (n_leaves + (((size_t)1 << level) - 1)) >> level);
}

static zk_poseidon_tree* poseidon_tree_build(zk_ctx* ctx, const void* d_leaves, size_t n_leaves, unsigned depth) {
    ZK_REQUIRE(depth <= 32, ZK_ERR_ARG, "poseidon tree: depth " + std::to_string(depth) + " is above 32");
    ZK_REQUIRE(n_leaves <= ((size_t)1 << depth), ZK_ERR_ARG,
               "poseidon tree: " + std::to_string(n_leaves) + " leaves do not fit a tree of depth " + std::to_string(depth));
    ZK_REQUIRE(d_leaves || !n_leaves, ZK_ERR_ARG, "poseidon tree: null device pointer");
    ZK_REQUIRE((uintptr_t)d_leaves % 8 == 0, ZK_ERR_ARG, "poseidon tree: the leaves must be 8-byte aligned");
    std::unique_ptr<zk_poseidon_tree> t(new zk_poseidon_tree());
    t->ctx = ctx;
    t->n_leaves = n_leaves;
    t->depth = depth;
    size_t total = 0;
    for (unsigned k = 0; k <= depth; ++k) {
        t->meta.push_back(total);
        t->meta.push_back(poseidon_level_size(n_leaves, k));
        total += t->meta.back();
    }
    const std::vector<Fr> z = poseidon_zero_hashes(depth);
    std::vector<uint64_t> zw(4 * (size_t)(depth + 1));
    for (unsigned k = 0; k <= depth; ++k) fr_to_words(z[k].to_canonical(), zw.data() + 4 * (size_t)k);
    hipStream_t st = ctx->stream;
    t->nodes.alloc(std::max<size_t>(4 * total, 4));
    t->d_meta.alloc(t->meta.size());
    t->zeros.alloc(zw.size());
    ZK_HIP(hipMemcpyAsync(t->d_meta.p, t->meta.data(), t->meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(t->zeros.p, zw.data(), zw.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (n_leaves) ZK_HIP(hipMemcpyAsync(t->nodes.p, d_leaves, n_leaves * 32, hipMemcpyDeviceToDevice, st));
    poseidon_flag_reset(ctx);
    for (unsigned k = 0; k < depth; ++k)      // same stream: a level starts when the one below is complete
        poseidon_launch(ctx, 2, t->nodes.p + 4 * t->meta[2 * k], t->meta[2 * k + 1], t->meta[2 * k + 3], z[k], t->nodes.p + 4 * t->meta[2 * k + 2], 1);
    const unsigned long long bad = poseidon_flag_read(ctx);
    ZK_REQUIRE(bad == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon tree: leaf " + std::to_string(bad) + " is >= r");
    if (t->meta[2 * depth + 1]) {
        ZK_HIP(hipMemcpy(t->root, t->nodes.p + 4 * t->meta[2 * depth], 32, hipMemcpyDeviceToHost));
        // depth 0: no launch has looked at the one leaf
        ZK_REQUIRE(depth || fr_from_words(t->root).raw_in_range(), ZK_ERR_RANGE, "poseidon tree: leaf 0 is >= r");
    } else {
        std::memcpy(t->root, zw.data() + 4 * (size_t)depth, 32);   // no leaf, depth 0: z_0
    }
    return t.release();
}

static void poseidon_tree_paths(zk_poseidon_tree& t, const void* d_indices, size_t count, void* d_fields, size_t field_stride, void* d_bits,
                                size_t bits_stride) {
    zk_ctx* ctx = t.ctx;
    const size_t slots = (size_t)t.depth + 1;
    ZK_REQUIRE(count <= ((size_t)1 << 31), ZK_ERR_SIZE, "poseidon tree: too many paths for one call");
    poseidon_flag_reset(ctx);
    {
        ProfScope ps(ctx, "poseidon_paths", (double)count * slots * 64.0);
        hipLaunchKernelGGL(k_poseidon_paths, dim3(ceil_div(count * slots, POSEIDON_BLOCK)), dim3(POSEIDON_BLOCK), 0, ctx->stream, t.nodes.p, t.d_meta.p,
                           t.zeros.p, t.depth, t.n_leaves, (const uint64_t*)d_indices, count, (uint64_t*)d_fields, field_stride, (uint8_t*)d_bits,
                           bits_stride, ctx->poseidon->flag.p);
    }
    ZK_HIP(hipGetLastError());
    const unsigned long long bad = poseidon_flag_read(ctx);
    ZK_REQUIRE(bad == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon tree: the index of instance " + std::to_string(bad) + " is not below n_leaves");
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_poseidon_hash_batch(zk_ctx* ctx, const void* d_inputs, size_t arity, size_t count, void* d_out) {
    if (!ctx) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        ZK_REQUIRE(poseidon_rp(arity), ZK_ERR_ARG, "poseidon: the arity must be 1, 2 or 4, got " + std::to_string(arity));
        if (count == 0) return;
        ZK_REQUIRE(d_inputs && d_out, ZK_ERR_ARG, "poseidon: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_inputs | (uintptr_t)d_out) % 16 == 0, ZK_ERR_ARG, "poseidon: the device pointers must be 16-byte aligned");
        poseidon_hash_batch(ctx, d_inputs, arity, count, d_out);
    });
}
int zk_poseidon_tree_build(zk_ctx* ctx, const void* d_leaves, size_t n_leaves, unsigned depth, zk_poseidon_tree** out) {
    if (!ctx || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return guarded(ctx, [&] { *out = poseidon_tree_build(ctx, d_leaves, n_leaves, depth); });
}
void zk_poseidon_tree_free(zk_poseidon_tree* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    delete t;
}
int zk_poseidon_tree_root(const zk_poseidon_tree* t, uint64_t out[4]) {
    if (!t || !out) return ZK_ERR_ARG;
    std::memcpy(out, t->root, 32);
    return ZK_OK;
}
int zk_poseidon_tree_dims(const zk_poseidon_tree* t, size_t* n_leaves, unsigned* depth) {
    if (!t) return ZK_ERR_ARG;
    if (n_leaves) *n_leaves = t->n_leaves;
    if (depth) *depth = t->depth;
    return ZK_OK;
}
int zk_poseidon_tree_nodes(const zk_poseidon_tree* t, unsigned level, uint64_t* out) {
    if (!t) return ZK_ERR_ARG;
    return guarded(t->ctx, [&] {
        ZK_REQUIRE(level <= t->depth, ZK_ERR_ARG, "poseidon tree: level " + std::to_string(level) + " is above the depth " + std::to_string(t->depth));
        const size_t size = t->meta[2 * level + 1];
        if (!size) return;
        ZK_REQUIRE(out, ZK_ERR_ARG, "poseidon tree: null output");
        ZK_HIP(hipMemcpy(out, t->nodes.p + 4 * t->meta[2 * level], size * 32, hipMemcpyDeviceToHost));
    });
}
int zk_poseidon_tree_paths(zk_poseidon_tree* t, const void* d_indices, size_t count, void* d_fields_out, size_t field_stride_words, void* d_bits_out,
                           size_t bits_stride_bytes) {
    if (!t) return ZK_ERR_ARG;
    return guarded(t->ctx, [&] {
        ZK_REQUIRE(field_stride_words >= 4 * ((size_t)t->depth + 1), ZK_ERR_ARG, "poseidon tree: field_stride_words is shorter than leaf and siblings of one path");
        ZK_REQUIRE(bits_stride_bytes >= (t->depth + 7) / 8, ZK_ERR_ARG, "poseidon tree: bits_stride_bytes is shorter than the direction bits of one path");
        if (count == 0) return;
        ZK_REQUIRE(d_indices && d_fields_out && (d_bits_out || !t->depth), ZK_ERR_ARG, "poseidon tree: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_indices | (uintptr_t)d_fields_out) % 8 == 0, ZK_ERR_ARG, "poseidon tree: indices and fields must be 8-byte aligned");
        poseidon_tree_paths(*t, d_indices, count, d_fields_out, field_stride_words, d_bits_out, bits_stride_bytes);
    });
}

}  // extern "C"
