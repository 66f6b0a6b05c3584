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
//   k_poseidon_range, k_poseidon_update_check, k_poseidon_update_scatter, k_poseidon_update_level
//                       zk_poseidon_tree_append / _update: every refusal is found before anything is written (range of the new
//                       values, index bound, a duplicate election by atomicOr over a bitmap of the tree's node slots); the new leaves
//                       are scattered to level 0; then one launch per level over a dense list of the level's changed nodes: a node's
//                       parent is hashed once, by its left child's lane or, where that one did not change, its right child's, with
//                       the rounds of k_poseidon, and entered into the next level's list by a wave-aggregated atomicAdd.
//                       An append's dirty nodes are a contiguous range per level and go through k_poseidon itself.
// Per-hash cost for arity 2: 3 (R_F t + R_P) = 243 multiplications in the S-boxes and t^2 (R_F + R_P) = 585 in the mix.
#include <utility>
#include "common.hpp"
#include "poseidon.hpp"

namespace zk {

static constexpr unsigned POSEIDON_BLOCK = 256;
static constexpr unsigned long long POSEIDON_NO_ERROR = ~0ull;
static constexpr unsigned POSEIDON_FLAGS = 3;   // flag[0]: every call; zk_poseidon_tree_update: [0] index, [1] value, [2] duplicate

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

// 4 canonical words behind an 8-byte aligned pointer: below r?
__device__ __forceinline__ bool poseidon_words_in_range(const uint64_t* __restrict__ w) {
    Fr x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t v = w[i];
        x.l[2 * i] = (uint32_t)v;
        x.l[2 * i + 1] = (uint32_t)(v >> 32);
    }
    return x.raw_in_range();
}

// grid: ceil(count / POSEIDON_BLOCK) blocks; the flag records the lowest element >= r.  Writes nothing else.
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon_range(const uint64_t* __restrict__ values, size_t count, unsigned long long* __restrict__ flag) {
    const size_t j = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    if (j >= count) return;
    if (!poseidon_words_in_range(values + 4 * j)) atomicMin(flag, (unsigned long long)j);
}

// The marks are one bit per node SLOT of the tree (bit meta[2 k] + i for node i of level k), cleared by the host at the start of a call.
// grid: ceil(count / POSEIDON_BLOCK) blocks, one lane per instance.  flags[0]: the lowest instance whose index is >= n_leaves;
// flags[1]: the lowest instance whose value is >= r; flags[2]: the lowest LEAF that occurs twice -- every lane sets its leaf's mark and
// a lane that finds it set reports the leaf, so the answer does not depend on which lane came first.  Writes the marks only; after
// an accepted call they are the changed nodes of level 0.
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon_update_check(const uint64_t* __restrict__ indices, const uint64_t* __restrict__ values, size_t count, size_t n_leaves,
                        unsigned* __restrict__ marks, unsigned long long* __restrict__ flags) {
    const size_t j = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t index = indices[j];
    if (index >= n_leaves) {
        atomicMin(flags, (unsigned long long)j);
    } else {
        const unsigned bit = 1u << (index & 31);
        if (atomicOr(marks + (index >> 5), bit) & bit) atomicMin(flags + 2, (unsigned long long)index);
    }
    if (!poseidon_words_in_range(values + 4 * j)) atomicMin(flags + 1, (unsigned long long)j);
}

// grid as above.  The call was accepted -- every index is below n_leaves and occurs once: stores value j at leaf indices[j] and
// writes the leaf into list[j], the changed nodes of level 0.
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon_update_scatter(const uint64_t* __restrict__ indices, const uint64_t* __restrict__ values, size_t count, size_t n_leaves,
                          uint64_t* __restrict__ leaves, unsigned* __restrict__ list) {
    const size_t j = (size_t)blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    if (j >= count) return;
    const uint64_t index = indices[j];
    if (index >= n_leaves) return;
    list[j] = (unsigned)index;   // n_leaves <= 2^32
#pragma unroll
    for (int w = 0; w < 4; ++w) leaves[4 * index + w] = values[4 * j + w];
}

// One level of an update, k -> k + 1.  list[0 .. *len) holds the changed nodes of level k, each once and in no order, and their marks
// are set.  The grid is sized by the call's count, ceil(count / POSEIDON_BLOCK) blocks, and lanes past *len leave at once.  Lane j
// takes node i = list[j]; its parent p = i >> 1 belongs to the left child, or to the right one where the left one's mark is clear,
// so every changed parent has one lane and no election is needed.  That lane sets p's mark, enters p into list_next -- one atomicAdd
// on *len_next per wave, the lanes' places by their rank in the wave's ballot -- and hashes the two children (`fill` = z_k where the
// right one is not stored) with the rounds of k_poseidon.  The other lanes leave before the rounds.
// below: the stored nodes of level k, size_below of them; above: level k + 1; mark_below, mark_above: the first mark of each level.
__global__ void __launch_bounds__(POSEIDON_BLOCK)
k_poseidon_update_level(const Fr* __restrict__ par, unsigned rp, const unsigned* __restrict__ list, const unsigned* __restrict__ len,
                        unsigned* __restrict__ list_next, unsigned* __restrict__ len_next, const uint64_t* __restrict__ below,
                        size_t size_below, Fr fill, uint64_t* __restrict__ above, size_t mark_below, size_t mark_above, unsigned* marks,
                        unsigned long long* __restrict__ flag) {
    constexpr unsigned T = 3;
    const unsigned j = blockIdx.x * POSEIDON_BLOCK + threadIdx.x;
    if (j >= *len) return;
    const unsigned i = list[j];
    const unsigned p = i >> 1;   // one register across the rounds
    bool mine = true;
    if (i & 1) {
        const size_t left = mark_below + (i ^ 1);
        mine = !((marks[left >> 5] >> (left & 31)) & 1);
    }
    const unsigned long long owners = __ballot(mine);
    if (!mine) return;
    {
        const size_t mark = mark_above + p;
        atomicOr(marks + (mark >> 5), 1u << (mark & 31));
        const unsigned lane = threadIdx.x & 63, leader = (unsigned)__ffsll((long long)owners) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(len_next, (unsigned)__popcll(owners));
        base = __shfl(base, leader);
        list_next[base + __popcll(owners & ((1ull << lane) - 1))] = p;
    }
    Fr s[T];
    s[0] = Fr::zero();
    s[1] = poseidon_load(below, 2 * (size_t)p, size_below, fill, flag, 2 * (size_t)p);   // stored nodes are canonical: the flag stays as it is
    s[2] = poseidon_load(below, 2 * (size_t)p + 1, size_below, fill, flag, 2 * (size_t)p + 1);
    const Fr* __restrict__ c = par;
    const Fr* __restrict__ m = par + (size_t)(POSEIDON_RF + rp) * T;
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += T) poseidon_full_round<T>(s, c, m);
#pragma unroll 1
    for (unsigned r = 0; r < rp; ++r, c += T) poseidon_partial_round<T>(s, c, m);
#pragma unroll 1
    for (unsigned r = 0; r < POSEIDON_RF / 2; ++r, c += T) poseidon_full_round<T>(s, c, m);
    const Fr d = s[0].to_canonical();
    uint4* dst = reinterpret_cast<uint4*>(above + 4 * (size_t)p);
    dst[0] = make_uint4(d.l[0], d.l[1], d.l[2], d.l[3]);
    dst[1] = make_uint4(d.l[4], d.l[5], d.l[6], d.l[7]);
}

static PoseidonState& poseidon_state(zk_ctx* ctx, size_t arity, const PoseidonParams& p) {
    if (!ctx->poseidon) ctx->poseidon = std::make_shared<PoseidonState>();
    PoseidonState& st = *ctx->poseidon;
    if (!st.flag.p) st.flag.alloc(POSEIDON_FLAGS);
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
    if (!ctx->poseidon->flag.p) ctx->poseidon->flag.alloc(POSEIDON_FLAGS);
    static const unsigned long long none[POSEIDON_FLAGS] = {POSEIDON_NO_ERROR, POSEIDON_NO_ERROR, POSEIDON_NO_ERROR};
    ZK_HIP(hipMemcpyAsync(ctx->poseidon->flag.p, none, sizeof(none), hipMemcpyHostToDevice, ctx->stream));
}
// waits for the stream; the lowest index an earlier launch recorded, or POSEIDON_NO_ERROR
static unsigned long long poseidon_flag_read(zk_ctx* ctx) {
    unsigned long long bad = POSEIDON_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(&bad, ctx->poseidon->flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
    return bad;
}
// the same for all the flags of zk_poseidon_tree_update
static void poseidon_flags_read(zk_ctx* ctx, unsigned long long (&bad)[POSEIDON_FLAGS]) {
    ZK_HIP(hipMemcpyAsync(bad, ctx->poseidon->flag.p, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->resolve_profile();
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
    size_t capacity = 0;               // the leaves the node buffer has room for: the levels are laid out as those of `capacity` leaves
    std::vector<uint64_t> meta;        // per level: offset into nodes (in nodes, by capacity), stored size (by n_leaves)
    zk::DevBuf<uint64_t> nodes;        // every level, canonical, 4 words per node
    zk::DevBuf<uint64_t> d_meta, zeros;
    zk::DevBuf<unsigned> marks;        // zk_poseidon_tree_update: one bit per node slot, allocated on first use, cleared per call
    zk::DevBuf<unsigned> lists;        // zk_poseidon_tree_update: the changed nodes of a level, twice, and the lists' lengths
    std::vector<zk::Fr> z;             // z_0 .. z_depth, Montgomery form
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
    t->n_leaves = t->capacity = n_leaves;
    t->depth = depth;
    size_t total = 0;
    for (unsigned k = 0; k <= depth; ++k) {
        t->meta.push_back(total);
        t->meta.push_back(poseidon_level_size(n_leaves, k));
        total += t->meta.back();
    }
    t->z = poseidon_zero_hashes(depth);
    const std::vector<Fr>& z = t->z;
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

// the stored sizes of `n_leaves` leaves into meta, the meta to the device, the root to the host; complete on return
static void poseidon_tree_publish(zk_poseidon_tree& t, size_t n_leaves) {
    hipStream_t st = t.ctx->stream;
    if (n_leaves != t.n_leaves) {
        t.n_leaves = n_leaves;
        for (unsigned k = 0; k <= t.depth; ++k) t.meta[2 * k + 1] = poseidon_level_size(n_leaves, k);
        ZK_HIP(hipMemcpyAsync(t.d_meta.p, t.meta.data(), t.meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    if (t.meta[2 * t.depth + 1]) ZK_HIP(hipMemcpyAsync(t.root, t.nodes.p + 4 * t.meta[2 * t.depth], 32, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    t.ctx->resolve_profile();
}

// Room for `capacity` leaves: a new buffer laid out by `capacity`, every stored level copied device to device.  The stored sizes, the
// nodes and the root stay as they are, so nothing a caller can observe changes.
static void poseidon_tree_grow(zk_poseidon_tree& t, size_t capacity) {
    hipStream_t st = t.ctx->stream;
    std::vector<uint64_t> meta(t.meta);
    size_t total = 0;
    for (unsigned k = 0; k <= t.depth; ++k) {
        meta[2 * k] = total;
        total += poseidon_level_size(capacity, k);
    }
    DevBuf<uint64_t> nodes(4 * total);
    for (unsigned k = 0; k <= t.depth; ++k)
        if (meta[2 * k + 1])
            ZK_HIP(hipMemcpyAsync(nodes.p + 4 * meta[2 * k], t.nodes.p + 4 * t.meta[2 * k], meta[2 * k + 1] * 32, hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipMemcpyAsync(t.d_meta.p, meta.data(), meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));   // the old buffer goes away
    t.nodes = std::move(nodes);
    t.meta = std::move(meta);
    t.capacity = capacity;
}

static void poseidon_tree_append(zk_poseidon_tree& t, const void* d_leaves, size_t count) {
    zk_ctx* ctx = t.ctx;
    const size_t n_old = t.n_leaves, full = (size_t)1 << t.depth;
    ZK_REQUIRE(count <= full - n_old, ZK_ERR_ARG,
               "poseidon tree: " + std::to_string(n_old) + " + " + std::to_string(count) + " leaves do not fit a tree of depth " + std::to_string(t.depth));
    const size_t n_new = n_old + count;
    poseidon_flag_reset(ctx);
    {
        ProfScope ps(ctx, "poseidon_range", (double)count * 32.0);
        hipLaunchKernelGGL(k_poseidon_range, dim3(ceil_div(count, POSEIDON_BLOCK)), dim3(POSEIDON_BLOCK), 0, ctx->stream, (const uint64_t*)d_leaves, count,
                           ctx->poseidon->flag.p);
    }
    ZK_HIP(hipGetLastError());
    const unsigned long long bad = poseidon_flag_read(ctx);
    ZK_REQUIRE(bad == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon tree: the new leaf at position " + std::to_string(bad) + " is >= r");
    // nothing was written so far; from here on only a HIP error ends the call early
    if (n_new > t.capacity) poseidon_tree_grow(t, std::min(full, std::max(n_new, 2 * t.capacity)));
    ZK_HIP(hipMemcpyAsync(t.nodes.p + 4 * n_old, d_leaves, count * 32, hipMemcpyDeviceToDevice, ctx->stream));
    // the nodes with a new leaf under them are parents n_old >> (k + 1) .. (n_new - 1) >> (k + 1) of level k + 1: k_poseidon over the
    // pairs of level k from the first of them on, the level's NEW size behind the launch's start as `avail`
    for (unsigned k = 0; k < t.depth; ++k) {
        const size_t first = n_old >> (k + 1), last = (n_new - 1) >> (k + 1);
        poseidon_launch(ctx, 2, t.nodes.p + 4 * (t.meta[2 * k] + 2 * first), poseidon_level_size(n_new, k) - 2 * first, last - first + 1, t.z[k],
                        t.nodes.p + 4 * (t.meta[2 * k + 2] + first), 1);
    }
    poseidon_tree_publish(t, n_new);
}

static void poseidon_tree_update(zk_poseidon_tree& t, const void* d_indices, const void* d_values, size_t count) {
    zk_ctx* ctx = t.ctx;
    hipStream_t st = ctx->stream;
    ZK_REQUIRE(count <= ((size_t)1 << 31), ZK_ERR_SIZE, "poseidon tree: too many leaves for one update");
    const PoseidonParams& p = *poseidon_params(2);
    PoseidonState& state = poseidon_state(ctx, 2, p);
    const size_t slots = t.meta[2 * t.depth] + 1, mark_words = (slots + 31) / 32;
    t.marks.ensure(mark_words);
    ZK_HIP(hipMemsetAsync(t.marks.p, 0, mark_words * sizeof(unsigned), st));
    // two lists of changed nodes, read and written in turn, and behind them the length of the list of every level
    t.lists.ensure(2 * count + t.depth + 1);
    unsigned *list[2] = {t.lists.p, t.lists.p + count}, *len = t.lists.p + 2 * count;
    std::vector<unsigned> lens((size_t)t.depth + 1, 0);   // alive until the flags are read
    lens[0] = (unsigned)count;
    ZK_HIP(hipMemcpyAsync(len, lens.data(), lens.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    const uint64_t *indices = (const uint64_t*)d_indices, *values = (const uint64_t*)d_values;
    const dim3 grid(ceil_div(count, POSEIDON_BLOCK)), block(POSEIDON_BLOCK);
    poseidon_flag_reset(ctx);
    {
        ProfScope ps(ctx, "poseidon_update_check", (double)count * 40.0);
        hipLaunchKernelGGL(k_poseidon_update_check, grid, block, 0, st, indices, values, count, t.n_leaves, t.marks.p, state.flag.p);
    }
    ZK_HIP(hipGetLastError());
    unsigned long long bad[POSEIDON_FLAGS];
    poseidon_flags_read(ctx, bad);
    ZK_REQUIRE(bad[0] == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon tree: the index of instance " + std::to_string(bad[0]) + " is not below n_leaves");
    ZK_REQUIRE(bad[1] == POSEIDON_NO_ERROR, ZK_ERR_RANGE, "poseidon tree: the value of instance " + std::to_string(bad[1]) + " is >= r");
    ZK_REQUIRE(bad[2] == POSEIDON_NO_ERROR, ZK_ERR_ARG, "poseidon tree: leaf " + std::to_string(bad[2]) + " occurs more than once in the update");
    // nothing but the marks and the lengths was written so far; from here on only a HIP error ends the call early
    {
        ProfScope ps(ctx, "poseidon_update_scatter", (double)count * 72.0);
        hipLaunchKernelGGL(k_poseidon_update_scatter, grid, block, 0, st, indices, values, count, t.n_leaves, t.nodes.p, list[0]);
    }
    ZK_HIP(hipGetLastError());
    for (unsigned k = 0; k < t.depth; ++k) {   // same stream: a level starts when the one below is complete
        ProfScope ps(ctx, "poseidon_update_level", (double)count * 96.0);
        hipLaunchKernelGGL(k_poseidon_update_level, grid, block, 0, st, state.par[2].p, p.rp, list[k & 1], len + k, list[~k & 1], len + k + 1,
                           t.nodes.p + 4 * t.meta[2 * k], (size_t)t.meta[2 * k + 1], t.z[k], t.nodes.p + 4 * t.meta[2 * k + 2], (size_t)t.meta[2 * k],
                           (size_t)t.meta[2 * k + 2], t.marks.p, state.flag.p);
        ZK_HIP(hipGetLastError());
    }
    poseidon_tree_publish(t, t.n_leaves);
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
int zk_poseidon_tree_update(zk_poseidon_tree* t, const void* d_indices, const void* d_values, size_t count) {
    if (!t) return ZK_ERR_ARG;
    return guarded(t->ctx, [&] {
        if (count == 0) return;
        ZK_REQUIRE(d_indices && d_values, ZK_ERR_ARG, "poseidon tree: null device pointer");
        ZK_REQUIRE(((uintptr_t)d_indices | (uintptr_t)d_values) % 8 == 0, ZK_ERR_ARG, "poseidon tree: indices and values must be 8-byte aligned");
        poseidon_tree_update(*t, d_indices, d_values, count);
    });
}
int zk_poseidon_tree_append(zk_poseidon_tree* t, const void* d_leaves, size_t count) {
    if (!t) return ZK_ERR_ARG;
    return guarded(t->ctx, [&] {
        if (count == 0) return;
        ZK_REQUIRE(d_leaves, ZK_ERR_ARG, "poseidon tree: null device pointer");
        ZK_REQUIRE((uintptr_t)d_leaves % 8 == 0, ZK_ERR_ARG, "poseidon tree: the leaves must be 8-byte aligned");
        poseidon_tree_append(*t, d_leaves, count);
    });
}

}  // extern "C"
