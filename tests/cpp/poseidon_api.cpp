// poseidon_api.cpp -- poseidon::hash / zero_hashes / hash_batch, PoseidonTree and builder::Circuit::poseidon / merkle_root of the C++
// host API (include/zksnark.hpp).  Built with g++ and linked against libzkgpu.so by tests/test_cpp_poseidon.py.  "host": the hash and
// the gadgets (no context, runs without a GPU); "gpu": batch hashing, a tree, its paths and the membership circuit's witnesses on the
// device.  Prints "ok <name>" per test and exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using builder::WireId;

#define ASSERT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static FrLocal from_words(uint64_t w3, uint64_t w2, uint64_t w1, uint64_t w0) {
    FrLocal x;
    x.w = {w0, w1, w2, w3};
    return x;
}
static FrLocal r_minus(uint64_t k) {
    FrLocal x;
    x.w = FrLocal::MODULUS;
    x.w[0] -= k;
    return x;
}

// circomlib's published digests
static const FrLocal H12 = from_words(0x115cc0f5e7d69041ull, 0x3df64c6b9662e9cfull, 0x2a3617f274324551ull, 0x9e19607a4417189aull);
static const FrLocal H1234 = from_words(0x299c867db6c1fdd7ull, 0x9dcefa40e4510b98ull, 0x37e60ebb1ce0663dull, 0xbaa525df65250465ull);
static const FrLocal Z1 = from_words(0x2098f5fb9e239eabull, 0x3ceac3f27b81e481ull, 0xdc3124d55ffed523ull, 0xa839ee8446b64864ull);
static const FrLocal ROOT_123_D2 = from_words(0x0d9e989a60f1961eull, 0x8fda683cfc358560ull, 0x8a47d513f9af9167ull, 0xc1287fa8cea0720eull);

static void hash_and_refusals() {
    ASSERT(poseidon::hash({FrLocal(1), FrLocal(2)}) == H12);
    ASSERT(poseidon::hash({FrLocal(1), FrLocal(2), FrLocal(3), FrLocal(4)}) == H1234);
    const auto z = poseidon::zero_hashes(2);
    ASSERT(z.size() == 3 && z[0] == FrLocal(0) && z[1] == Z1 && z[2] == poseidon::hash({Z1, Z1}));
    int refused = 0;
    try { poseidon::hash({FrLocal(1), FrLocal(2), FrLocal(3)}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    try { poseidon::hash({}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    try { poseidon::hash({FrLocal(1), r_minus(0)}); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    ASSERT(refused == 3);
    std::printf("ok hash_and_refusals\n");
}

struct Membership {
    Circuit c;
    size_t depth;
};
// public: the root; private: leaf, siblings (field wires), directions (bit wires), created in that order
static Membership membership(size_t depth) {
    builder::Circuit b;
    const WireId leaf = b.new_wire();
    std::vector<WireId> sibs, dirs;
    for (size_t k = 0; k < depth; ++k) sibs.push_back(b.new_wire());
    for (size_t k = 0; k < depth; ++k) dirs.push_back(b.new_bit());
    const WireId root = b.merkle_root(leaf, sibs, dirs);
    ASSERT(b.gates() == 246 * depth);
    return {b.finish({root}), depth};
}

static void gadgets_on_the_host() {
    {
        builder::Circuit b;
        const std::vector<WireId> in{b.new_wire(), b.new_wire()};
        const WireId h = b.poseidon(in);
        ASSERT(b.gates() == 244);
        const WireId h4 = b.poseidon(std::vector<WireId>{h, in[0], b.unity_wire(), b.zero_wire()});
        ASSERT(b.gates() == 244 + 301);
        bool refused = false;
        try { b.poseidon(std::vector<WireId>{in[0], in[1], h}); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
        ASSERT(refused && b.gates() == 244 + 301);
        Circuit c = b.finish({h, h4});
        const std::vector<FrLocal> w = c.weights({FrLocal(1), FrLocal(2)});
        ASSERT(w[1] == H12 && w[2] == poseidon::hash({H12, FrLocal(1), FrLocal(1), FrLocal(0)}));
        ASSERT(c.weights_tape({FrLocal(1), FrLocal(2)}) == w && c.weights_mixed({}, {FrLocal(1), FrLocal(2)}) == w);
    }
    Membership m = membership(2);
    const auto d = m.c.mixed_dims();
    ASSERT(d.n_bit_inputs == 2 && d.n_field_inputs == 3 && d.core_ops == 0 && !m.c.is_boolean());
    // leaves (1, 2, 3), depth 2: the path of leaf 2 is sibling z_0 = 0 at level 0 (leaf 3 does not exist), hash(1, 2) at level 1
    const std::vector<FrLocal> in{FrLocal(3), FrLocal(0), H12, FrLocal(0), FrLocal(1)};
    const auto w = m.c.weights(in);
    ASSERT(w[1] == ROOT_123_D2);
    ASSERT(m.c.weights_mixed({0x02}, {FrLocal(3), FrLocal(0), H12}) == w);
    std::printf("ok gadgets_on_the_host\n");
}

// the HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void tree_paths_and_witnesses_on_the_device() {
    Context ctx;
    const size_t n = 5, depth = 3, count = 5;
    std::vector<FrLocal> leaves;
    for (size_t i = 0; i < n; ++i) leaves.push_back(FrLocal(100 + i));
    void *d_leaves = nullptr, *d_hash = nullptr, *d_idx = nullptr, *d_f = nullptr, *d_b = nullptr, *d_w = nullptr;
    HIP_OK(hipMalloc(&d_leaves, n * 32));
    HIP_OK(hipMalloc(&d_hash, 2 * 32));
    HIP_OK(hipMemcpy(d_leaves, leaves[0].w.data(), n * 32, hipMemcpyHostToDevice));
    poseidon::hash_batch(ctx, d_leaves, 2, 2, d_hash);
    std::vector<FrLocal> pairs(2);
    HIP_OK(hipMemcpy(pairs[0].w.data(), d_hash, 2 * 32, hipMemcpyDeviceToHost));
    ASSERT(pairs[0] == poseidon::hash({leaves[0], leaves[1]}) && pairs[1] == poseidon::hash({leaves[2], leaves[3]}));

    PoseidonTree tree(ctx, d_leaves, n, depth);
    ASSERT(tree.n_leaves() == n && tree.depth() == depth);
    const auto z = poseidon::zero_hashes(depth);
    const auto l1 = tree.nodes(1), l2 = tree.nodes(2), l3 = tree.nodes(3);
    ASSERT(l1.size() == 3 && l2.size() == 2 && l3.size() == 1 && tree.nodes(0) == leaves);
    ASSERT(l1[0] == pairs[0] && l1[1] == pairs[1] && l1[2] == poseidon::hash({leaves[4], z[0]}));
    ASSERT(l2[0] == poseidon::hash({l1[0], l1[1]}) && l2[1] == poseidon::hash({l1[2], z[1]}));
    ASSERT(l3[0] == poseidon::hash({l2[0], l2[1]}) && tree.root() == l3[0]);

    Membership m = membership(depth);
    const size_t wires = m.c.wires();
    const uint64_t idx[count] = {0, 1, 2, 3, 4};
    HIP_OK(hipMalloc(&d_idx, sizeof(idx)));
    HIP_OK(hipMalloc(&d_f, count * (depth + 1) * 32));
    HIP_OK(hipMalloc(&d_b, count));
    HIP_OK(hipMalloc(&d_w, count * wires * 32));
    HIP_OK(hipMemcpy(d_idx, idx, sizeof(idx), hipMemcpyHostToDevice));
    tree.paths(d_idx, count, d_f, (depth + 1) * 4, d_b, 1);
    Mixgen mg(ctx, m.c);
    mg.run(d_b, 1, d_f, count, d_w, wires);                 // device to device: no host step between
    uint8_t bits[count];
    HIP_OK(hipMemcpy(bits, d_b, count, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < count; ++j) {
        FrLocal root;
        HIP_OK(hipMemcpy(root.w.data(), (const char*)d_w + (j * wires + 1) * 32, 32, hipMemcpyDeviceToHost));
        ASSERT(root == tree.root() && bits[j] == idx[j]);
    }
    bool refused = false;
    const uint64_t bad[2] = {4, 5};
    HIP_OK(hipMemcpy(d_idx, bad, sizeof(bad), hipMemcpyHostToDevice));
    try { tree.paths(d_idx, 2, d_f, (depth + 1) * 4, d_b, 1); } catch (const Error& e) { refused = e.status == ZK_ERR_RANGE && std::string(e.what()).find("instance 1") != std::string::npos; }
    ASSERT(refused);
    refused = false;
    try { tree.paths(d_idx, 1, d_f, depth * 4, d_b, 1); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused);
    HIP_OK(hipFree(d_leaves)); HIP_OK(hipFree(d_hash)); HIP_OK(hipFree(d_idx)); HIP_OK(hipFree(d_f)); HIP_OK(hipFree(d_b)); HIP_OK(hipFree(d_w));
    std::printf("ok tree_paths_and_witnesses_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    hash_and_refusals();
    gadgets_on_the_host();
    if (mode == "gpu") tree_paths_and_witnesses_on_the_device();
    return 0;
}
