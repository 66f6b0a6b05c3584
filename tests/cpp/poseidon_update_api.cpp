// poseidon_update_api.cpp -- PoseidonTree::update and PoseidonTree::append of the C++ host API (include/zksnark.hpp).  Built with g++
// and linked against libzkgpu.so by tests/test_cpp_poseidon_update.py.  "host": the program links and the two calls are members of
// the class (runs without a GPU); "gpu": one update and one append, compared with a tree built over the final leaves.  Prints
// "ok <name>" per test and exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;

#define ASSERT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void api_links() {
    void (PoseidonTree::*update)(const void*, const void*, size_t) = &PoseidonTree::update;
    void (PoseidonTree::*append)(const void*, size_t) = &PoseidonTree::append;
    int (*c_update)(zk_poseidon_tree*, const void*, const void*, size_t) = &zk_poseidon_tree_update;
    int (*c_append)(zk_poseidon_tree*, const void*, size_t) = &zk_poseidon_tree_append;
    ASSERT(update && append && c_update && c_append);
    ASSERT(zk_poseidon_tree_update(nullptr, nullptr, nullptr, 0) == ZK_ERR_ARG && zk_poseidon_tree_append(nullptr, nullptr, 0) == ZK_ERR_ARG);
    std::printf("ok api_links\n");
}

// the HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void same_tree(const PoseidonTree& a, const PoseidonTree& b) {
    ASSERT(a.n_leaves() == b.n_leaves() && a.depth() == b.depth() && a.root() == b.root());
    for (unsigned k = 0; k <= a.depth(); ++k) ASSERT(a.nodes(k) == b.nodes(k));
}

static void update_and_append_on_the_device() {
    Context ctx;
    const size_t n = 5, extra = 4, depth = 4;
    std::vector<FrLocal> leaves;
    for (size_t i = 0; i < n + extra; ++i) leaves.push_back(FrLocal(100 + i));
    void *d_leaves = nullptr, *d_idx = nullptr, *d_val = nullptr;
    HIP_OK(hipMalloc(&d_leaves, (n + extra) * 32));
    HIP_OK(hipMalloc(&d_idx, 3 * sizeof(uint64_t)));
    HIP_OK(hipMalloc(&d_val, 3 * 32));
    HIP_OK(hipMemcpy(d_leaves, leaves[0].w.data(), (n + extra) * 32, hipMemcpyHostToDevice));
    PoseidonTree tree(ctx, d_leaves, n, depth);

    const uint64_t idx[3] = {4, 0, 1};                      // the last leaf (its sibling is z_0) and both children of one parent
    const std::vector<FrLocal> val{FrLocal(7), FrLocal(0), FrLocal(9)};
    HIP_OK(hipMemcpy(d_idx, idx, sizeof(idx), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_val, val[0].w.data(), 3 * 32, hipMemcpyHostToDevice));
    const FrLocal before = tree.root();
    tree.update(d_idx, d_val, 3);
    ASSERT(!(tree.root() == before));
    for (size_t j = 0; j < 3; ++j) leaves[idx[j]] = val[j];
    HIP_OK(hipMemcpy(d_leaves, leaves[0].w.data(), (n + extra) * 32, hipMemcpyHostToDevice));
    {
        PoseidonTree want(ctx, d_leaves, n, depth);
        same_tree(tree, want);
    }
    tree.append((const char*)d_leaves + n * 32, extra);
    ASSERT(tree.n_leaves() == n + extra);
    {
        PoseidonTree want(ctx, d_leaves, n + extra, depth);
        same_tree(tree, want);
    }

    // refusals: the tree stays as it was
    const FrLocal root = tree.root();
    int refused = 0;
    const uint64_t twice[2] = {3, 3}, far[2] = {1, n + extra};
    HIP_OK(hipMemcpy(d_idx, twice, sizeof(twice), hipMemcpyHostToDevice));
    try { tree.update(d_idx, d_val, 2); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG && std::string(e.what()).find("leaf 3") != std::string::npos; }
    HIP_OK(hipMemcpy(d_idx, far, sizeof(far), hipMemcpyHostToDevice));
    try { tree.update(d_idx, d_val, 2); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE && std::string(e.what()).find("instance 1") != std::string::npos; }
    try { tree.append(d_leaves, 8); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    ASSERT(refused == 3 && tree.root() == root && tree.n_leaves() == n + extra);
    HIP_OK(hipFree(d_leaves)); HIP_OK(hipFree(d_idx)); HIP_OK(hipFree(d_val));
    std::printf("ok update_and_append_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    api_links();
    if (mode == "gpu") update_and_append_on_the_device();
    return 0;
}
