// babyjub_api.cpp -- babyjub::params / on_curve / add / mul / mul_batch and builder::Circuit::babyjub_* of the C++ host API
// (include/zksnark.hpp).  Built with g++ and linked against libzkgpu.so by tests/test_cpp_babyjub.py.  "host": the host arithmetic and
// the gadgets (no context, runs without a GPU); "gpu": batch multiplication on the device, fixed and variable base, against the host
// function.  Prints "ok <name>" per test, "value <name> <x> <y>" for what the Python test holds against its model, and exits non-zero
// on the first failed assertion.
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

static const std::array<uint64_t, 4> K1 = {0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, 0x8796a5b4c3d2e1f0ull};

static void print_point(const char* name, const babyjub::Point& p) {
    std::printf("value %s %016llx%016llx%016llx%016llx %016llx%016llx%016llx%016llx\n", name, (unsigned long long)p.x.w[3], (unsigned long long)p.x.w[2],
                (unsigned long long)p.x.w[1], (unsigned long long)p.x.w[0], (unsigned long long)p.y.w[3], (unsigned long long)p.y.w[2],
                (unsigned long long)p.y.w[1], (unsigned long long)p.y.w[0]);
}
static babyjub::Point identity() { return babyjub::Point{FrLocal(0), FrLocal(1)}; }

static void host_arithmetic_and_refusals() {
    const babyjub::Params p = babyjub::params();
    ASSERT(p.a == FrLocal(168700) && p.d == FrLocal(168696));
    ASSERT(babyjub::on_curve(p.base8) && babyjub::on_curve(p.generator) && babyjub::on_curve(identity()));
    ASSERT(babyjub::mul(p.order.w) == identity());
    ASSERT(babyjub::mul({8, 0, 0, 0}, &p.generator) == p.base8);
    ASSERT(!(babyjub::mul(p.order.w, &p.generator) == identity()));
    ASSERT(babyjub::add(p.base8, identity()) == p.base8 && babyjub::add(p.base8, p.base8) == babyjub::mul({2, 0, 0, 0}));
    print_point("k1_base8", babyjub::mul(K1));
    print_point("k1_generator", babyjub::mul(K1, &p.generator));
    print_point("sum", babyjub::add(p.base8, p.generator));
    babyjub::Point off = p.base8, big = p.base8;
    off.y = FrLocal(5);
    big.x.w = FrLocal::MODULUS;
    ASSERT(!babyjub::on_curve(off));
    int refused = 0;
    try { babyjub::add(off, p.base8); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { babyjub::mul(K1, &off); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { babyjub::on_curve(big); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { babyjub::add(p.base8, big); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    ASSERT(refused == 4);
    std::printf("ok host_arithmetic_and_refusals\n");
}

static void gadgets_on_the_host() {
    const babyjub::Params prm = babyjub::params();
    builder::Circuit b;
    const WireId px = b.new_wire(), py = b.new_wire(), ax = b.new_wire(), ay = b.new_wire(), sx = b.new_wire(), sy = b.new_wire();
    std::vector<WireId> bits;
    for (int i = 0; i < 6; ++i) bits.push_back(b.new_bit());
    const builder::Circuit::Point fixed = b.babyjub_mul_fixed(bits);
    ASSERT(b.gates() == 24);
    b.babyjub_affine(fixed, ax, ay);
    const builder::Circuit::Point var = b.babyjub_mul(px, py, bits);
    ASSERT(b.gates() == 24 + 4 + 107);
    const builder::Circuit::Point sum = b.babyjub_add(var, fixed);
    b.babyjub_affine(sum, sx, sy);
    b.babyjub_assert_on_curve(sx, sy);
    ASSERT(b.gates() == 24 + 4 + 107 + 11 + 4 + 4);
    bool refused = false;
    try { b.babyjub_mul_fixed(std::vector<WireId>{}); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused && b.gates() == 154);
    Circuit c = b.finish({ax, ay, sx, sy});
    const uint64_t k = 0x2d;
    const babyjub::Point a = babyjub::mul({k, 0, 0, 0}), v = babyjub::mul({k, 0, 0, 0}, &prm.generator), s = babyjub::add(a, v);
    std::vector<FrLocal> in{prm.generator.x, prm.generator.y, a.x, a.y, s.x, s.y};
    for (int i = 0; i < 6; ++i) in.push_back(FrLocal((k >> i) & 1));
    const std::vector<FrLocal> w = c.weights(in);
    ASSERT(w[1] == a.x && w[2] == a.y && w[3] == s.x && w[4] == s.y);
    ASSERT(c.weights_tape(in) == w);
    ASSERT(c.weights_mixed({(uint8_t)k}, {prm.generator.x, prm.generator.y, a.x, a.y, s.x, s.y}) == w);
    std::printf("ok gadgets_on_the_host\n");
}

// the HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
int hipMemset(void* dst, int value, size_t size);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void batch_on_the_device() {
    Context ctx;
    const babyjub::Params prm = babyjub::params();
    const size_t count = 70, stride = 12;
    std::vector<uint64_t> scalars(4 * count), points(8 * count), out(stride * count);
    std::vector<babyjub::Point> pts(count);
    for (size_t j = 0; j < count; ++j) {
        for (int i = 0; i < 4; ++i) scalars[4 * j + i] = K1[i] * (2 * j + 1) + (j << (7 * i));
        pts[j] = babyjub::mul({j + 1, 0, 0, 0}, &prm.generator);
        std::copy(pts[j].x.w.begin(), pts[j].x.w.end(), points.begin() + 8 * j);
        std::copy(pts[j].y.w.begin(), pts[j].y.w.end(), points.begin() + 8 * j + 4);
    }
    void *d_s = nullptr, *d_p = nullptr, *d_o = nullptr;
    HIP_OK(hipMalloc(&d_s, scalars.size() * 8));
    HIP_OK(hipMalloc(&d_p, points.size() * 8));
    HIP_OK(hipMalloc(&d_o, out.size() * 8));
    HIP_OK(hipMemcpy(d_s, scalars.data(), scalars.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_p, points.data(), points.size() * 8, hipMemcpyHostToDevice));
    for (int variable = 0; variable < 2; ++variable) {
        HIP_OK(hipMemset(d_o, 0xA5, out.size() * 8));
        babyjub::mul_batch(ctx, d_s, variable ? d_p : nullptr, count, d_o, stride);
        HIP_OK(hipMemcpy(out.data(), d_o, out.size() * 8, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < count; ++j) {
            const std::array<uint64_t, 4> k = {scalars[4 * j], scalars[4 * j + 1], scalars[4 * j + 2], scalars[4 * j + 3]};
            const babyjub::Point want = babyjub::mul(k, variable ? &pts[j] : nullptr);
            ASSERT(std::equal(want.x.w.begin(), want.x.w.end(), out.begin() + stride * j));
            ASSERT(std::equal(want.y.w.begin(), want.y.w.end(), out.begin() + stride * j + 4));
            for (size_t i = 8; i < stride; ++i) ASSERT(out[stride * j + i] == 0xA5A5A5A5A5A5A5A5ull);
        }
    }
    points[8 * 3 + 4] ^= 1;                                 // instance 3 leaves the curve
    HIP_OK(hipMemcpy(d_p, points.data(), points.size() * 8, hipMemcpyHostToDevice));
    bool refused = false;
    try { babyjub::mul_batch(ctx, d_s, d_p, count, d_o, stride); } catch (const Error& e) { refused = e.status == ZK_ERR_RANGE && std::string(e.what()).find("instance 3") != std::string::npos; }
    ASSERT(refused);
    HIP_OK(hipFree(d_s)); HIP_OK(hipFree(d_p)); HIP_OK(hipFree(d_o));
    std::printf("ok batch_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    host_arithmetic_and_refusals();
    gadgets_on_the_host();
    if (mode == "gpu") batch_on_the_device();
    return 0;
}
