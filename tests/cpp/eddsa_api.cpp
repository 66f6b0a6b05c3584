// eddsa_api.cpp -- eddsa::challenge / public_key / sign / verify / verify_batch and builder::Circuit::eddsa_verify of the C++ host API
// (include/zksnark.hpp).  Built with g++ and linked against libzkgpu.so by tests/test_cpp_eddsa.py.  "host": the scheme and the gadget
// (no context, runs without a GPU); "gpu": batch verification on the device against the host function.  Prints "ok <name>" per test,
// "value <name> <hex>..." for what the Python test holds against its model, and exits non-zero on the first failed assertion.
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

static FrLocal words(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    FrLocal x;
    x.w = {w0, w1, w2, w3};
    return x;
}
static const FrLocal K1 = words(0x0123456789abcdefull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull, 0x0096a5b4c3d2e1f0ull);

static void print_words(const FrLocal& x) {
    std::printf(" %016llx%016llx%016llx%016llx", (unsigned long long)x.w[3], (unsigned long long)x.w[2], (unsigned long long)x.w[1], (unsigned long long)x.w[0]);
}

static void scheme_on_the_host() {
    const FrLocal digest = eddsa::challenge(babyjub::Point{FrLocal(1), FrLocal(2)}, babyjub::Point{FrLocal(3), FrLocal(4)}, FrLocal(5));
    std::printf("value challenge");
    print_words(digest);
    std::printf("\n");
    const babyjub::Point a = eddsa::public_key(K1);
    ASSERT(a == babyjub::mul(K1.w));
    const eddsa::Signature sig = eddsa::sign(K1, FrLocal(9), FrLocal(1234));
    std::printf("value signature");
    print_words(sig.r8.x); print_words(sig.r8.y); print_words(sig.s);
    std::printf("\n");
    ASSERT(eddsa::verify(a, FrLocal(1234), sig) == eddsa::Status::Valid);
    ASSERT(eddsa::verify(a, FrLocal(1235), sig) == eddsa::Status::Mismatch);
    eddsa::Signature bad = sig;
    bad.s.w = FrLocal::MODULUS;
    ASSERT(eddsa::verify(a, FrLocal(1234), bad) == eddsa::Status::Range);
    bad = sig;
    bad.s = babyjub::params().order;
    ASSERT(eddsa::verify(a, FrLocal(1234), bad) == eddsa::Status::SRange);
    bad = sig;
    bad.r8.y = FrLocal(5);
    ASSERT(eddsa::verify(a, FrLocal(1234), bad) == eddsa::Status::ROffCurve);
    ASSERT(eddsa::verify(bad.r8, FrLocal(1234), sig) == eddsa::Status::KeyOffCurve);
    int refused = 0;
    try { eddsa::sign(FrLocal(0), FrLocal(9), FrLocal(1)); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { eddsa::public_key(babyjub::params().order); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    FrLocal r;
    r.w = FrLocal::MODULUS;
    try { eddsa::sign(K1, FrLocal(9), r); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { eddsa::challenge(a, a, r); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    ASSERT(refused == 4);
    std::printf("ok scheme_on_the_host\n");
}

static void gadget_on_the_host() {
    builder::Circuit b;
    const WireId ax = b.new_wire(), ay = b.new_wire(), rx = b.new_wire(), ry = b.new_wire(), m = b.new_wire();
    std::vector<WireId> s_bits, hm_bits;
    for (int i = 0; i < 251; ++i) s_bits.push_back(b.new_bit());
    for (int i = 0; i < 254; ++i) hm_bits.push_back(b.new_bit());
    bool refused = false;
    try { b.eddsa_verify(ax, ay, rx, ry, m, hm_bits, s_bits); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused && b.gates() == 0);
    b.eddsa_verify(ax, ay, rx, ry, m, s_bits, hm_bits);
    ASSERT(b.gates() == 73384);
    Circuit c = b.finish({});
    const babyjub::Point a = eddsa::public_key(K1);
    const eddsa::Signature sig = eddsa::sign(K1, FrLocal(9), FrLocal(1234));
    const FrLocal hm = eddsa::challenge(sig.r8, a, FrLocal(1234));
    const std::vector<FrLocal> fields{a.x, a.y, sig.r8.x, sig.r8.y, FrLocal(1234)};
    std::vector<FrLocal> in(fields);
    std::vector<uint8_t> packed(64, 0);
    for (int i = 0; i < 505; ++i) {
        const FrLocal& src = i < 251 ? sig.s : hm;
        const int at = i < 251 ? i : i - 251;
        const uint64_t bit = (src.w[at / 64] >> (at % 64)) & 1;
        in.push_back(FrLocal(bit));
        packed[i / 8] |= (uint8_t)(bit << (i % 8));
    }
    const std::vector<FrLocal> w = c.weights(in);
    ASSERT(c.weights_tape(in) == w);
    ASSERT(c.weights_mixed(packed, fields) == w);
    std::printf("ok gadget_on_the_host\n");
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
    const size_t count = 70, stride = 72;
    const babyjub::Point a = eddsa::public_key(K1);
    std::vector<uint64_t> points(20 * count), s(4 * count);
    std::vector<eddsa::Signature> sigs(count);
    std::vector<FrLocal> msgs(count);
    for (size_t j = 0; j < count; ++j) {
        msgs[j] = FrLocal(1000 + j);
        sigs[j] = eddsa::sign(K1, FrLocal(j), msgs[j]);
        if (j % 7 == 3) msgs[j] = FrLocal(5);                              // a wrong message
        if (j % 7 == 5) sigs[j].s = babyjub::params().order;                // S = l
        uint64_t* p = points.data() + 20 * j;
        std::copy(a.x.w.begin(), a.x.w.end(), p);
        std::copy(a.y.w.begin(), a.y.w.end(), p + 4);
        std::copy(sigs[j].r8.x.w.begin(), sigs[j].r8.x.w.end(), p + 8);
        std::copy(sigs[j].r8.y.w.begin(), sigs[j].r8.y.w.end(), p + 12);
        std::copy(msgs[j].w.begin(), msgs[j].w.end(), p + 16);
        std::copy(sigs[j].s.w.begin(), sigs[j].s.w.end(), s.begin() + 4 * j);
    }
    void *d_p = nullptr, *d_s = nullptr, *d_st = nullptr, *d_b = nullptr;
    HIP_OK(hipMalloc(&d_p, points.size() * 8));
    HIP_OK(hipMalloc(&d_s, s.size() * 8));
    HIP_OK(hipMalloc(&d_st, count * 4));
    HIP_OK(hipMalloc(&d_b, count * stride));
    HIP_OK(hipMemcpy(d_p, points.data(), points.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_s, s.data(), s.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_b, 0xA5, count * stride));
    eddsa::verify_batch(ctx, d_p, d_s, count, d_st, d_b, stride);
    std::vector<uint32_t> status(count);
    std::vector<uint8_t> bits(count * stride);
    HIP_OK(hipMemcpy(status.data(), d_st, count * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bits.data(), d_b, count * stride, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < count; ++j) {
        ASSERT((int)status[j] == (int)eddsa::verify(a, msgs[j], sigs[j]));
        ASSERT(status[j] == (j % 7 == 3 ? ZK_EDDSA_MISMATCH : j % 7 == 5 ? ZK_EDDSA_S_RANGE : ZK_EDDSA_VALID));
        const FrLocal hm = eddsa::challenge(sigs[j].r8, a, msgs[j]);
        for (int i = 0; i < 512; ++i) {
            const FrLocal& src = i < 251 ? sigs[j].s : hm;
            const int at = i < 251 ? i : i - 251;
            const unsigned want = i < 505 ? (unsigned)((src.w[at / 64] >> (at % 64)) & 1) : 0u;
            ASSERT(((bits[j * stride + i / 8] >> (i % 8)) & 1u) == want);
        }
        for (size_t i = 64; i < stride; ++i) ASSERT(bits[j * stride + i] == 0xA5);
    }
    bool refused = false;
    try { eddsa::verify_batch(ctx, d_p, d_s, count, d_st, d_b, 60); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused);
    HIP_OK(hipFree(d_p)); HIP_OK(hipFree(d_s)); HIP_OK(hipFree(d_st)); HIP_OK(hipFree(d_b));
    std::printf("ok batch_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    scheme_on_the_host();
    gadget_on_the_host();
    if (mode == "gpu") batch_on_the_device();
    return 0;
}
