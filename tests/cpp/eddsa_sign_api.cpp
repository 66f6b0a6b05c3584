// eddsa_sign_api.cpp -- eddsa::sign_batch of the C++ host API (include/zksnark.hpp).  Built with g++ and linked against libzkgpu.so by
// tests/test_cpp_eddsa_sign.py.  "host": nothing but the link and one host signature (runs without a GPU); "gpu": 65 instances signed
// on the device, verified by eddsa::verify_batch, instance 0 held against eddsa::sign, and a refusal.  Prints "ok <name>" per test and
// exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "zksnark.hpp"

using namespace zksnark;

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

static void links_on_the_host() {
    void (*fn)(const Context&, const void*, const void*, const void*, size_t, void*, void*, void*, size_t) = &eddsa::sign_batch;
    ASSERT(fn != nullptr);
    const eddsa::Signature sig = eddsa::sign(K1, FrLocal(9), FrLocal(1234));
    ASSERT(eddsa::verify(eddsa::public_key(K1), FrLocal(1234), sig) == eddsa::Status::Valid);
    std::printf("ok links_on_the_host\n");
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
    const size_t count = 65, stride = 72;
    std::vector<uint64_t> keys(4 * count), nonces(4 * count), msgs(4 * count);
    for (size_t j = 0; j < count; ++j) {
        FrLocal k = K1;
        k.w[0] += j;                                                        // distinct keys below l
        const FrLocal n(7 * j + 1), m(1000 + j);
        std::copy(k.w.begin(), k.w.end(), keys.begin() + 4 * j);
        std::copy(n.w.begin(), n.w.end(), nonces.begin() + 4 * j);
        std::copy(m.w.begin(), m.w.end(), msgs.begin() + 4 * j);
    }
    void *d_k = nullptr, *d_n = nullptr, *d_m = nullptr, *d_p = nullptr, *d_s = nullptr, *d_b = nullptr, *d_b2 = nullptr, *d_st = nullptr;
    HIP_OK(hipMalloc(&d_k, 32 * count)); HIP_OK(hipMalloc(&d_n, 32 * count)); HIP_OK(hipMalloc(&d_m, 32 * count));
    HIP_OK(hipMalloc(&d_p, 160 * count)); HIP_OK(hipMalloc(&d_s, 32 * count));
    HIP_OK(hipMalloc(&d_b, stride * count)); HIP_OK(hipMalloc(&d_b2, stride * count)); HIP_OK(hipMalloc(&d_st, 4 * count));
    HIP_OK(hipMemcpy(d_k, keys.data(), 32 * count, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_n, nonces.data(), 32 * count, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_m, msgs.data(), 32 * count, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_p, 0xA5, 160 * count)); HIP_OK(hipMemset(d_s, 0xA5, 32 * count));
    HIP_OK(hipMemset(d_b, 0xA5, stride * count)); HIP_OK(hipMemset(d_b2, 0xA5, stride * count));
    eddsa::sign_batch(ctx, d_k, d_n, d_m, count, d_p, d_s, d_b, stride);
    eddsa::verify_batch(ctx, d_p, d_s, count, d_st, d_b2, stride);
    std::vector<uint32_t> status(count);
    std::vector<uint8_t> bits(count * stride), bits2(count * stride);
    std::vector<uint64_t> points(20 * count), s(4 * count);
    HIP_OK(hipMemcpy(status.data(), d_st, 4 * count, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bits.data(), d_b, count * stride, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bits2.data(), d_b2, count * stride, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(points.data(), d_p, 160 * count, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(s.data(), d_s, 32 * count, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < count; ++j) ASSERT(status[j] == ZK_EDDSA_VALID);
    ASSERT(bits == bits2);
    for (size_t j = 0; j < count; ++j)
        for (size_t i = 64; i < stride; ++i) ASSERT(bits[j * stride + i] == 0xA5);
    // instance 0 is what the host signs
    const babyjub::Point a = eddsa::public_key(K1);
    const eddsa::Signature sig = eddsa::sign(K1, FrLocal(1), FrLocal(1000));
    for (int i = 0; i < 4; ++i) {
        ASSERT(points[i] == a.x.w[i] && points[4 + i] == a.y.w[i]);
        ASSERT(points[8 + i] == sig.r8.x.w[i] && points[12 + i] == sig.r8.y.w[i]);
        ASSERT(points[16 + i] == FrLocal(1000).w[i] && s[i] == sig.s.w[i]);
    }
    // a key that is 0 refuses the call and writes nothing
    HIP_OK(hipMemset((char*)d_k + 32 * 64, 0, 32));
    HIP_OK(hipMemset(d_s, 0xA5, 32 * count));
    bool refused = false;
    try { eddsa::sign_batch(ctx, d_k, d_n, d_m, count, d_p, d_s); } catch (const Error& e) {
        refused = e.status == ZK_ERR_RANGE && std::string(e.what()).find("instance 64") != std::string::npos;
    }
    ASSERT(refused);
    HIP_OK(hipMemcpy(s.data(), d_s, 32 * count, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 4 * count; ++i) ASSERT(s[i] == 0xA5A5A5A5A5A5A5A5ull);
    refused = false;
    try { eddsa::sign_batch(ctx, d_k, d_n, d_m, count, d_p, d_s, d_b, 60); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused);
    for (void* p : {d_k, d_n, d_m, d_p, d_s, d_b, d_b2, d_st}) HIP_OK(hipFree(p));
    std::printf("ok batch_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    links_on_the_host();
    if (mode == "gpu") batch_on_the_device();
    return 0;
}
