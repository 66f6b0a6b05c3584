// tests/cpp/eddsa_modl_check.hip -- the arithmetic mod l of csrc/eddsa_modl.hpp on raw triples (rho, h, k): tests/test_eddsa_modl.py writes
// the triples, this program calls the product's own functions and prints what they return.  Signing can never choose h, so this is the
// only way to the edges of the two reductions.  No formula lives here.
//   eddsa_modl_check          the functions on the host, then in a one-block kernel
//   eddsa_modl_check --host   the host only (no GPU is touched): the mode tests/test_eddsa_modl.py runs under the sanitizers.  Built
//                             with -DMODL_CHECK_HOST_ONLY (hipcc --cuda-host-only has no code object to link) it has no other mode.
// stdin: one triple a line, 64 hex digits each, at most 1024 lines; h < 8 l.  Prints
//   "l V", "l2 V", "l4 V", "mu V"     the constants of modl_consts()
//   "host I H S" per triple           h mod l (modl_reduce_r) and (rho + 8 (h mod l) k) mod l (modl_response)
//   "device I H S" per triple         the same from the kernel
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "eddsa_modl.hpp"
using namespace zk;

enum { MAX_TRIPLES = 1024, BLOCK = 256 };

// in: 24 limbs a triple (rho, h, k); out: 16 limbs (h mod l, the response)
ZK_HD void one_triple(const uint32_t* in, uint32_t* out) {
    uint32_t rho[8], h[8], k[8], s[8];
    for (int i = 0; i < 8; ++i) { rho[i] = in[i]; h[i] = in[8 + i]; k[i] = in[16 + i]; }
    modl_response(rho, h, k, s);
    modl_reduce_r(h);
    for (int i = 0; i < 8; ++i) { out[i] = h[i]; out[8 + i] = s[i]; }
}

#ifndef MODL_CHECK_HOST_ONLY
__global__ __launch_bounds__(BLOCK) void k_triples(const uint32_t* __restrict__ in, int n, uint32_t* __restrict__ out) {
    for (int t = threadIdx.x; t < n; t += BLOCK) one_triple(in + 24 * t, out + 16 * t);
}
#endif

static bool parse(const std::string& s, uint32_t* l) {
    if (s.size() != 64 || s.find_first_not_of("0123456789abcdefABCDEF") != std::string::npos) return false;
    for (int i = 0; i < 8; ++i) l[7 - i] = (uint32_t)std::stoul(s.substr(8 * i, 8), nullptr, 16);
    return true;
}
static void print_limbs(const uint32_t* l, int n) {
    for (int i = n - 1; i >= 0; --i) std::printf("%08x", l[i]);
}
static void print_results(const char* tag, const uint32_t* out, int n) {
    for (int t = 0; t < n; ++t) {
        std::printf("%s %d ", tag, t);
        print_limbs(out + 16 * t, 8);
        std::printf(" ");
        print_limbs(out + 16 * t + 8, 8);
        std::printf("\n");
    }
}
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "eddsa_modl_check: %s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char** argv) {
    const bool host_only = argc == 2 && !std::strcmp(argv[1], "--host");
    if (argc != 1 && !host_only) { std::fprintf(stderr, "usage: eddsa_modl_check [--host] < triples\n"); return 1; }
    std::vector<uint32_t> in;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        std::string a, b, c;
        is >> a >> b >> c;
        in.resize(in.size() + 24);
        uint32_t* t = in.data() + in.size() - 24;
        if (!parse(a, t) || !parse(b, t + 8) || !parse(c, t + 16)) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 1; }
    }
    const int n = (int)(in.size() / 24);
    if (n == 0 || n > MAX_TRIPLES) { std::fprintf(stderr, "1..%d triples are expected, got %d\n", (int)MAX_TRIPLES, n); return 1; }
    constexpr ModlConsts C = modl_consts();
    std::printf("l "); print_limbs(C.l, 8);
    std::printf("\nl2 "); print_limbs(C.l2, 8);
    std::printf("\nl4 "); print_limbs(C.l4, 8);
    std::printf("\nmu "); print_limbs(C.mu, 9);
    std::printf("\n");
    // exact-size heap blocks, so that the sanitizers see every access past an end
    std::unique_ptr<uint32_t[]> req(new uint32_t[24 * n]), out(new uint32_t[16 * n]);
    std::memcpy(req.get(), in.data(), sizeof(uint32_t) * 24 * n);
    for (int t = 0; t < n; ++t) one_triple(req.get() + 24 * t, out.get() + 16 * t);
    print_results("host", out.get(), n);
#ifdef MODL_CHECK_HOST_ONLY
    if (!host_only) { std::fprintf(stderr, "built for the host only\n"); return 1; }
#else
    if (!host_only) {
        uint32_t *d_in = nullptr, *d_out = nullptr;
        HIP_OK(hipMalloc(&d_in, sizeof(uint32_t) * 24 * n));
        HIP_OK(hipMalloc(&d_out, sizeof(uint32_t) * 16 * n));
        HIP_OK(hipMemcpy(d_in, req.get(), sizeof(uint32_t) * 24 * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_out, 0xA5, sizeof(uint32_t) * 16 * n));
        hipLaunchKernelGGL(k_triples, dim3(1), dim3(BLOCK), 0, 0, d_in, n, d_out);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.get(), d_out, sizeof(uint32_t) * 16 * n, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_in));
        HIP_OK(hipFree(d_out));
        print_results("device", out.get(), n);
    }
#endif
    return 0;
}
