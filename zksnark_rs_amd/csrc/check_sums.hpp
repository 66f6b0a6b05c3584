// check_sums.hpp -- what the checks that test arrays of points through random linear combinations share (crs_check.hip: zk_crs_check;
// powers.hip: zk_powers_check): a stream of the call's own, the gatherer of the inner products, and the pairing product on the host.
#pragma once
#include <initializer_list>
#include <random>
#include <vector>
#include "pipeline.hpp"
#include "pairing.cuh"

namespace zk {
namespace {

// ctx->stream is what the shared launchers (spmv, the transforms, msm_build_table) enqueue on: for the length of one check it is the
// call's own stream, so that nothing of the check is ordered into -- or waits behind -- the prover's main stream.
struct StreamScope {
    zk_ctx* ctx;
    hipStream_t saved, own = nullptr;
    explicit StreamScope(zk_ctx* c) : ctx(c), saved(c->stream) {
        ZK_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        ctx->stream = own;
    }
    ~StreamScope() {
        ctx->stream = saved;
        (void)hipStreamSynchronize(own);
        (void)hipStreamDestroy(own);
    }
};

template <class T>
T fetch(const T* d, hipStream_t st) {
    T h;
    ZK_HIP(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return h;
}

Fr fr_from_u64x4(const uint64_t* w) {
    Fr x;
    for (int i = 0; i < 4; ++i) { x.l[2 * i] = (uint32_t)w[i]; x.l[2 * i + 1] = (uint32_t)(w[i] >> 32); }
    return x;
}

// 256 bits from the OS, reduced mod r; never 0
Fr draw_challenge() {
    std::random_device rd;
    for (;;) {
        Fr x;
        for (int i = 0; i < 8; ++i) x.l[i] = (uint32_t)rd();
        while (!x.raw_in_range()) {           // 2^256 < 6 r
            uint64_t borrow = 0;
            for (int i = 0; i < 8; ++i) {
                const uint64_t d = (uint64_t)x.l[i] - FrParams::P[i] - borrow;
                x.l[i] = (uint32_t)d;
                borrow = (d >> 32) & 1;
            }
        }
        if (!x.is_zero()) return x;
    }
}

struct Pair {
    G1A p;
    G2A q;
};
// prod e(p_i, q_i) == 1: one product of Miller values, one final exponentiation
bool pairing_product_is_one(std::initializer_list<Pair> terms) {
    Fq12 f = Fq12::one();
    for (const Pair& t : terms) f = f * ml_proj(t.p, t.q);
    return final_exp_exact(f) == Fq12::one();
}

template <class F>
bool same_point(const Aff<F>& a, const Aff<F>& b) { return a.x == b.x && a.y == b.y; }

// the inner products of one check: results gathered on the device, read once
struct Sums {
    zk_ctx* ctx;
    MsmWorkspace ws;
    DevBuf<G1J> d1;
    DevBuf<G2J> d2;
    size_t n1 = 0, n2 = 0;
    explicit Sums(zk_ctx* c) : ctx(c), d1(24), d2(8) {}
    // a sum over no points (n = 1: no xi_t; input = m - 1: no sum_delta) has no table to run over
    template <class F>
    size_t empty(Jac<F>* d, size_t& counter) {
        static const Jac<F> inf = Jac<F>::infinity();
        ZK_HIP(hipMemcpyAsync(d, &inf, sizeof(inf), hipMemcpyHostToDevice, ctx->stream));
        return counter++;
    }
    size_t g1(const MsmTable<Fq>& t, const Fr* sc, size_t count, size_t off = 0) {
        ZK_REQUIRE(n1 < d1.n, ZK_ERR_ARG, "crs_check: too many sums");
        if (!count) return empty(d1.p + n1, n1);
        msm_run<Fq>(ctx, ws, ctx->stream, t, sc, count, 0, 1, d1.p + n1, nullptr, nullptr, off);
        return n1++;
    }
    size_t g2(const MsmTable<Fq2>& t, const Fr* sc, size_t count, size_t off = 0) {
        ZK_REQUIRE(n2 < d2.n, ZK_ERR_ARG, "crs_check: too many sums");
        if (!count) return empty(d2.p + n2, n2);
        msm_run<Fq2>(ctx, ws, ctx->stream, t, sc, count, 0, 1, d2.p + n2, nullptr, nullptr, off);
        return n2++;
    }
    std::vector<G1A> h1;
    std::vector<G2A> h2;
    void read() {
        std::vector<G1J> j1(std::max<size_t>(n1, 1));
        std::vector<G2J> j2(std::max<size_t>(n2, 1));
        if (n1) ZK_HIP(hipMemcpyAsync(j1.data(), d1.p, n1 * sizeof(G1J), hipMemcpyDeviceToHost, ctx->stream));
        if (n2) ZK_HIP(hipMemcpyAsync(j2.data(), d2.p, n2 * sizeof(G2J), hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
        h1.resize(n1);
        h2.resize(n2);
        for (size_t i = 0; i < n1; ++i) h1[i] = jac_to_affine(j1[i]);
        for (size_t i = 0; i < n2; ++i) h2[i] = jac_to_affine(j2[i]);
    }
};

}  // namespace
}  // namespace zk
