// vk_batch.hip -- the device side of a verifying key (vk.hpp): zk_vk_from_crs, the binding of a key to a context, the batch
// verify calls over a key, and the fixed-base form of the input sums S_j = sum_gamma_0 + sum_{i=1..k} x_ji sum_gamma_i.
//
// The bases of a key are fixed, so each gets a window table once per key and context:
//   k_vk_table    T[i][s][d] = d 2^(4 s) sum_gamma_i for base i = 1..l, window s < 64, digit d = 1..15 (affine, Montgomery).  One
//                 block per base, one lane per window: 4 s doublings, the 15 multiples by complete additions, and ONE inversion
//                 for the lane's 15 points (prefix products kept in LDS).  A base at infinity gives 15 infinities.
//   k_vk_inputs   one lane per proof: S_j = sum_gamma_0 + sum_i sum_s T[i][s][digit_s(x_ji)], zero digits skipped, no doublings,
//                 at most 64 complete mixed additions per input against the 254 / k doublings + ~127 additions of k_vb_inputs.
// Affine coordinates are canonical, so S_j is bit for bit k_vb_inputs' whatever the order of the additions.
// Everything runs on the verify stream of the context (verify_batch.hpp); buffers that go out of use are retired, never freed
// under a ticket.
#define ZK_MUL_OUTLINE 1
#include "pipeline.hpp"
#include "pairing.cuh"
#include "verify_batch.hpp"

namespace zk {

static constexpr int VK_BLOCK = 64;
static_assert(VK_WINDOWS == VK_BLOCK, "k_vk_table: one lane per window");

// sg: the l + 1 bases (entry 0 takes no table); T: l x VK_WINDOWS x VK_ENTRIES points
__global__ void __launch_bounds__(VK_BLOCK) k_vk_table(const G1A* sg, size_t l, G1A* T) {
    __shared__ uint32_t zs[VK_ENTRIES][8][VK_BLOCK];   // Z of the lane's d-th multiple (0: infinity)
    __shared__ uint32_t pf[VK_ENTRIES][8][VK_BLOCK];   // product of the finite Z's up to d
    const size_t i = blockIdx.x;
    const int s = threadIdx.x;
    if (i >= l) return;
    G1J B = G1J::from_affine(sg[i + 1]);
    for (int t = 0; t < VK_WINDOW_BITS * (VK_WINDOWS - 1); ++t)
        if (t < VK_WINDOW_BITS * s) B = jac_dbl_ni(B);
    G1A* out = T + (i * VK_WINDOWS + s) * VK_ENTRIES;
    G1J acc = B;
    Fq run = Fq::one();
    for (int d = 0; d < VK_ENTRIES; ++d) {   // acc = (d + 1) B: X, Y parked in the entry, Z in LDS
        out[d] = G1A{acc.X, acc.Y};
        const bool inf = acc.is_inf();
        if (!inf) run = run * acc.Z;
        for (int h = 0; h < 8; ++h) {
            zs[d][h][s] = inf ? 0u : acc.Z.l[h];
            pf[d][h][s] = run.l[h];
        }
        acc = jac_add_ni(acc, B);
    }
    Fq inv = run.inv();   // one inversion for the lane's 15 points (run = 1 when all are infinity)
    for (int d = VK_ENTRIES - 1; d >= 0; --d) {
        Fq z, before = Fq::one();
        for (int h = 0; h < 8; ++h) z.l[h] = zs[d][h][s];
        if (z.is_zero()) {
            out[d] = G1A::infinity();
            continue;
        }
        if (d)
            for (int h = 0; h < 8; ++h) before.l[h] = pf[d - 1][h][s];
        const Fq zi = inv * before;   // 1 / Z_d
        inv = inv * z;
        const Fq zi2 = zi.sqr();
        const G1A p = out[d];
        out[d] = G1A{p.x * zi2, p.y * zi2 * zi};
    }
}

// x: n rows of k canonical inputs (4 words each), all < r (checked on the host); sg[0] the constant wire's base; T as above
__global__ void __launch_bounds__(VK_BLOCK) k_vk_inputs(const uint64_t* x, size_t k, const G1A* sg, const G1A* T, size_t n, G1A* S) {
    const size_t j = (size_t)blockIdx.x * VK_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint64_t* xj = x + j * k * 4;
    G1J acc = G1J::infinity();
    for (size_t i = 0; i < k; ++i) {
        const G1A* Ti = T + i * (size_t)(VK_WINDOWS * VK_ENTRIES);
        for (int w = 0; w < 4; ++w) {
            uint64_t v = xj[4 * i + w];
            for (int s = 16 * w; v; ++s, v >>= VK_WINDOW_BITS) {
                const unsigned d = (unsigned)v & VK_ENTRIES;
                if (d) acc = jac_madd_ni(acc, Ti[s * VK_ENTRIES + d - 1]);
            }
        }
    }
    S[j] = jac_to_affine(jac_madd_ni(acc, sg[0]));
}

void vk_launch_inputs(const uint64_t* d_x, size_t k, const G1A* d_sg, const G1A* d_tab, size_t m, G1A* d_S, hipStream_t s) {
    hipLaunchKernelGGL(k_vk_inputs, dim3(ceil_div(m, VK_BLOCK)), dim3(VK_BLOCK), 0, s, d_x, k, d_sg, d_tab, m, d_S);
    ZK_HIP(hipGetLastError());
}

namespace {

// zk_vk_free before zk_ctx_destroy: the buffers go to the context's retired list and the context forgets the key
void vk_retire(VkBinding& b) {
    if (!b.alive || !b.ctx || !b.ctx->verify_batch) return;
    VerifyBatchState& st = *b.ctx->verify_batch;
    if (b.consts.p) st.retired.push_back(std::move(b.consts));
    if (b.tables.p) st.retired.push_back(std::move(b.tables));
    for (size_t i = 0; i < st.keys.size(); ++i)
        if (st.keys[i].get() == &b) {
            st.keys.erase(st.keys.begin() + i);   // the key still holds the binding: `b` outlives this line
            break;
        }
}

bool vk_tables_allowed(const zk_ctx* ctx, const zk_vk& vk) {
    const long cap = ctx->opt_vk_table_kib;
    return vk.input > 0 && cap > 0 && vk_table_bytes(vk.input) <= (size_t)cap * 1024;
}

// The key's constants on this context (uploaded on the first call) and, when `want_tables`, its tables (built on the first call
// that may use them).  ZK_ERR_ARG for a key bound to another context or to one that is gone.
VerifyConsts vk_bind(zk_ctx* ctx, zk_vk* vk, bool want_tables) {
    VerifyBatchState& st = vb_state(ctx);
    hipStream_t s = st.stream;
    if (vk->binding) {
        ZK_REQUIRE(vk->binding->alive, ZK_ERR_ARG, "vk: the context this key was bound to has been destroyed");
        ZK_REQUIRE(vk->binding->ctx == ctx, ZK_ERR_ARG, "vk: the key is bound to another context");
    } else {
        auto b = std::make_shared<VkBinding>();
        b->ctx = ctx;
        b->retire = vk_retire;
        auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t l = vk->input;
        b->o_c = up(2 * ATE_LINES * sizeof(Line));
        b->o_sg = b->o_c + up(sizeof(Fq12));
        b->consts.alloc(b->o_sg + up((l + 1) * sizeof(G1A)));
        ZK_HIP(hipMemcpyAsync(b->consts.p, &vk->fx->lines[1][0], 2 * ATE_LINES * sizeof(Line), hipMemcpyHostToDevice, s));   // gamma | delta
        ZK_HIP(hipMemcpyAsync(b->consts.p + b->o_c, &vk->c, sizeof(Fq12), hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(b->consts.p + b->o_sg, vk->sg.data(), (l + 1) * sizeof(G1A), hipMemcpyHostToDevice, s));
        ZK_HIP(hipStreamSynchronize(s));
        st.keys.push_back(b);
        vk->binding = b;
    }
    VkBinding& b = *vk->binding;
    VerifyConsts vc;
    vc.l = vk->input;
    vc.d_lines = (const Line*)b.consts.p;
    vc.d_c = (const Fq12*)(b.consts.p + b.o_c);
    vc.d_sg = (const G1A*)(b.consts.p + b.o_sg);
    vc.alpha = vk->alpha;
    if (want_tables && vk_tables_allowed(ctx, *vk)) {
        if (!b.tables.p && !b.tables_refused) {
            DevBuf<uint8_t> t;
            try {
                t.alloc(vk_table_bytes(vk->input));
            } catch (const HipError& e) {
                // no room for the tables: a memory condition like the cap, so the bit-serial kernel serves this key from now on
                if (e.code != hipErrorOutOfMemory) throw;
                (void)hipGetLastError();
                b.tables_refused = true;
                return vc;
            }
            hipLaunchKernelGGL(k_vk_table, dim3((unsigned)vk->input), dim3(VK_BLOCK), 0, s, vc.d_sg, vk->input, (G1A*)t.p);
            ZK_HIP(hipGetLastError());
            ZK_HIP(hipStreamSynchronize(s));
            b.tables = std::move(t);
        }
        vc.d_tab = (const G1A*)b.tables.p;   // null after a refused allocation
    }
    return vc;
}

void point_words(const G1A& p, uint64_t* w) {
    words_of(p.x, w);
    words_of(p.y, w + 4);
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zk_vk_from_crs(zk_ctx* ctx, const zk_crs* crs, zk_vk** out) {
    if (!ctx || !crs || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return guarded(ctx, [&] {
        hipStream_t s = vb_state(ctx).stream;
        const size_t l = crs->input;
        G1A h_alpha;
        G2A h_g2[3];
        std::vector<G1A> h_sg(l + 1);
        ZK_HIP(hipMemcpyAsync(&h_alpha, crs->alpha1.p, sizeof(G1A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_g2[0], crs->beta2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_g2[1], crs->gamma2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(&h_g2[2], crs->delta2.p, sizeof(G2A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(h_sg.data(), crs->sum_gamma1.p, (l + 1) * sizeof(G1A), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipStreamSynchronize(s));
        std::vector<uint64_t> w(vk_payload_words(l));
        point_words(h_alpha, w.data());
        for (int q = 0; q < 3; ++q) {
            uint64_t* o = w.data() + 8 + 16 * q;
            words_of(h_g2[q].x.c0, o); words_of(h_g2[q].x.c1, o + 4); words_of(h_g2[q].y.c0, o + 8); words_of(h_g2[q].y.c1, o + 12);
        }
        for (size_t i = 0; i <= l; ++i) point_words(h_sg[i], w.data() + 56 + 8 * i);
        const zk_vk_desc d{l, w.data(), w.data() + 8, w.data() + 24, w.data() + 40, w.data() + 56};
        const int rc = zk_vk_create(&d, out);
        ZK_REQUIRE(rc == ZK_OK, rc, "vk_from_crs: CRS point not on the curve or outside G2");
    });
}

static int vk_verify_batch_impl(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs,
                                int* ok, bool compressed) {
    if (!ctx || !vk) return ZK_ERR_ARG;
    if (n_proofs == 0) return ZK_OK;
    if (!proofs || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    std::fill(ok, ok + n_proofs, 0);
    return guarded(ctx, [&] {
        vb_check_inputs(inputs, n_inputs, std::min(vk->input, n_inputs), n_proofs, "verify_batch: input >= r");
        const VerifyConsts vc = vk_bind(ctx, vk, true);
        verify_batch_run(ctx, vc, inputs, n_inputs, proofs, n_proofs, ok, compressed);
    });
}
int zk_vk_verify_batch(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs, int* ok) {
    return vk_verify_batch_impl(ctx, vk, inputs, n_inputs, proofs, n_proofs, ok, false);
}
int zk_vk_verify_batch_compressed(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                                  size_t n_proofs, int* ok) {
    return vk_verify_batch_impl(ctx, vk, inputs, n_inputs, proofs, n_proofs, ok, true);
}

int zk_vk_verify_batch_all(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs,
                           const uint64_t* z, int* ok) {
    if (!ctx || !vk || !proofs || !z || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    *ok = 0;
    if (n_proofs == 0) {
        *ok = 1;
        return ZK_OK;
    }
    return guarded(ctx, [&] {
        uint64_t t0[4];
        vba_check(z, inputs, n_inputs, std::min(vk->input, n_inputs), n_proofs, t0);
        const VerifyConsts vc = vk_bind(ctx, vk, false);   // T_S is one product per call: no tables
        auto fx = std::make_unique<VbaFixed>(*vk->fx);
        verify_batch_all_run(ctx, vc, *fx, t0, inputs, n_inputs, proofs, n_proofs, z, ok);
    });
}

int zk_vk_input_sums(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, size_t n, int tables, uint64_t* out) {
    if (!ctx || !vk) return ZK_ERR_ARG;
    if (n == 0) return ZK_OK;
    if (!out || (n_inputs && !inputs)) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        const size_t k = std::min(vk->input, n_inputs);
        vb_check_inputs(inputs, n_inputs, k, n, "vk_input_sums: input >= r");
        ZK_REQUIRE(!tables || vk->input == 0 || vk_tables_allowed(ctx, *vk), ZK_ERR_SIZE, "vk_input_sums: the key's tables exceed the option vk_table_kib");
        const VerifyConsts vc = vk_bind(ctx, vk, tables != 0);
        ZK_REQUIRE(!tables || k == 0 || vc.d_tab, ZK_ERR_SIZE, "vk_input_sums: no device memory for the key's tables");
        VerifyBatchState& st = vb_state(ctx);
        hipStream_t s = st.stream;
        const size_t m_max = std::min(n, (size_t)ZK_VERIFY_BATCH_CHUNK);
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_x = 0, o_S = o_x + up(m_max * k * 32), total = o_S + up(m_max * sizeof(G1A));
        if (st.arena.n < total) {
            if (st.arena.p) st.retired.push_back(std::move(st.arena));
            st.arena.alloc(total);
        }
        uint64_t* d_x = (uint64_t*)(st.arena.p + o_x);
        G1A* d_S = (G1A*)(st.arena.p + o_S);
        std::vector<G1A> h_S(m_max);
        for (size_t j0 = 0; j0 < n; j0 += m_max) {
            const size_t m = std::min(m_max, n - j0);
            if (k)   // only the first k inputs of a row are read (zip truncation)
                ZK_HIP(hipMemcpy2DAsync(d_x, k * 32, inputs + j0 * n_inputs * 4, n_inputs * 32, k * 32, m, hipMemcpyHostToDevice, s));
            if (tables) vk_launch_inputs(d_x, k, vc.d_sg, vc.d_tab, m, d_S, s);
            else vb_launch_inputs(d_x, k, vc.d_sg, m, d_S, s);
            ZK_HIP(hipMemcpyAsync(h_S.data(), d_S, m * sizeof(G1A), hipMemcpyDeviceToHost, s));
            ZK_HIP(hipStreamSynchronize(s));
            for (size_t j = 0; j < m; ++j) point_words(h_S[j], out + (j0 + j) * 8);
        }
    });
}

}  // extern "C"
