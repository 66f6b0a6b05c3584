// crs_from_powers.hip -- zk_crs_from_powers: the CRS of a circuit from a powers-of-tau transcript, by group operations only.
//
// zk_setup knows x: it evaluates every wire's beta u_i(x) + alpha v_i(x) + w_i(x) on SCALARS (k_setup_comb_sparse, crs.hip) and encrypts
// the m results.  Without x the same sum runs over POINTS:
//   wire i = sum_j u_ij [beta L_j]_1 + v_ij [alpha L_j]_1 + w_ij [L_j]_1                 (L_j: the Lagrange polynomial of gate j)
// a sparse matrix (the QAP's rows by wire, resident: u_wire, v_wire, w_wire) times three vectors of curve points.  The three vectors
// are one linear map applied to tau_g1, alpha_tau_g1 and beta_tau_g1:
//   roots of unity   [L_j] = 1/n sum_k w^-jk [x^k]: n-point inverse transform (k_gb_stage, gbasis.cuh), 1/n through k_g1_scale
//   integer roots    the transposed interpolation tree (group_interp_transpose, gbasis.hip)
// and xi_t_g1[k] = [x^k t(x)]_1 = sum_j t_j tau_g1[k + j]: tau_g1[n + k] - tau_g1[k] for t = X^n - 1; for the integer roots a
// correlation of 2n - 1 points with t's n + 1 coefficients, run as a cyclic convolution of N = 2^ceil(log2(2n - 1)) points at EVERY
// size (no direct form, no threshold): with rev[i] = t_{n-i} the linear convolution c[s] = sum_i rev[i] tau[s - i] has
// c[n + k] = xi_t[k], its support ends at 3n - 2, and n + k + N >= 3n - 1 for N >= 2n - 1, so nothing folds onto the wanted indices.
//
// k_wire_points.  Row values of real circuits are overwhelmingly 1 and -1, then small integers (the .zk front end's constants), and a
// few full-width ones (the powers of two of a bit decomposition, r - c).  One lane multiplying a 254-bit value would stall its wave
// for every entry, so the entries are partitioned by class first and only homogeneous lists are multiplied:
//   k_wire_classify   one lane per entry: +1 / -1 / zero are marked in slot[e]; a small value (|v| < 2^32, v or r - v) is appended to
//                     the small list, everything else to the full list, slot[e] = its place in the product array
//   k_wire_products   one lane per listed entry: SMALL: a double-and-add over the <= 32 bits of |v| with mixed additions; FULL: gb_mul
//                     (the endomorphism split).  The +-1 entries are never multiplied.
//   k_wire_points     sums a wire's entries: +-1 entries are ONE mixed addition of the Lagrange point (y negated for -1), the others one
//                     general addition of their product.  A row of at most WP_SPLIT entries (u, v and w together) is one lane's; longer
//                     rows (the constant wire, x in the chain circuit: up to 3n entries) are listed by k_wire_long_rows and take one
//                     work-group each: 256 lanes stride over the entries, then a tree over LDS.
// Every addition is madd_lazy / add_lazy / dbl_lazy of lazy29.cuh with their special cases: an infinity operand is skipped, P + P is
// doubled (madd_lazy's `false`, add_lazy's own branch), P - P clears the accumulator, and an empty row leaves it at infinity, which
// jac_to_affine writes as zeros -- what k_fixed_base_mul writes for the scalar 0.
#include "pipeline.hpp"
#include "interp.hpp"
#include "gbasis.cuh"

namespace zk {

constexpr int WP_SPLIT = 32;          // rows with more entries than this are summed by a work-group
constexpr int WP_LONG_BLOCK = 256;
constexpr uint32_t WP_POS1 = 0xFFFFFFFFu, WP_NEG1 = 0xFFFFFFFEu, WP_ZERO = 0xFFFFFFFDu;   // slot[e] of the entries without a product
constexpr uint32_t WP_FULL = 0x40000000u;   // slot[e] bit: the product sits behind the small ones

typedef FpR<FqParams> WpL;

// the three matrices by wire (u, v, w), the point array each multiplies (beta L, alpha L, L), and where each one's entries start in
// the concatenated entry numbering e = off[k] + position
struct WireMats {
    const uint32_t* ptr[3];
    const uint32_t* idx[3];
    const Fr* val[3];
    const G1A* lag[3];
    uint32_t off[4];
};
__device__ __forceinline__ int wp_matrix(const WireMats& M, uint32_t e) { return e >= M.off[2] ? 2 : (e >= M.off[1] ? 1 : 0); }

// |v| < 2^32 for v or r - v: the magnitude and the sign.  v canonical, non-zero.
__device__ __forceinline__ bool wp_small(const Fr& v, uint32_t& mag, bool& neg) {
    uint32_t hi = 0, nhi = 0, nl[8];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t d = (int64_t)FrParams::P[i] - v.l[i] + br;
        nl[i] = (uint32_t)d;
        br = d >> 32;
    }
#pragma unroll
    for (int i = 1; i < 8; ++i) { hi |= v.l[i]; nhi |= nl[i]; }
    if (!hi) { mag = v.l[0]; neg = false; return true; }
    if (!nhi) { mag = nl[0]; neg = true; return true; }
    return false;
}

__global__ void k_wire_classify(WireMats M, uint32_t* __restrict__ slot, uint32_t* __restrict__ list_small, uint32_t* __restrict__ list_full,
                                uint32_t* __restrict__ counts) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M.off[3]) return;
    const int k = wp_matrix(M, e);
    const Fr v = M.val[k][e - M.off[k]].to_canonical();
    if (v.is_zero()) { slot[e] = WP_ZERO; return; }
    uint32_t mag;
    bool neg;
    if (wp_small(v, mag, neg)) {
        if (mag == 1) { slot[e] = neg ? WP_NEG1 : WP_POS1; return; }
        const uint32_t at = atomicAdd(counts, 1u);
        list_small[at] = e;
        slot[e] = at;
        return;
    }
    const uint32_t at = atomicAdd(counts + 1, 1u);
    list_full[at] = e;
    slot[e] = at | WP_FULL;
}

// prod[i] = value(list[i]) * point(list[i])
template <bool FULL>
__global__ __launch_bounds__(64) void k_wire_products(WireMats M, const uint32_t* __restrict__ list, uint32_t count, Jac<Fq>* __restrict__ prod, Fq beta) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = list[i];
    const int k = wp_matrix(M, e);
    const uint32_t at = e - M.off[k];
    const G1A p = M.lag[k][M.idx[k][at]];
    const Fr v = M.val[k][at].to_canonical();
    if (FULL) {
        prod[i] = jacr_store(gb_mul(jacr_load(Jac<Fq>::from_affine(p)), v, beta));
        return;
    }
    uint32_t mag = 0;
    bool neg = false;
    (void)wp_small(v, mag, neg);
    JacR<Fq> acc = jacr_load(Jac<Fq>::infinity());
    if (!p.is_inf()) {
        const WpL x = WpL::load(p.x), yp = WpL::load(p.y), y = neg ? yp.neg().norm() : yp;
        for (int b = 31 - __clz(mag | 1); b >= 0; --b) {
            if (!acc.inf) acc = dbl_lazy(acc);
            if (((mag >> b) & 1) && !madd_lazy(acc, x, y)) acc = dbl_lazy(acc);
        }
    }
    prod[i] = jacr_store(acc);
}

// member by member: a whole-struct copy also moves JacR's three padding bytes, which the compiler does through scratch
__device__ __forceinline__ void wp_assign(JacR<Fq>& acc, const JacR<Fq>& r) { acc.X = r.X; acc.Y = r.Y; acc.Z = r.Z; acc.inf = r.inf; }

// acc += entry `at` of matrix k
__device__ __forceinline__ void wp_add_entry(JacR<Fq>& acc, const WireMats& M, int k, uint32_t at, const uint32_t* __restrict__ slot,
                                             const Jac<Fq>* __restrict__ prod, uint32_t n_small) {
    const uint32_t s = slot[M.off[k] + at];
    if (s == WP_ZERO) return;
    if (s >= WP_NEG1) {   // +-1: a mixed addition of the Lagrange point itself
        const G1A p = M.lag[k][M.idx[k][at]];
        if (p.is_inf()) return;
        const WpL yp = WpL::load(p.y);
        if (!madd_lazy(acc, WpL::load(p.x), s == WP_NEG1 ? yp.neg().norm() : yp)) wp_assign(acc, dbl_lazy(acc));
        return;
    }
    wp_assign(acc, add_lazy(acc, jacr_load(prod[(s & WP_FULL) ? n_small + (s & ~WP_FULL) : s])));
}
__device__ __forceinline__ uint32_t wp_row_len(const WireMats& M, uint32_t i) {
    return (M.ptr[0][i + 1] - M.ptr[0][i]) + (M.ptr[1][i + 1] - M.ptr[1][i]) + (M.ptr[2][i + 1] - M.ptr[2][i]);
}
__device__ __forceinline__ G1A* wp_out(uint32_t i, uint32_t input, G1A* sum_gamma, G1A* sum_delta) {
    return i <= input ? sum_gamma + i : sum_delta + (i - input - 1);
}

// the wires whose rows one lane does not sum
__global__ void k_wire_long_rows(WireMats M, uint32_t m, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (wp_row_len(M, i) > (uint32_t)WP_SPLIT) list[atomicAdd(count, 1u)] = i;
}

// LONG = false: one lane per wire, rows of at most WP_SPLIT entries.  LONG = true: one work-group per listed wire.
template <bool LONG>
__global__ __launch_bounds__(LONG ? WP_LONG_BLOCK : 64) void k_wire_points(WireMats M, uint32_t m, uint32_t input, const uint32_t* __restrict__ slot,
                                                                         const Jac<Fq>* __restrict__ prod, uint32_t n_small,
                                                                         const uint32_t* __restrict__ long_list, G1A* __restrict__ sum_gamma,
                                                                         G1A* __restrict__ sum_delta) {
    JacR<Fq> acc = jacr_load(Jac<Fq>::infinity());
    if (!LONG) {
        __shared__ Jac<Fq> sum[64];   // jac_to_affine is a call and takes its argument by reference: a sum in LDS keeps it out of scratch
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= m || wp_row_len(M, i) > (uint32_t)WP_SPLIT) return;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (uint32_t at = M.ptr[k][i]; at < M.ptr[k][i + 1]; ++at) wp_add_entry(acc, M, k, at, slot, prod, n_small);
        sum[threadIdx.x] = jacr_store(acc);
        *wp_out(i, input, sum_gamma, sum_delta) = jac_to_affine(sum[threadIdx.x]);
    } else {
        __shared__ Jac<Fq> part[WP_LONG_BLOCK];
        const uint32_t i = long_list[blockIdx.x], t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (uint32_t at = M.ptr[k][i] + t; at < M.ptr[k][i + 1]; at += WP_LONG_BLOCK) wp_add_entry(acc, M, k, at, slot, prod, n_small);
        part[t] = jacr_store(acc);
        __syncthreads();
        for (uint32_t s = WP_LONG_BLOCK / 2; s >= 1; s >>= 1) {
            if (t < s) part[t] = jacr_store(add_lazy(jacr_load(part[t]), jacr_load(part[t + s])));
            __syncthreads();
        }
        if (t == 0) *wp_out(i, input, sum_gamma, sum_delta) = jac_to_affine(part[0]);
    }
}

// out[brev(i)] = the affine image of in[i], i < 2^log_n
__global__ void k_fp_affine_brev(const Jac<Fq>* __restrict__ in, unsigned log_n, G1A* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << log_n)) return;
    const uint32_t j = log_n ? (__brev((uint32_t)i) >> (32 - log_n)) : 0;
    out[j] = jac_to_affine(in[i]);
}

// roots of unity: out[k] = tau[n + k] - tau[k], k < n - 1
__global__ __launch_bounds__(64) void k_xi_t_unity(const G1A* __restrict__ tau, size_t n, G1A* __restrict__ out) {
    __shared__ Jac<Fq> sum[64];   // as in k_wire_points
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k + 1 >= n) return;
    JacR<Fq> acc = jacr_load(Jac<Fq>::from_affine(tau[n + k]));
    const G1A b = tau[k];
    if (!b.is_inf() && !madd_lazy(acc, WpL::load(b.x), WpL::load(b.y).neg().norm())) acc = dbl_lazy(acc);
    sum[threadIdx.x] = jacr_store(acc);
    out[k] = jac_to_affine(sum[threadIdx.x]);
}

// data[p] = (mult[p] scale) data[p]: the point-wise product of two transforms (mult: Montgomery, in the points' own order)
__global__ __launch_bounds__(64) void k_fp_pointwise(Jac<Fq>* __restrict__ data, const Fr* __restrict__ mult, Fr scale, size_t count, Fq beta) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    data[p] = jacr_store(gb_mul(jacr_load(data[p]), (mult[p] * scale).to_canonical(), beta));
}
// rev[i] = t[n - i], i <= n; zero behind
__global__ void k_fp_reverse_t(const Fr* __restrict__ t, size_t n, size_t count, Fr* __restrict__ rev) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) rev[i] = i <= n ? t[n - i] : Fr::zero();
}

namespace {

// ctx->stream is what the shared launchers enqueue on: for the length of the call it is the call's own stream (as crs_check.hip)
struct OwnStream {
    zk_ctx* ctx;
    hipStream_t saved, own = nullptr;
    explicit OwnStream(zk_ctx* c) : ctx(c), saved(c->stream) {
        ZK_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        ctx->stream = own;
    }
    ~OwnStream() {
        ctx->stream = saved;
        (void)hipStreamSynchronize(own);
        (void)hipStreamDestroy(own);
    }
};

template <class A>
void up_points(zk_ctx* ctx, DevBuf<A>& d, const uint64_t* src, size_t count, int* d_flag) {
    d.alloc(std::max<size_t>(count, 1));
    ZK_HIP(hipMemcpyAsync(d.p, src, count * sizeof(A), hipMemcpyHostToDevice, ctx->stream));
    pts_to_mont<A>(ctx, d.p, d.p, count, d_flag);
    pts_check_on_curve<A>(ctx, d.p, count, d_flag);
}
int fetch_flag(zk_ctx* ctx, const int* d_flag) {
    int h = 0;
    ZK_HIP(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    return h;
}
template <class A>
void copy_points(zk_ctx* ctx, DevBuf<A>& dst, const A* src, size_t count) {
    dst.alloc(std::max<size_t>(count, 1));
    if (count) ZK_HIP(hipMemcpyAsync(dst.p, src, count * sizeof(A), hipMemcpyDeviceToDevice, ctx->stream));
}

// canonical w^j (or w^-j), j < 2^(log_n - 1), w of order 2^log_n
void twiddles(zk_ctx* ctx, unsigned log_n, bool inverse, DevBuf<Fr>& tw) {
    const size_t half = std::max<size_t>(((size_t)1 << log_n) / 2, 1);
    tw.alloc(half);
    const Fr w = host_root_of_unity(log_n);
    fr_powers(ctx, inverse ? w.inv() : w, Fr::one(), tw.p, half);
    fr_from_mont(ctx, tw.p, tw.p, half);
}

// roots of unity: lag[j] = 1/n sum_k w^-jk src[k], j < n = 2^log_n
void lagrange_unity(zk_ctx* ctx, unsigned log_n, const G1A* src, const Fr* tw_inv, G1A* lag) {
    const size_t n = (size_t)1 << log_n;
    hipStream_t st = ctx->stream;
    const Fq beta = glv_beta<Fq>();
    DevBuf<Jac<Fq>> data(n);
    hipLaunchKernelGGL(k_gb_load<Fq>, dim3(ceil_div(n, 256)), dim3(256), 0, st, src, n, n, data.p);
    for (unsigned stg = 0; stg < log_n; ++stg)   // decimation in frequency: natural -> bit-reversed
        hipLaunchKernelGGL((k_gb_stage<Fq, false>), dim3(ceil_div(n / 2, 64)), dim3(64), 0, st, data.p, n, log_n, stg, tw_inv, log_n, beta);
    hipLaunchKernelGGL(k_fp_affine_brev, dim3(ceil_div(n, 64)), dim3(64), 0, st, data.p, log_n, lag);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));   // data goes out of scope
    if (log_n) {
        Fr nn = Fr::zero();
        nn.l[0] = (uint32_t)n;
        g1_scale_resident(ctx, st, lag, lag, n, Fr::from_canonical(nn).inv().to_canonical());
    }
}

// integer roots: out[k] = sum_{j <= n} t[j] tau[k + j], k < n - 1 (tau: 2n - 1 points; t: n + 1 Montgomery coefficients)
void xi_t_correlation(zk_ctx* ctx, const G1A* tau, size_t n, const Fr* t, G1A* out) {
    hipStream_t st = ctx->stream;
    unsigned log_N = 0;
    while (((size_t)1 << log_N) < 2 * n - 1) ++log_N;
    const size_t N = (size_t)1 << log_N;
    const Fq beta = glv_beta<Fq>();
    DevBuf<Fr> rev(N), tw_f, tw_i;
    hipLaunchKernelGGL(k_fp_reverse_t, dim3(ceil_div(N, 256)), dim3(256), 0, st, t, n, N, rev.p);
    ZK_HIP(hipGetLastError());
    if (log_N) ntt_dif(ctx, rev.p, log_N, false, false);   // natural -> bit-reversed, as the points below
    twiddles(ctx, log_N, false, tw_f);
    twiddles(ctx, log_N, true, tw_i);
    DevBuf<Jac<Fq>> data(N);
    hipLaunchKernelGGL(k_gb_load<Fq>, dim3(ceil_div(N, 256)), dim3(256), 0, st, tau, 2 * n - 1, N, data.p);
    for (unsigned stg = 0; stg < log_N; ++stg)
        hipLaunchKernelGGL((k_gb_stage<Fq, false>), dim3(ceil_div(N / 2, 64)), dim3(64), 0, st, data.p, N, log_N, stg, tw_f.p, log_N, beta);
    const Fr n_inv = host_fr_pow(host_fr_from_u64(2), log_N).inv();   // the 1 / N of the inverse transform
    hipLaunchKernelGGL(k_fp_pointwise, dim3(ceil_div(N, 64)), dim3(64), 0, st, data.p, rev.p, n_inv, N, beta);
    for (unsigned stg = 0; stg < log_N; ++stg)   // decimation in time with the inverse twiddles: bit-reversed -> natural
        hipLaunchKernelGGL((k_gb_stage<Fq, true>), dim3(ceil_div(N / 2, 64)), dim3(64), 0, st, data.p, N, log_N, stg, tw_i.p, log_N, beta);
    hipLaunchKernelGGL(k_gb_affine<Fq>, dim3(ceil_div(n - 1, 64)), dim3(64), 0, st, data.p + n, n - 1, out);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));   // the temporaries go out of scope
}

void wire_points(zk_ctx* ctx, const zk_qap& q, const G1A* lag, const G1A* lag_alpha, const G1A* lag_beta, G1A* sum_gamma, G1A* sum_delta) {
    hipStream_t st = ctx->stream;
    const size_t m = q.m, total = q.u_wire.nnz + q.v_wire.nnz + q.w_wire.nnz;
    ZK_REQUIRE(total < WP_FULL && m < WP_FULL, ZK_ERR_SIZE, "zk_crs_from_powers: 2^30 row entries or wires, or more");
    WireMats M;
    const DevCsr* mats[3] = {&q.u_wire, &q.v_wire, &q.w_wire};
    const G1A* lags[3] = {lag_beta, lag_alpha, lag};
    M.off[0] = 0;
    for (int k = 0; k < 3; ++k) {
        M.ptr[k] = mats[k]->ptr.p; M.idx[k] = mats[k]->idx.p; M.val[k] = mats[k]->val.p; M.lag[k] = lags[k];
        M.off[k + 1] = M.off[k] + (uint32_t)mats[k]->nnz;
    }
    const Fq beta = glv_beta<Fq>();
    DevBuf<uint32_t> slot(std::max<size_t>(total, 1)), list_small(std::max<size_t>(total, 1)), list_full(std::max<size_t>(total, 1)), long_list(m), counts(3);
    ZK_HIP(hipMemsetAsync(counts.p, 0, 3 * sizeof(uint32_t), st));
    if (total) hipLaunchKernelGGL(k_wire_classify, dim3(ceil_div(total, 256)), dim3(256), 0, st, M, slot.p, list_small.p, list_full.p, counts.p);
    hipLaunchKernelGGL(k_wire_long_rows, dim3(ceil_div(m, 256)), dim3(256), 0, st, M, (uint32_t)m, long_list.p, counts.p + 2);
    ZK_HIP(hipGetLastError());
    uint32_t h[3];
    ZK_HIP(hipMemcpyAsync(h, counts.p, sizeof(h), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    const uint32_t n_small = h[0], n_full = h[1], n_long = h[2];
    DevBuf<Jac<Fq>> prod(std::max<size_t>((size_t)n_small + n_full, 1));
    if (n_small) hipLaunchKernelGGL((k_wire_products<false>), dim3(ceil_div(n_small, 64)), dim3(64), 0, st, M, list_small.p, n_small, prod.p, beta);
    if (n_full) hipLaunchKernelGGL((k_wire_products<true>), dim3(ceil_div(n_full, 64)), dim3(64), 0, st, M, list_full.p, n_full, prod.p + n_small, beta);
    hipLaunchKernelGGL((k_wire_points<false>), dim3(ceil_div(m, 64)), dim3(64), 0, st, M, (uint32_t)m, (uint32_t)q.input, slot.p, prod.p, n_small,
                       long_list.p, sum_gamma, sum_delta);
    if (n_long) hipLaunchKernelGGL((k_wire_points<true>), dim3(n_long), dim3(WP_LONG_BLOCK), 0, st, M, (uint32_t)m, (uint32_t)q.input, slot.p, prod.p, n_small,
                                   long_list.p, sum_gamma, sum_delta);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(st));   // the lists and the products go out of scope
}

}  // namespace

zk_crs* crs_from_powers(zk_ctx* ctx, const zk_qap& q, const zk_powers_desc& d) {
    ZK_REQUIRE(q.ctx == ctx, ZK_ERR_ARG, "zk_crs_from_powers: the QAP belongs to another context");
    ZK_REQUIRE(!q.dense, ZK_ERR_UNSUPPORTED, "zk_crs_from_powers: a dense QAP (only the roots-of-unity and the integer-roots forms are derived)");
    ZK_REQUIRE(q.roots != 2, ZK_ERR_UNSUPPORTED, "zk_crs_from_powers: an arbitrary-roots QAP (only the roots-of-unity and the integer-roots forms are derived)");
    ZK_REQUIRE(d.tau_g1 && d.tau_g2 && d.alpha_tau_g1 && d.beta_tau_g1 && d.beta_g2, ZK_ERR_ARG, "zk_crs_from_powers: null point array");
    const size_t n = q.n, m = q.m, l = q.input, nt = 2 * n - 1;
    const bool ap = q.roots == 1;
    ZK_REQUIRE(n >= 1 && d.n_tau_g1 >= nt, ZK_ERR_ARG, "zk_crs_from_powers: tau_g1 holds fewer than 2n - 1 powers");
    ZK_REQUIRE(d.n_rest >= n, ZK_ERR_ARG, "zk_crs_from_powers: tau_g2, alpha_tau_g1 or beta_tau_g1 holds fewer than n powers");
    ZK_REQUIRE(!ap || n <= ((size_t)1 << (NTT_MAX_LOG - 2)), ZK_ERR_UNSUPPORTED, "zk_crs_from_powers: an integer-roots QAP of more than 2^22 gates");
    OwnStream scope(ctx);
    hipStream_t st = ctx->stream;
    std::unique_ptr<zk_crs> c(new zk_crs());
    c->ctx = ctx;
    c->n = n; c->m = m; c->input = l;
    // ---- the transcript: range, curve, subgroup (zk_crs_upload's checks and statuses) ----
    DevBuf<G1A> tau, alpha_tau, beta_tau;
    DevBuf<int> flag(1);
    ZK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    up_points(ctx, tau, d.tau_g1, nt, flag.p);
    up_points(ctx, alpha_tau, d.alpha_tau_g1, n, flag.p);
    up_points(ctx, beta_tau, d.beta_tau_g1, n, flag.p);
    up_points(ctx, c->xi2, d.tau_g2, n, flag.p);
    up_points(ctx, c->beta2, d.beta_g2, 1, flag.p);
    int h = fetch_flag(ctx, flag.p);
    ZK_REQUIRE(!(h & 2), ZK_ERR_RANGE, "zk_crs_from_powers: coordinate >= q");
    ZK_REQUIRE(!(h & 4), ZK_ERR_RANGE, "zk_crs_from_powers: point not on the curve");
    g2_subgroup_check(ctx, c->beta2.p, 1, flag.p);
    g2_subgroup_check(ctx, c->xi2.p, n, flag.p);
    h = fetch_flag(ctx, flag.p);
    ZK_REQUIRE(!(h & 8), ZK_ERR_RANGE, "zk_crs_from_powers: G2 point outside the subgroup of order r");
    // ---- what is copied ----
    copy_points(ctx, c->alpha1, alpha_tau.p, 1);
    copy_points(ctx, c->beta1, beta_tau.p, 1);
    copy_points(ctx, c->delta1, tau.p, 1);
    copy_points(ctx, c->xi1, tau.p, n);
    copy_points(ctx, c->gamma2, c->xi2.p, 1);
    copy_points(ctx, c->delta2, c->xi2.p, 1);
    // ---- the three Lagrange arrays ----
    DevBuf<G1A> lag(n), lag_alpha(n), lag_beta(n);
    std::shared_ptr<InterpTree> tree;
    {
        ProfScope ps(ctx, "powers_lagrange", 6.0 * sizeof(G1A) * n, st);
        if (ap) {
            tree = integer_nodes_tree(ctx, 1, n);
            group_interp_transpose<Fq>(ctx, *tree, tau.p, lag.p);
            group_interp_transpose<Fq>(ctx, *tree, alpha_tau.p, lag_alpha.p);
            group_interp_transpose<Fq>(ctx, *tree, beta_tau.p, lag_beta.p);
        } else {
            DevBuf<Fr> tw_inv;
            twiddles(ctx, q.log_n, true, tw_inv);
            lagrange_unity(ctx, q.log_n, tau.p, tw_inv.p, lag.p);
            lagrange_unity(ctx, q.log_n, alpha_tau.p, tw_inv.p, lag_alpha.p);
            lagrange_unity(ctx, q.log_n, beta_tau.p, tw_inv.p, lag_beta.p);
        }
    }
    // ---- one point per wire ----
    c->sum_gamma1.alloc(l + 1);
    c->sum_delta1.alloc(std::max<size_t>(m - l - 1, 1));
    {
        ProfScope ps(ctx, "powers_wire_points", (double)sizeof(G1A) * m, st);
        wire_points(ctx, q, lag.p, lag_alpha.p, lag_beta.p, c->sum_gamma1.p, c->sum_delta1.p);
    }
    // ---- [x^k t(x)] ----
    c->xi_t1.alloc(std::max<size_t>(n - 1, 1));
    if (n >= 2) {
        ProfScope ps(ctx, "powers_xi_t", 2.0 * sizeof(G1A) * nt, st);
        if (ap) {
            xi_t_correlation(ctx, tau.p, n, tree->t.p, c->xi_t1.p);
        } else {
            hipLaunchKernelGGL(k_xi_t_unity, dim3(ceil_div(n - 1, 64)), dim3(64), 0, st, tau.p, n, c->xi_t1.p);
            ZK_HIP(hipGetLastError());
        }
    }
    if (ap) {   // the same CRS in the Lagrange bases of R = {1..n} and S = {n+1..2n-1}, as zk_setup attaches them
        ProfScope ps(ctx, "powers_lagrange", 0.0, st);
        c->lag1.alloc(n); c->lag2.alloc(n); c->lagS_t1.alloc(std::max<size_t>(n - 1, 1));
        ZK_HIP(hipMemcpyAsync(c->lag1.p, lag.p, n * sizeof(G1A), hipMemcpyDeviceToDevice, st));
        group_interp_transpose<Fq2>(ctx, *tree, c->xi2.p, c->lag2.p);
        if (n >= 2) {
            auto tree_s = integer_nodes_tree(ctx, (uint64_t)n + 1, n - 1);
            group_interp_transpose<Fq>(ctx, *tree_s, c->xi_t1.p, c->lagS_t1.p);
        }
        c->ap = true;
    }
    ZK_HIP(hipStreamSynchronize(st));
    return c.release();
}

}  // namespace zk
