// qap_check.hip -- zk_qap_check / zk_qap_check_dev: does a witness satisfy the QAP, and which gate fails first?
//
// groth16::prove drops the remainder of (U V - W) / t (groth16/mod.rs:233-253,277), so an unsatisfying
// witness costs a whole proof and comes back as 259 well-formed bytes.  The check answers per witness, for one or for `count` of them
// resident in HBM (zk_witgen_run's layout), before anything is proved:
//   k_qc_init     per instance: {bad_gates = 0, first_bad = NONE, flags = (weights[0] != 1)} -- the result record itself
//   k_qc_range    per (instance, element < a_len): word pattern >= r -> atomicMin of the instance index into a flag word
//   k_qap_check   per (instance, gate): the three row sums U_j, V_j, W_j in the lazy radix exactly as k_spmv forms them (qap.hip), one
//                 Montgomery product, one exact reduction per side, an 8-limb compare.  No field element is stored.  Failing lanes are
//                 counted within the wave (ballot / popcount; the lowest failing lane of an instance holds its lowest gate) and leave
//                 one atomicAdd and one atomicMin per (wave, failing instance): a satisfying batch issues no atomic at all.
// W by gate (zk_qap::w_gate) is what the prover never needs: it is built by the first check of a handle from w_wire -- downloaded
// once, transposed by the counting sort of upload_rows, converted once more (w_wire holds val R, the rows by gate hold val R^2 so that
// a CANONICAL witness element times a stored value is a Montgomery form) and uploaded.
// Everything runs on the call's own stream; buffers that have to grow are parked, never freed under an outstanding proof.
#include <algorithm>
#include "pipeline.hpp"
#include "fr_tile.cuh"

namespace zk {

struct QapCheckState {
    hipStream_t stream = nullptr;
    DevBuf<uint8_t> wit, res, flag;        // a host witness, the results of one chunk, the range flag
    std::vector<DevBuf<uint8_t>> retired;  // hipFree would wait for every stream of the device (an outstanding proof included)
    ~QapCheckState() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    void grow(DevBuf<uint8_t>& b, size_t bytes) {
        if (b.n >= bytes) return;
        if (b.p) retired.push_back(std::move(b));
        b.alloc(bytes);
    }
};

static constexpr int QC_BLOCK = 256;
static constexpr unsigned long long QC_NO_ERROR = ~0ull;
static constexpr size_t QC_MAX_LANES = (size_t)1 << 30;   // lane indices of one launch stay 32-bit

struct QcCsr {
    const uint32_t* ptr;
    const uint32_t* idx;
    const Fr* val;
};
static QcCsr qc_view(const DevCsr& m) { return QcCsr{m.ptr.p, m.idx.p, m.val.p}; }

// sum_k a[idx[k]] * val[k] over row j: k_spmv's loop (qap.hip) and its bound -- |value| below 2^7 p whatever the row length
__device__ __forceinline__ FrL qc_row_sum(const QcCsr& m, const Fr* __restrict__ a, size_t a_len, uint32_t j) {
    FrL acc = FrL::load(Fr::zero());
    uint32_t cnt = 0;
    for (uint32_t k = m.ptr[j]; k < m.ptr[j + 1]; ++k) {
        const uint32_t i = m.idx[k];
        if (i < a_len) {   // zip(weights) truncates (mod.rs:233-253)
            acc = (acc + FrL::load(a[i]) * FrL::load(m.val[k])).norm();
            if ((++cnt & 63u) == 0) acc = fr_reduce(acc);
        }
    }
    return acc;
}

__global__ void __launch_bounds__(QC_BLOCK) k_qc_init(const Fr* __restrict__ a, size_t stride, size_t a_len, uint32_t insts,
                                                      zk_qap_check_result* __restrict__ res) {
    const uint32_t i = blockIdx.x * QC_BLOCK + threadIdx.x;
    if (i >= insts) return;
    uint32_t rest = 1;
    if (a_len) {
        const Fr x = a[(size_t)i * stride];
        rest = x.l[0] ^ 1u;
#pragma unroll
        for (int k = 1; k < 8; ++k) rest |= x.l[k];
    }
    zk_qap_check_result r;
    r.bad_gates = 0;
    r.first_bad = ZK_QAP_CHECK_NONE;
    r.flags = rest ? ZK_QAP_CHECK_WIRE0 : 0u;
    res[i] = r;
}

// block = bx elements x by instances (bx * by = QC_BLOCK); instances strided over gridDim.y
__global__ void __launch_bounds__(QC_BLOCK) k_qc_range(const Fr* __restrict__ a, size_t stride, size_t a_len, uint32_t insts, size_t first,
                                                       unsigned long long* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a_len) return;
    for (size_t j = (size_t)blockIdx.y * blockDim.y + threadIdx.y; j < insts; j += (size_t)gridDim.y * blockDim.y)
        if (!a[j * stride + i].raw_in_range()) atomicMin(flag, (unsigned long long)(first + j));
}

// BY_INSTANCE = false: lane t -> (instance t / n, gate t % n): consecutive lanes read consecutive rows (coalesced row data), one
// instance's witness stays in cache.  true: lane t -> (gate t / insts, instance t % insts): the row data is wave-uniform, the witness
// reads are strided by the instance size.  insts * n < 2^31 (launcher).
template <bool BY_INSTANCE>
__global__ void __launch_bounds__(QC_BLOCK) k_qap_check(QcCsr u, QcCsr v, QcCsr w, const Fr* __restrict__ a, size_t stride, size_t a_len,
                                                        uint32_t n, uint32_t insts, zk_qap_check_result* __restrict__ res) {
    ZK_LATENCY_KERNEL();
    const uint32_t t = blockIdx.x * QC_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t inst = 0, gate = 0;
    bool bad = false;
    if (t < insts * n) {   // lanes behind the end take part in the ballots below
        if (BY_INSTANCE) { gate = t / insts; inst = t - gate * insts; }
        else { inst = t / n; gate = t - inst * n; }
        const Fr* wit = a + (size_t)inst * stride;
        const FrL U = fr_reduce(qc_row_sum(u, wit, a_len, gate));   // (-p - eps, 2p): multipliable
        const FrL V = fr_reduce(qc_row_sum(v, wit, a_len, gate));
        const Fr lhs = fr_store_exact(U * V);                       // u v R
        const Fr rhs = fr_store_exact(qc_row_sum(w, wit, a_len, gate));   // w R
        bad = !(lhs == rhs);
    }
    // Per (wave, failing instance): the count and, from the lowest failing lane, the lowest gate -- in both mappings the gates of one
    // instance ascend with the lane.  A wave without a failing lane leaves here at once.
    unsigned long long left = __ballot(bad);
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const uint32_t lead_inst = (uint32_t)__shfl((int)inst, lead);
        const bool mine = bad && inst == lead_inst;
        const unsigned long long set = __ballot(mine);
        if ((int)lane == lead) {
            atomicAdd(&res[inst].bad_gates, (uint32_t)__popcll(set));
            atomicMin(&res[inst].first_bad, gate);
        }
        bad = bad && !mine;
        left &= ~set;
    }
}

// w_wire (by wire, val R) -> w_gate (by gate, val R^2), once per handle
void qc_ensure_w_gate(const zk_qap& q, hipStream_t s) {
    if (q.has_w_gate) return;
    const DevCsr& src = q.w_wire;
    const size_t m = q.m, n = q.n, nnz = src.nnz;
    ZK_REQUIRE(src.rows == m, ZK_ERR_ARG, "qap_check: the QAP holds no rows of w");
    std::vector<uint32_t> ptr(m + 1), idx(nnz);
    std::vector<Fr> val(nnz);
    ZK_HIP(hipMemcpyAsync(ptr.data(), src.ptr.p, (m + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (nnz) {
        ZK_HIP(hipMemcpyAsync(idx.data(), src.idx.p, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        ZK_HIP(hipMemcpyAsync(val.data(), src.val.p, nnz * sizeof(Fr), hipMemcpyDeviceToHost, s));
    }
    ZK_HIP(hipStreamSynchronize(s));
    // counting-sort transpose (upload_rows, qap.hip): rows = gates, columns = wires, entries of a gate in wire order
    std::vector<uint32_t> gptr(n + 1, 0), gidx(nnz);
    std::vector<Fr> gval(nnz);
    for (size_t k = 0; k < nnz; ++k) ++gptr[idx[k] + 1];
    for (size_t j = 0; j < n; ++j) gptr[j + 1] += gptr[j];
    std::vector<uint32_t> cur(gptr.begin(), gptr.end() - 1);
    for (size_t i = 0; i < m; ++i)
        for (size_t k = ptr[i]; k < ptr[i + 1]; ++k) {
            const uint32_t pos = cur[idx[k]]++;
            gidx[pos] = (uint32_t)i;
            gval[pos] = Fr::from_canonical(val[k]);   // (val R) R
        }
    DevCsr& d = q.w_gate;
    d.rows = n;
    d.nnz = nnz;
    d.ptr.alloc(n + 1);
    d.idx.alloc(std::max<size_t>(nnz, 1));
    d.val.alloc(std::max<size_t>(nnz, 1));
    ZK_HIP(hipMemcpyAsync(d.ptr.p, gptr.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (nnz) {
        ZK_HIP(hipMemcpyAsync(d.idx.p, gidx.data(), nnz * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        ZK_HIP(hipMemcpyAsync(d.val.p, gval.data(), nnz * sizeof(Fr), hipMemcpyHostToDevice, s));
    }
    ZK_HIP(hipStreamSynchronize(s));   // the host vectors go out of scope
    q.has_w_gate = true;
}

static QapCheckState& qc_state(zk_ctx* ctx) {
    if (!ctx->qap_check) ctx->qap_check = std::make_shared<QapCheckState>();
    QapCheckState& st = *ctx->qap_check;
    if (!st.stream) ZK_HIP(hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking));
    return st;
}

// d_a: `count` witnesses of a_len elements read each, `stride` elements apart, on the device
static void qc_run(zk_ctx* ctx, QapCheckState& st, const zk_qap& q, const Fr* d_a, size_t a_len, size_t stride, size_t count,
                   zk_qap_check_result* out) {
    hipStream_t s = st.stream;
    const size_t n = q.n;
    ZK_REQUIRE(n >= 1 && n <= QC_MAX_LANES, ZK_ERR_SIZE, "qap_check: too many gates");
    qc_ensure_w_gate(q, s);
    const size_t cap = (size_t)std::min<long>(std::max<long>(ctx->opt_qap_check_chunk, 1), (long)QC_MAX_LANES);
    const size_t chunk = std::min(count, std::max<size_t>(cap / n, 1));   // chunk * n <= max(n, cap) <= 2^30
    st.grow(st.res, chunk * sizeof(zk_qap_check_result));
    st.grow(st.flag, sizeof(unsigned long long));
    zk_qap_check_result* d_res = (zk_qap_check_result*)st.res.p;
    unsigned long long* d_flag = (unsigned long long*)st.flag.p;
    const unsigned long long none = QC_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(d_flag, &none, sizeof(none), hipMemcpyHostToDevice, s));
    // range kernel: a block covers bx elements of by instances
    unsigned bx = 1;
    while (bx < QC_BLOCK && bx < a_len) bx *= 2;
    const unsigned by = QC_BLOCK / bx;
    const bool by_instance = ctx->opt_qap_check_by_instance != 0;
    const double row_bytes = 68.0 * (q.u_gate.nnz + q.v_gate.nnz + q.w_gate.nnz) + 12.0 * (n + 1);   // idx + val + the witness element; ptr
    for (size_t j0 = 0; j0 < count; j0 += chunk) {
        const size_t c = std::min(chunk, count - j0);
        const Fr* a = d_a ? d_a + j0 * stride : nullptr;
        ProfScope ps(ctx, "qap_check", (double)c * (row_bytes + 32.0 * a_len), s);
        hipLaunchKernelGGL(k_qc_init, dim3(ceil_div(c, QC_BLOCK)), dim3(QC_BLOCK), 0, s, a, stride, a_len, (uint32_t)c, d_res);
        ZK_HIP(hipGetLastError());
        if (a_len) {
            const unsigned gy = (unsigned)std::min<size_t>(ceil_div(c, by), 65535);
            hipLaunchKernelGGL(k_qc_range, dim3(ceil_div(a_len, bx), gy), dim3(bx, by), 0, s, a, stride, a_len, (uint32_t)c, j0, d_flag);
            ZK_HIP(hipGetLastError());
        }
        const unsigned grid = ceil_div(c * n, QC_BLOCK);
        if (by_instance)
            hipLaunchKernelGGL(k_qap_check<true>, dim3(grid), dim3(QC_BLOCK), 0, s, qc_view(q.u_gate), qc_view(q.v_gate), qc_view(q.w_gate), a,
                               stride, a_len, (uint32_t)n, (uint32_t)c, d_res);
        else
            hipLaunchKernelGGL(k_qap_check<false>, dim3(grid), dim3(QC_BLOCK), 0, s, qc_view(q.u_gate), qc_view(q.v_gate), qc_view(q.w_gate), a,
                               stride, a_len, (uint32_t)n, (uint32_t)c, d_res);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(out + j0, d_res, c * sizeof(zk_qap_check_result), hipMemcpyDeviceToHost, s));
    }
    unsigned long long bad = QC_NO_ERROR;
    ZK_HIP(hipMemcpyAsync(&bad, d_flag, sizeof(bad), hipMemcpyDeviceToHost, s));
    ZK_HIP(hipStreamSynchronize(s));
    ZK_REQUIRE(bad == QC_NO_ERROR, ZK_ERR_RANGE, "qap_check: weight >= r in instance " + std::to_string(bad));
}

static void qc_check_args(zk_ctx* ctx, const zk_qap& q) {
    ZK_REQUIRE(q.ctx == ctx, ZK_ERR_ARG, "qap_check: the QAP belongs to another context");
    ZK_REQUIRE(!q.dense, ZK_ERR_UNSUPPORTED,
               "qap_check: the dense form holds coefficients and t, not its roots, so no gate can be named (use zk_circuit_qap_sparse)");
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_qap_check(zk_ctx* ctx, const zk_qap* qap, const uint64_t* weights, size_t m, zk_qap_check_result* out) {
    if (!ctx || !qap || !out || (m && !weights)) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        qc_check_args(ctx, *qap);
        QapCheckState& st = qc_state(ctx);
        const size_t a_len = std::min(m, qap->m);   // zip truncates
        if (a_len) {
            st.grow(st.wit, a_len * sizeof(Fr));
            ZK_HIP(hipMemcpyAsync(st.wit.p, weights, a_len * sizeof(Fr), hipMemcpyHostToDevice, st.stream));
        }
        qc_run(ctx, st, *qap, a_len ? (const Fr*)st.wit.p : nullptr, a_len, a_len, 1, out);
        ctx->resolve_profile();
    });
}

int zk_qap_check_dev(zk_ctx* ctx, const zk_qap* qap, const void* d_weights, size_t m, size_t stride, size_t count, zk_qap_check_result* out) {
    if (!ctx || !qap) return ZK_ERR_ARG;
    if (count == 0) return ZK_OK;
    if (!out || (m && !d_weights) || stride < m) return ZK_ERR_ARG;
    return guarded(ctx, [&] {
        qc_check_args(ctx, *qap);
        QapCheckState& st = qc_state(ctx);
        qc_run(ctx, st, *qap, (const Fr*)d_weights, std::min(m, qap->m), stride, count, out);
        ctx->resolve_profile();
    });
}

}  // extern "C"
