// tests/cpp/point_forms_check.hip -- every point-addition form of the MSMs (lazy29.cuh, quad29.cuh, fold_park.cuh, madd_asm.inc) run on
// raw limb vectors: tests/test_gpu_point_forms.py writes the operands, this program calls the product's own functions and dumps the
// raw limbs of every output coordinate.  No formula lives here.
//   point_forms_check REQUEST RESULT          every section on the GPU
//   point_forms_check --host REQUEST RESULT   the one-lane ZK_HD forms of the job sections on the CPU (no GPU is touched)
// Built by the test with the library's CXXFLAGS (csrc/Makefile) and -I zksnark_rs_amd/csrc.
//
// Files are little-endian int32.  Request: header {MAGIC, nj1, nj2, nasm, c1 lanes, c1 T, c1 steps, c2 lanes, c2 T, c2 steps,
// fold lanes, fold T, fold steps}, then the sections in that order.  Result: the sections' outputs in the same order.
//   job      {form, flags (1: A.inf, 2: B.inf), k, 0, A.X, A.Y, A.ZZ, A.ZZZ, B.X, B.Y, B.ZZ, B.ZZZ}, 18 limbs a coordinate (G1: the first 9;
//            Jacobian forms: Z in the ZZ slot; affine operands: B.X, B.Y)
//   job out  4 lanes x {status, inf, 0, 0, X, Y, ZZ, ZZZ}: the four lanes of a quad run the same job (a quad form needs them, a one-lane
//            form simply runs four times)
//   asm lane {active, mode (0 even, 1 odd, 2 even then odd), X, Y, ZZ, ZZZ, qx, qy, qx2, qy2}, 9 limbs each
//   asm out  {same_x lo, hi, same_point lo, hi of the first body, the same of the second, X, Y, ZZ, ZZZ after the first body, after the second}
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>
#include "quad29.cuh"
#include "fold_park.cuh"
using namespace zk;

typedef FpR<FqParams> L1;
typedef Fp2R<FqParams> L2;
enum { MAGIC = 0x50464331, JOB_IN = 4 + 8 * 18, JOB_OUT = 4 + 4 * 18, ASM_IN = 2 + 8 * 9, ASM_OUT = 8 + 8 * 9, NOT_RUN = -99 };
enum Form { MADD = 0, MADD_NZ, MADD_SECOND, ADD, DBL, ADD_FROM, ADD_PARKED, DBL_JAC, ADD_JAC, MADD_JAC, MUL_SMALL_JAC, QUAD_ADD, QUAD_DBL, QUAD_MUL_SMALL };

ZK_HD void ld(L1& x, const int32_t* s) { for (int i = 0; i < 9; ++i) x.v[i] = s[i]; }
ZK_HD void ld(L2& x, const int32_t* s) { ld(x.c0, s); ld(x.c1, s + 9); }
ZK_HD void st(int32_t* d, const L1& x) { for (int i = 0; i < 9; ++i) d[i] = x.v[i]; }
ZK_HD void st(int32_t* d, const L2& x) { st(d, x.c0); st(d + 9, x.c1); }
template <class L> ZK_HD XyzzR<L> ld_xyzz(const int32_t* s, bool inf) {
    XyzzR<L> p;
    ld(p.X, s); ld(p.Y, s + 18); ld(p.ZZ, s + 36); ld(p.ZZZ, s + 54);
    p.inf = inf;
    return p;
}
template <class L> ZK_HD void st_xyzz(int32_t* o, int status, const XyzzR<L>& p) {
    o[0] = status; o[1] = p.inf;
    st(o + 4, p.X); st(o + 22, p.Y); st(o + 40, p.ZZ); st(o + 58, p.ZZZ);
}
template <class L> ZK_HD JacR<typename L::Elem> ld_jac(const int32_t* s, bool inf) {
    JacR<typename L::Elem> p;
    ld(p.X, s); ld(p.Y, s + 18); ld(p.Z, s + 36);
    p.inf = inf;
    return p;
}
template <class F> ZK_HD void st_jac(int32_t* o, int status, const JacR<F>& p) {
    o[0] = status; o[1] = p.inf;
    st(o + 4, p.X); st(o + 22, p.Y); st(o + 40, p.Z);
}

// the forms that are ZK_HD: the same code path on the host and on the device
template <class L> ZK_HD bool one_lane_form(const int32_t* j, int32_t* o) {
    typedef typename L::Elem F;
    const int form = j[0];
    const bool ainf = j[1] & 1, binf = j[1] & 2;
    const uint32_t k = (uint32_t)j[2];
    const int32_t *A = j + 4, *B = j + 4 + 72;
    L qx, qy;
    ld(qx, B); ld(qy, B + 18);
    switch (form) {
    case MADD: { XyzzR<L> p = ld_xyzz<L>(A, ainf); const bool ok = madd_xyzz(p, qx, qy); st_xyzz(o, ok, p); return true; }
    case MADD_NZ: { XyzzR<L> p = ld_xyzz<L>(A, false); const int s = madd_xyzz_nz(p, qx, qy); st_xyzz(o, s, p); return true; }
    case MADD_SECOND: { XyzzR<L> p = ld_xyzz<L>(A, false); const int s = madd_xyzz_second(p, qx, qy); st_xyzz(o, s, p); return true; }
    case ADD: { const XyzzR<L> r = add_xyzz(ld_xyzz<L>(A, ainf), ld_xyzz<L>(B, binf)); st_xyzz(o, 0, r); return true; }
    case DBL: { XyzzR<L> p = ld_xyzz<L>(A, ainf); dbl_xyzz(p); st_xyzz(o, 0, p); return true; }
    case DBL_JAC: { st_jac(o, 0, dbl_lazy(ld_jac<L>(A, ainf))); return true; }
    case ADD_JAC: { st_jac(o, 0, add_lazy(ld_jac<L>(A, ainf), ld_jac<L>(B, binf))); return true; }
    case MADD_JAC: { JacR<F> p = ld_jac<L>(A, ainf); const bool ok = madd_lazy(p, qx, qy); st_jac(o, ok, p); return true; }
    case MUL_SMALL_JAC: { st_jac(o, 0, mul_small_lazy(ld_jac<L>(A, ainf), k)); return true; }
    }
    return false;
}

__device__ __forceinline__ void parked_form(const int32_t* j, int32_t* o, FoldPark* pk) {
    XyzzR<L2> p = ld_xyzz<L2>(j + 4, j[1] & 1);
    const XyzzR<L2> q = ld_xyzz<L2>(j + 4 + 72, j[1] & 2);
    bool inf = p.inf;
    fpark_put(pk, 0, p.Y); fpark_put(pk, 1, p.ZZ); fpark_put(pk, 2, p.ZZZ);
    add_xyzz_from_parked(p.X, inf, pk, &q);
    p.Y = fpark_get(pk, 0); p.ZZ = fpark_get(pk, 1); p.ZZZ = fpark_get(pk, 2); p.inf = inf;
    st_xyzz(o, 0, p);
}

// one job per quad: lane `role` of the quad writes its own copy of the result
template <class L>
__global__ __launch_bounds__(TAIL_THREADS) void k_jobs(const int32_t* __restrict__ req, int n, int32_t* __restrict__ res) {
    __shared__ FoldPark pk;
    const int t = blockIdx.x * blockDim.x + threadIdx.x, job = t >> 2, role = t & 3;
    if (job >= n) return;
    const int32_t* j = req + (size_t)job * JOB_IN;
    int32_t* o = res + ((size_t)job * 4 + role) * JOB_OUT;
    if (one_lane_form<L>(j, o)) return;
    const bool ainf = j[1] & 1, binf = j[1] & 2;
    const int32_t *A = j + 4, *B = j + 4 + 72;
    switch (j[0]) {
    case ADD_FROM: { XyzzR<L> p = ld_xyzz<L>(A, ainf); const XyzzR<L> q = ld_xyzz<L>(B, binf); add_xyzz_from(p, &q); st_xyzz(o, 0, p); break; }
    case ADD_PARKED:
        if constexpr (std::is_same<L, L2>::value) parked_form(j, o, &pk); else o[0] = NOT_RUN;   // the G2 fold only
        break;
    case QUAD_ADD: st_xyzz(o, 0, quad_add_xyzz(ld_xyzz<L>(A, ainf), ld_xyzz<L>(B, binf), role)); break;
    case QUAD_DBL: st_xyzz(o, 0, quad_dbl_xyzz(ld_xyzz<L>(A, ainf), role)); break;
    case QUAD_MUL_SMALL: st_xyzz(o, 0, quad_mul_small_xyzz(ld_xyzz<L>(A, ainf), (uint32_t)j[2], role)); break;
    default: o[0] = NOT_RUN;
    }
}

// the two generated bodies as a wave: one lane per request, lanes with active == 0 sit the bodies out as lanes past `kf` do in
// k_msm_accumulate
__global__ __launch_bounds__(64) void k_asm(const int32_t* __restrict__ req, int n, int32_t* __restrict__ res) {
#if ZK_MONT_ASM_ON
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int32_t* j = req + (size_t)t * ASM_IN;
    int32_t* o = res + (size_t)t * ASM_OUT;
    const int mode = j[1];
    L1 X, Y, ZZ, ZZZ, qx, qy, xb;
    ld(X, j + 2); ld(Y, j + 11); ld(ZZ, j + 20); ld(ZZZ, j + 29); ld(qx, j + 38); ld(qy, j + 47);
    if (j[0]) {
        uint64_t sx, sp;
        if (mode == 1) madd_asm_g1_odd<FqParams>(X.v, Y.v, ZZ.v, ZZZ.v, qx.v, qy.v, xb.v, sx, sp);
        else madd_asm_g1_even<FqParams>(X.v, Y.v, ZZ.v, ZZZ.v, qx.v, qy.v, xb.v, sx, sp);
        o[0] = (int32_t)sx; o[1] = (int32_t)(sx >> 32); o[2] = (int32_t)sp; o[3] = (int32_t)(sp >> 32);
        st(o + 8, xb); st(o + 17, Y); st(o + 26, ZZ); st(o + 35, ZZZ);
        if (mode == 2 && !((sx >> (threadIdx.x & 63)) & 1)) {   // a lane with the same x is done, as `kf = k + 1` ends it in the loop
            ld(qx, j + 56); ld(qy, j + 65);
            madd_asm_g1_odd<FqParams>(xb.v, Y.v, ZZ.v, ZZZ.v, qx.v, qy.v, X.v, sx, sp);
            o[4] = (int32_t)sx; o[5] = (int32_t)(sx >> 32); o[6] = (int32_t)sp; o[7] = (int32_t)(sp >> 32);
            st(o + 44, X); st(o + 53, Y); st(o + 62, ZZ); st(o + 71, ZZZ);
        }
    }
#endif
}

// point of step s for lane l out of a table of T
__host__ __device__ inline int chain_index(int lane, int step, int T) { return (lane * 5 + step * (2 * lane + 1)) % T; }

// G1 chain: even and odd body in turn on the same registers, as the accumulation loop runs them; every state is dumped
// out: per lane and step {X, Y register, ZZ, ZZZ, same_x bit, same_point bit} (38)
__global__ __launch_bounds__(64) void k_chain_g1(const int32_t* __restrict__ table, int T, const int32_t* __restrict__ start, int lanes, int steps, int32_t* __restrict__ res) {
#if ZK_MONT_ASM_ON
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    L1 X, Y, ZZ, ZZZ, xb;
    ld(X, start + t * 36); ld(Y, start + t * 36 + 9); ld(ZZ, start + t * 36 + 18); ld(ZZZ, start + t * 36 + 27);
    int32_t* o = res + (size_t)t * steps * 38;
    for (int s = 0; s < steps; ++s, o += 38) {
        const int32_t* pt = table + chain_index(t, s, T) * 18;
        L1 qx, qy;
        ld(qx, pt); ld(qy, pt + 9);
        uint64_t sx, sp;
        if (s & 1) {
            madd_asm_g1_odd<FqParams>(xb.v, Y.v, ZZ.v, ZZZ.v, qx.v, qy.v, X.v, sx, sp);
            st(o, X);
        } else {
            madd_asm_g1_even<FqParams>(X.v, Y.v, ZZ.v, ZZZ.v, qx.v, qy.v, xb.v, sx, sp);
            st(o, xb);
        }
        st(o + 9, Y); st(o + 18, ZZ); st(o + 27, ZZZ);
        o[36] = (int32_t)((sx >> (threadIdx.x & 63)) & 1); o[37] = (int32_t)((sp >> (threadIdx.x & 63)) & 1);
    }
#endif
}

// G2 chain: madd_xyzz_nz; out: per lane and step {X, Y, ZZ, ZZZ, status} (73)
__global__ __launch_bounds__(64) void k_chain_g2(const int32_t* __restrict__ table, int T, const int32_t* __restrict__ start, int lanes, int steps, int32_t* __restrict__ res) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    XyzzR<L2> p;
    ld(p.X, start + t * 72); ld(p.Y, start + t * 72 + 18); ld(p.ZZ, start + t * 72 + 36); ld(p.ZZZ, start + t * 72 + 54);
    p.inf = false;
    int32_t* o = res + (size_t)t * steps * 73;
    for (int s = 0; s < steps; ++s, o += 73) {
        const int32_t* pt = table + chain_index(t, s, T) * 36;
        L2 qx, qy;
        ld(qx, pt); ld(qy, pt + 18);
        const int status = madd_xyzz_nz(p, qx, qy);
        st(o, p.X); st(o + 18, p.Y); st(o + 36, p.ZZ); st(o + 54, p.ZZZ);
        o[72] = status;
    }
}

// the fold: successive add_xyzz_from_parked from images in global memory; table / start entries {X, Y, ZZ, ZZZ, inf} (73), out the same
__global__ __launch_bounds__(TAIL_THREADS) void k_chain_fold(const int32_t* __restrict__ table, int T, const int32_t* __restrict__ start, int lanes, int steps, XyzzR<L2>* __restrict__ img,
                                                             int32_t* __restrict__ res) {
    __shared__ FoldPark pk;
    const int t = threadIdx.x;
    for (int i = t; i < T; i += TAIL_THREADS) img[i] = ld_xyzz<L2>(table + i * 73, table[i * 73 + 72] != 0);
    __syncthreads();
    if (t >= lanes) return;
    L2 X;
    ld(X, start + t * 73);
    { L2 c; ld(c, start + t * 73 + 18); fpark_put(&pk, 0, c); ld(c, start + t * 73 + 36); fpark_put(&pk, 1, c); ld(c, start + t * 73 + 54); fpark_put(&pk, 2, c); }
    bool inf = start[t * 73 + 72] != 0;
    int32_t* o = res + (size_t)t * steps * 73;
    for (int s = 0; s < steps; ++s, o += 73) {
        add_xyzz_from_parked(X, inf, &pk, &img[chain_index(t, s, T)]);
        st(o, X); st(o + 18, fpark_get(&pk, 0)); st(o + 36, fpark_get(&pk, 1)); st(o + 54, fpark_get(&pk, 2));
        o[72] = inf;
    }
}

static void die(const char* what, hipError_t e) {
    fprintf(stderr, "point_forms_check: %s: %s\n", what, hipGetErrorString(e));
    exit(2);
}
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) die(#x, e_); } while (0)
static void after_launch(const char* name) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) die(name, e);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) die(name, e);
}
static int32_t* to_device(const int32_t* h, size_t n) {
    int32_t* d = nullptr;
    HIP_OK(hipMalloc(&d, (n ? n : 1) * sizeof(int32_t)));
    if (n) HIP_OK(hipMemcpy(d, h, n * sizeof(int32_t), hipMemcpyHostToDevice));
    return d;
}
static int32_t* device_out(size_t n) {
    int32_t* d = nullptr;
    HIP_OK(hipMalloc(&d, (n ? n : 1) * sizeof(int32_t)));
    HIP_OK(hipMemset(d, 0, (n ? n : 1) * sizeof(int32_t)));
    return d;
}
static void fetch(std::vector<int32_t>& out, const int32_t* d, size_t n) {
    const size_t at = out.size();
    out.resize(at + n);
    if (n) HIP_OK(hipMemcpy(out.data() + at, d, n * sizeof(int32_t), hipMemcpyDeviceToHost));
}

int main(int argc, char** argv) {
    const bool host = argc == 4 && !strcmp(argv[1], "--host");
    if (argc != 3 && !host) { fprintf(stderr, "usage: point_forms_check [--host] REQUEST RESULT\n"); return 1; }
    FILE* f = fopen(argv[argc - 2], "rb");
    if (!f) { perror("request"); return 1; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<int32_t> req(bytes / 4);
    if (fread(req.data(), 4, req.size(), f) != req.size()) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);
    if (req.size() < 13 || req[0] != MAGIC) { fprintf(stderr, "not a request file\n"); return 1; }
    const int nj1 = req[1], nj2 = req[2], nasm = req[3], c1l = req[4], c1t = req[5], c1s = req[6], c2l = req[7], c2t = req[8], c2s = req[9], fl = req[10], ft = req[11], fs = req[12];
    for (int i = 1; i < 13; ++i) if (req[i] < 0 || req[i] > (1 << 20)) { fprintf(stderr, "bad header\n"); return 1; }
    if (nasm % 64 || c1l > 64 || c2l > 64 || fl > TAIL_THREADS) { fprintf(stderr, "bad header\n"); return 1; }
    const size_t o_j1 = 13, o_j2 = o_j1 + (size_t)nj1 * JOB_IN, o_asm = o_j2 + (size_t)nj2 * JOB_IN, o_c1 = o_asm + (size_t)nasm * ASM_IN,
                 o_c2 = o_c1 + (size_t)c1t * 18 + (size_t)c1l * 36, o_f = o_c2 + (size_t)c2t * 36 + (size_t)c2l * 72, end = o_f + (size_t)ft * 73 + (size_t)fl * 73;
    if (req.size() != end) { fprintf(stderr, "request is %zu words, header says %zu\n", req.size(), end); return 1; }
    if ((c1l && !c1t) || (c2l && !c2t) || (fl && !ft)) { fprintf(stderr, "chain without a table\n"); return 1; }
    std::vector<int32_t> out;
    if (host) {
        out.assign(((size_t)nj1 + nj2) * 4 * JOB_OUT, 0);
        for (int i = 0; i < nj1 + nj2; ++i) {
            const int32_t* j = req.data() + o_j1 + (size_t)i * JOB_IN;
            int32_t* o = out.data() + (size_t)i * 4 * JOB_OUT;
            const bool ran = i < nj1 ? one_lane_form<L1>(j, o) : one_lane_form<L2>(j, o);
            if (!ran) o[0] = NOT_RUN;
            for (int r = 1; r < 4; ++r) memcpy(o + r * JOB_OUT, o, JOB_OUT * sizeof(int32_t));
        }
    } else {
        int32_t* d;
        int32_t* r;
        if (nj1) {
            d = to_device(req.data() + o_j1, (size_t)nj1 * JOB_IN); r = device_out((size_t)nj1 * 4 * JOB_OUT);
            hipLaunchKernelGGL(k_jobs<L1>, dim3((nj1 * 4 + TAIL_THREADS - 1) / TAIL_THREADS), dim3(TAIL_THREADS), 0, 0, d, nj1, r);
            after_launch("k_jobs<G1>");
            fetch(out, r, (size_t)nj1 * 4 * JOB_OUT);
        }
        if (nj2) {
            d = to_device(req.data() + o_j2, (size_t)nj2 * JOB_IN); r = device_out((size_t)nj2 * 4 * JOB_OUT);
            hipLaunchKernelGGL(k_jobs<L2>, dim3((nj2 * 4 + TAIL_THREADS - 1) / TAIL_THREADS), dim3(TAIL_THREADS), 0, 0, d, nj2, r);
            after_launch("k_jobs<G2>");
            fetch(out, r, (size_t)nj2 * 4 * JOB_OUT);
        }
        if (nasm) {
            d = to_device(req.data() + o_asm, (size_t)nasm * ASM_IN); r = device_out((size_t)nasm * ASM_OUT);
            hipLaunchKernelGGL(k_asm, dim3(nasm / 64), dim3(64), 0, 0, d, nasm, r);
            after_launch("k_asm");
            fetch(out, r, (size_t)nasm * ASM_OUT);
        }
        if (c1l) {
            d = to_device(req.data() + o_c1, (size_t)c1t * 18 + (size_t)c1l * 36); r = device_out((size_t)c1l * c1s * 38);
            hipLaunchKernelGGL(k_chain_g1, dim3(1), dim3(64), 0, 0, d, c1t, d + (size_t)c1t * 18, c1l, c1s, r);
            after_launch("k_chain_g1");
            fetch(out, r, (size_t)c1l * c1s * 38);
        }
        if (c2l) {
            d = to_device(req.data() + o_c2, (size_t)c2t * 36 + (size_t)c2l * 72); r = device_out((size_t)c2l * c2s * 73);
            hipLaunchKernelGGL(k_chain_g2, dim3(1), dim3(64), 0, 0, d, c2t, d + (size_t)c2t * 36, c2l, c2s, r);
            after_launch("k_chain_g2");
            fetch(out, r, (size_t)c2l * c2s * 73);
        }
        if (fl) {
            d = to_device(req.data() + o_f, (size_t)ft * 73 + (size_t)fl * 73); r = device_out((size_t)fl * fs * 73);
            XyzzR<L2>* img = nullptr;
            HIP_OK(hipMalloc(&img, (size_t)ft * sizeof(XyzzR<L2>)));
            hipLaunchKernelGGL(k_chain_fold, dim3(1), dim3(TAIL_THREADS), 0, 0, d, ft, d + (size_t)ft * 73, fl, fs, img, r);
            after_launch("k_chain_fold");
            fetch(out, r, (size_t)fl * fs * 73);
        }
    }
    f = fopen(argv[argc - 1], "wb");
    if (!f) { perror("result"); return 1; }
    if (fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) { fprintf(stderr, "short write\n"); return 1; }
    printf("point_forms_check: %d + %d jobs, %d asm lanes, chains %d x %d, %d x %d, %d x %d (%s)\n", nj1, nj2, nasm, c1l, c1s, c2l, c2s, fl, fs, host ? "host" : "device");
    return 0;
}
