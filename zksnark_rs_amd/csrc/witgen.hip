// witgen.hip -- zk_witgen_*: circuit::weights (circuit/mod.rs:529-637) for many input sets at once on the GPU.
//
// The program's tape (witgen_tape.hpp: single-assignment field operations over numbered slots, sorted by level) is uploaded once.
// k_witgen runs it with one INSTANCE per lane:
//   group      64 consecutive instances = one workgroup of W waves; lane l of every wave works on instance 64 g + l
//   scratch    the group's slot values in HBM, slot-major: value of slot s for lane l at (s * 64 + l), so one wave's access to a slot
//              is 2 KiB contiguous; slots * 64 * 32 bytes per group in flight
//   load       inputs range-checked (word pattern >= r: atomicMin of the instance index into a flag word), to Montgomery form, to
//              their slots -- strided over the W waves
//   evaluate   level by level; the operations of a level are independent and strided over the W waves, __syncthreads() between
//              levels when W > 1.  W = 1 (a chain) has one wave per group, program order, no barrier at all.  Either way a wave
//              requests the operands of its next operation before it computes the current one (witgen_run_ops)
//   store      slots 0..m-1 to canonical form, instance-major (what zk_prove_dev / zk_prove_batch_submit take per witness)
// Lanes behind `count` in the last group never return early: they take part in every barrier and are predicated off every load and
// store.  Groups run in chunks of as many as the scratch cap holds (option "witgen_scratch_kib"), so `count` is not bounded by memory.
#include "witgen_kernels.cuh"
#include "circuit.hpp"

struct zk_witgen {
    zk_ctx* ctx = nullptr;
    size_t n_in = 0, m = 0, slots = 0, levels = 0;
    unsigned waves = 1;
    size_t scratch_cap = 0;                 // bytes
    zk::DevBuf<zk::TapeOp> ops;
    zk::DevBuf<uint32_t> level_ptr, in_slot;
    zk::DevBuf<zk::Fr> consts, scratch;
    zk::DevBuf<unsigned long long> flag;
    std::vector<uint32_t> h_in_bit;         // a built circuit's bit inputs (Tape::in_bit); empty for a parsed program
    zk::DevBuf<uint32_t> in_bit;
};

namespace zk {

// an operand of the whole-circuit tape: a pooled constant or a slot of the lane's scratch (run: witgen_kernels.cuh)
struct WitgenFetch {
    const Fr* __restrict__ consts;
    const Fr* sc;
    __device__ __forceinline__ bool is_slot(uint32_t x) const { return !(x & TAPE_CONST); }
    __device__ __forceinline__ Fr operator()(uint32_t x) const { return (x & TAPE_CONST) ? consts[x & ~TAPE_CONST] : sc[(size_t)x * WG_LANES]; }
};

__global__ void __launch_bounds__(WG_LANES * WG_MAX_WAVES)
k_witgen(const TapeOp* __restrict__ ops, const uint32_t* __restrict__ level_ptr, unsigned levels, const uint32_t* __restrict__ in_slot,
         const Fr* __restrict__ consts, const uint64_t* __restrict__ inputs, unsigned n_in, unsigned m, size_t slots, size_t first, size_t count,
         Fr* __restrict__ scratch, uint64_t* __restrict__ out, unsigned long long* __restrict__ flag) {
    const unsigned lane = threadIdx.x & (WG_LANES - 1), wave = threadIdx.x / WG_LANES, W = blockDim.x / WG_LANES;
    const size_t j = first + (size_t)blockIdx.x * WG_LANES + lane;      // instance
    const bool live = j < count;
    Fr* sc = scratch + (size_t)blockIdx.x * slots * WG_LANES + lane;    // slot s of this lane: sc[s * 64]

    if (live) {
        if (wave == 0) sc[0] = Fr::one();
        const uint64_t* in = inputs + j * (size_t)n_in * 4;
        for (unsigned i = wave; i < n_in; i += W) {
            Fr x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t w = in[4 * (size_t)i + k];
                x.l[2 * k] = (uint32_t)w;
                x.l[2 * k + 1] = (uint32_t)(w >> 32);
            }
            if (!x.raw_in_range()) atomicMin(flag, (unsigned long long)j);
            sc[(size_t)in_slot[i] * WG_LANES] = Fr::from_canonical(x);
        }
    }
    if (W > 1) __syncthreads();

    const WitgenFetch fetch{consts, sc};
    if (W == 1) {                       // one wave, program order: the whole tape as one run, no barrier
        if (live) witgen_run_ops(ops, 0, level_ptr[levels], 1, sc, fetch);
    } else {
        for (unsigned l = 0; l < levels; ++l) {
            if (live) witgen_run_ops(ops, level_ptr[l] + wave, level_ptr[l + 1], W, sc, fetch);
            __syncthreads();
        }
    }

    if (live) {
        uint64_t* o = out + j * (size_t)m * 4;
        for (unsigned i = wave; i < m; i += W) {
            const Fr x = sc[(size_t)i * WG_LANES].to_canonical();
#pragma unroll
            for (int k = 0; k < 4; ++k) o[4 * (size_t)i + k] = (uint64_t)x.l[2 * k] | ((uint64_t)x.l[2 * k + 1] << 32);
        }
    }
}

// A built circuit's bit inputs: any value other than 0 or 1 records the lowest (instance * n_in + input).  A pass of its own in front
// of k_witgen, launched only for circuits that have such inputs.
__global__ void __launch_bounds__(256)
k_witgen_bits(const uint64_t* __restrict__ inputs, const uint32_t* __restrict__ in_bit, unsigned n_in, size_t count, unsigned long long* __restrict__ flag) {
    const size_t total = count * (size_t)n_in;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        if (!in_bit[idx % n_in]) continue;
        const uint64_t* x = inputs + 4 * idx;
        if (x[0] > 1 || x[1] || x[2] || x[3]) atomicMin(flag, (unsigned long long)idx);
    }
}

static zk_witgen* witgen_create(zk_ctx* ctx, const Tape& t) {
    ZK_REQUIRE(!t.status, t.status, t.error);
    ZK_REQUIRE(t.n_in < (1u << 31) && t.m < (1u << 31), ZK_ERR_SIZE, "witgen: program too large");
    std::unique_ptr<zk_witgen> w(new zk_witgen());
    w->ctx = ctx;
    w->n_in = t.n_in; w->m = t.m; w->slots = t.slots; w->levels = t.levels();
    w->waves = witgen_waves(t);
    w->scratch_cap = (size_t)std::max<long>(ctx->opt_witgen_scratch_kib, 0) * 1024;
    hipStream_t st = ctx->stream;
    auto up = [&](auto& buf, const auto& host) {
        buf.alloc(std::max<size_t>(host.size(), 1));   // never a null array
        if (!host.empty()) ZK_HIP(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, st));
    };
    up(w->ops, t.ops);
    up(w->in_slot, t.in_slot);
    up(w->consts, t.consts);
    const std::vector<uint32_t> lp = t.level_ptr.empty() ? std::vector<uint32_t>{0} : t.level_ptr;
    up(w->level_ptr, lp);
    w->flag.alloc(2);
    w->h_in_bit = t.in_bit;
    if (!t.in_bit.empty()) up(w->in_bit, t.in_bit);
    ZK_HIP(hipStreamSynchronize(st));   // the host vectors may go away with the circuit
    return w.release();
}

static void witgen_run(zk_witgen& w, const void* d_inputs, size_t count, void* d_out) {
    zk_ctx* ctx = w.ctx;
    hipStream_t st = ctx->stream;
    const size_t group_bytes = w.slots * WG_LANES * sizeof(Fr);
    const size_t groups = (count + WG_LANES - 1) / WG_LANES;
    const size_t fit = w.scratch_cap / group_bytes;
    ZK_REQUIRE(fit >= 1, ZK_ERR_SIZE, "witgen: one group of 64 instances needs " + std::to_string(group_bytes >> 10) +
                                          " KiB of scratch, more than the option witgen_scratch_kib allows");
    const size_t chunk = std::min(std::min(groups, fit), (size_t)1 << 30);
    w.scratch.ensure(chunk * w.slots * WG_LANES);
    const unsigned long long none[2] = {WG_NO_ERROR, WG_NO_ERROR};
    ZK_HIP(hipMemcpyAsync(w.flag.p, none, sizeof(none), hipMemcpyHostToDevice, st));
    if (!w.h_in_bit.empty()) {
        const size_t total = count * w.n_in;
        hipLaunchKernelGGL(k_witgen_bits, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65536)), dim3(256), 0, st, (const uint64_t*)d_inputs,
                           w.in_bit.p, (unsigned)w.n_in, count, w.flag.p + 1);
        ZK_HIP(hipGetLastError());
    }
    for (size_t g0 = 0; g0 < groups; g0 += chunk) {      // same stream: a chunk starts when the one before has left the scratch
        const size_t g = std::min(chunk, groups - g0);
        ProfScope ps(ctx, "witgen", 0.0);
        hipLaunchKernelGGL(k_witgen, dim3((unsigned)g), dim3(WG_LANES * w.waves), 0, st, w.ops.p, w.level_ptr.p, (unsigned)w.levels, w.in_slot.p,
                           w.consts.p, (const uint64_t*)d_inputs, (unsigned)w.n_in, (unsigned)w.m, w.slots, g0 * WG_LANES, count, w.scratch.p,
                           (uint64_t*)d_out, w.flag.p);
        ZK_HIP(hipGetLastError());
    }
    unsigned long long bad[2] = {WG_NO_ERROR, WG_NO_ERROR};
    ZK_HIP(hipMemcpyAsync(bad, w.flag.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    ZK_REQUIRE(bad[0] == WG_NO_ERROR, ZK_ERR_RANGE, "witgen: input value >= r in instance " + std::to_string(bad[0]));
    ZK_REQUIRE(bad[1] == WG_NO_ERROR, ZK_ERR_RANGE,
               "witgen: " + bit_input_error(bad[1] / w.n_in, bad[1] % w.n_in, w.h_in_bit[bad[1] % w.n_in] - 1));
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_witgen_create(zk_ctx* ctx, const zk_circuit* c, zk_witgen** out) {
    if (!ctx || !c || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return guarded(ctx, [&] { *out = witgen_create(ctx, zk_circuit_tape(c)); });
}
void zk_witgen_free(zk_witgen* w) {
    if (!w) return;
    (void)hipSetDevice(w->ctx->device);
    delete w;
}
int zk_witgen_run(zk_witgen* w, const void* d_inputs, size_t n_in, size_t count, void* d_weights_out, size_t m) {
    if (!w) return ZK_ERR_ARG;
    return guarded(w->ctx, [&] {
        ZK_REQUIRE(n_in == w->n_in, ZK_ERR_ARG, "StructureErr(None, Wrong number of values supplied)");
        ZK_REQUIRE(m == w->m, ZK_ERR_ARG, "StructureErr(None, weights buffer size mismatch)");
        if (count == 0) return;
        ZK_REQUIRE(d_weights_out && (d_inputs || !n_in), ZK_ERR_ARG, "witgen: null device pointer");
        witgen_run(*w, d_inputs, count, d_weights_out);
    });
}

}  // extern "C"
