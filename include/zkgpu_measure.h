/* zkgpu_measure.h -- measurement and test entry points of libzkgpu.so, kept OUT of the product ABI (include/zkgpu.h).
 *
 * Nothing here replaces an interface of the reference (/root/reference has no profiling and no tuning knobs): these are the hooks of
 * bench.py (HIP-event timing of the library's own kernels for the `roofline` object), of tools/ (same-box A/B switches) and of
 * tests/test_lazy29.py (the lazy radix at its limb extremes) and of tests/test_msm_plan.py (the record of what every inner product
 * decided from its size).  The product library exports the three zk_profile_* functions and zk_lazy29_batch and answers the
 * "msm_plan" keys of zk_get_option / zk_set_option described at the end of this file; the tuning KEYS below are accepted only by a library built with -DZK_MEASURE (make -C zksnark_rs_amd/csrc measure;
 * zk_get_option(ctx, "measure_build") == 1) -- the product build answers ZK_ERR_UNSUPPORTED to them.
 *
 * Keys of zk_set_option in a ZK_MEASURE build (defaults are what the product build has compiled in):
 *   "profile"            0 off, 1 event-time the bucket accumulations, 2 every launch group (also accepted by the product build: bench.py)
 *   "serialize"          1: every kernel of a proof on one stream (stand-alone kernel durations)
 *   "ablate"             bit 0: reuse the previous sorted list of a workspace (repeated inputs only; prices the sort)
 *   "msm_fold"           images summed per lane and pass in the row / column sums of the MSM tail (4)
 *   "msm_run_entries"    longest run of the accumulation when buckets are cut into several runs (32)
 *   "msm_run_whole"      products with at most this many entries per bucket keep every bucket in ONE run (128)
 *   "msm_run_fill"       runs as long as one round of accumulation lanes allows (1)
 *   "msm_small_lanes", "msm_unchain_lanes"   thresholds of the small-product forms (65536, 140000)
 *   "chain_order"        order of a proof's accumulation chain (1 = A, B2, L + H)
 *   "alt_stream", "tail_stream"   the merged L + H product or its reduction tail on the idle L stream (0; profiles/r5_experiments.txt 8, 11)
 *   "ntt_fuse"           element-wise kernels folded into the DIF tile loads / stores (1)
 *   "apply_cu_reserve"   mask the inner-product streams now (tools/rccl_starvation.py)
 */
#ifndef ZKGPU_MEASURE_H
#define ZKGPU_MEASURE_H
#include "zkgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Profiling: HIP-event timing of the library's own kernels on the stream they run on.
 * ---------------------------------------------------------------------------------------- */
int zk_profile_reset(zk_ctx* ctx);
/* n_names = number of distinct kernels recorded; name(i) / stats(i) enumerate them */
int zk_profile_count(const zk_ctx* ctx);
int zk_profile_entry(const zk_ctx* ctx, int i, const char** name, double* total_ms, uint64_t* launches, double* algo_bytes);


/* The lazy radix-2^29 form of the same field arithmetic (what `Fr * Fr`, fr.rs:44-48, and bn's Fq multiply become inside
 * the bucket accumulation and the NTT tiles: csrc/lazy29.cuh, csrc/ntt.hip) on caller-supplied limb patterns, so that the
 * bounds the kernels rely on can be tested at their extremes.  Every operand is 9 signed 32-bit limbs per element, value =
 * sum v[k] 2^(29 k) (not reduced).  field: 0 = Fr, 1 = Fq.  out: canonical residues (4 words each) of the result;
 * raw_out (may be null): the result's 9 limbs before the final reduction.
 *   ZK_LAZY_MONT       a b 2^-261          (|a limbs| <= 2^30, |b limbs| < 2^29)
 *   ZK_LAZY_SQR        a a 2^-261          (|limbs| < 2^29)
 *   ZK_LAZY_MONT_DIFF  (a b - c d) 2^-261  (all |limbs| < 2^29)
 *   ZK_LAZY_NORM       a after carry propagation; ZK_LAZY_STORE  a itself        (|value| < 8 p)
 *   ZK_LAZY_FR_REDUCE  fr_reduce(a) of the NTT tiles (|value| < 2^9 r); ZK_LAZY_FR_STORE  fr_store_exact(a)   (Fr only)
 * The Fq2 multiplier of the G2 accumulation and the G2 tails (Fq only, field 1): one element = two Fq components, each 9 limbs as
 * above (components with |limbs| < 2^29 and |value| < 8 q).  out holds 2 n residues, c0 then c1 of each element (8 words per
 * element); raw_out 18 limbs per element, c0's 9 then c1's 9.
 *   ZK_LAZY_FP2_MUL    (a + b i)(c + d i) 2^-261 = (a c - b d) 2^-261 + (a d + b c) 2^-261 i   (Fp2R::operator*)
 *   ZK_LAZY_FP2_SQR    (a + b i)^2 2^-261                                                   (Fp2R::sqr; operands a, b)
 * The scalar preparation of zk_g1_scale_batch / zk_crs_contribute (csrc/crs_contribution.hip: the GLV split and the width-4
 * non-adjacent forms, host code) is reached through the same entry point, so that the test hook adds no symbol: HOST code, ctx may be
 * NULL, field / b / c / d ignored.
 *   ZK_LAZY_GLV_RECODE a: n scalars below r as eight 32-bit words each (little-endian); out: 4 words per scalar, |k1| (2 words) then
 *                      |k2| (2 words), k = k1 + k2 lambda mod r; raw_out: ZK_GLV_RECODE_WORDS per scalar: k1 < 0, k2 < 0, the top
 *                      digit position (-1 for k = 0), then ZK_GLV_RECODE_DIGITS signed digits of k1 and as many of k2 (position i
 *                      weighs 2^i; the half's sign is folded into its digits) */
/* The scalar side of k_mul_each (csrc/mul_each_recode.hpp: the split with nearest rounding and the REGULAR signed fixed-window
 * recoding every lane does for its own scalar; the same functions compiled for the host), likewise: HOST code, ctx may be NULL,
 * b / c / d ignored; field selects the group whose window width W is used (0 = G1, 1 = G2).
 *   ZK_LAZY_REGULAR_RECODE a, out: as ZK_LAZY_GLV_RECODE; raw_out: ZK_REGULAR_RECODE_WORDS per scalar: k1 < 0, k2 < 0, |k1| even,
 *                      |k2| even (the half was recoded as its magnitude + 1), the digit count ND, then ZK_REGULAR_RECODE_DIGITS slots
 *                      for the digits of k1 and as many for k2, of which the first ND are used (position i weighs 2^(W i); every
 *                      digit odd, |digit| < 2^W; they recompose to the MAGNITUDE, plus one where it is even -- the sign is separate) */
enum { ZK_LAZY_MONT = 0, ZK_LAZY_SQR = 1, ZK_LAZY_MONT_DIFF = 2, ZK_LAZY_NORM = 3, ZK_LAZY_STORE = 4, ZK_LAZY_FR_REDUCE = 5, ZK_LAZY_FR_STORE = 6,
       ZK_LAZY_FP2_MUL = 7, ZK_LAZY_FP2_SQR = 8, ZK_LAZY_GLV_RECODE = 9, ZK_LAZY_REGULAR_RECODE = 10 };
enum { ZK_GLV_RECODE_DIGITS = 132, ZK_GLV_RECODE_WORDS = 3 + 2 * 132 };
enum { ZK_REGULAR_RECODE_DIGITS = 48, ZK_REGULAR_RECODE_WORDS = 5 + 2 * 48 };
int zk_lazy29_batch(zk_ctx* ctx, int field, int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, size_t n,
                    uint64_t* out, int32_t* raw_out);


/* ------------------------------------------------------------------------------------------
 * The plan record: what every inner product since the last reset decided from its size (csrc/msm_impl.hpp, msm_run) -- a few host
 * stores per product, nothing on the device.  It adds no entry point: it is read through the option calls of zkgpu.h, in the
 * product build as well (the tests run against that build).
 *   zk_set_option(ctx, "msm_plan_reset", 0)          empties the record
 *   zk_get_option(ctx, "msm_plan_count")             products recorded
 *   zk_get_option(ctx, "msm_plan.<i>.<field>")       one field of product i (decimal), -1 for an unknown field or index
 * Product i is the i-th in the order the host enqueued them (a proof: A, B in G2, the merged L + H product; with merge_lh = 0: L, A,
 * B, H).  A product without valid scalars launches nothing and is not recorded.  The record keeps the first 4096 products after a
 * reset; tests/msm_plan_model.py restates the rules and the GPU tests compare the two.  Fields:
 *   g2            0 = G1, 1 = G2
 *   n_used        scalars of the product (all groups of a batch together: groups x the longest group)
 *   groups        proofs of a batch that share the product (1 otherwise)
 *   c             window size of the table
 *   windows_owned how many of its floor(254 / c) + 1 windows this call sums (all of them unless ranks share the windows)
 *   buckets       2^(c-1) per group (a bucket-range shard: this rank's share)
 *   run_len       T: longest run of the bucket accumulation
 *   run_branch    the rule that set T: ZK_MSM_RUN_PLAIN (msm_run_entries as it stands), _WHOLE (one run per bucket: 128 or 256),
 *                 _FILL (as long as one round of accumulation lanes allows), _SMALL (few entries: 4 .. 28)
 *   quad_tail     1: merge and reduction tail with four lanes per addition (at most msm_quad_buckets buckets), 0: one lane
 *   unchained     1: too few lanes to fill the chip, the accumulation does not wait for the previous product's
 *   cu_count      compute units the rules were evaluated with
 * ---------------------------------------------------------------------------------------- */
enum { ZK_MSM_RUN_PLAIN = 0, ZK_MSM_RUN_WHOLE = 1, ZK_MSM_RUN_FILL = 2, ZK_MSM_RUN_SMALL = 3 };

#ifdef __cplusplus
}
#endif
#endif /* ZKGPU_MEASURE_H */
