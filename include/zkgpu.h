/* zkgpu.h -- C ABI of the MI355X-native Groth16 prover (drop-in boundary).
 *
 * The reference (republicprotocol/zksnark-rs, crate `zksnark` 0.0.2) is pure Rust with no FFI of
 * its own; this header IS the seam a maintainer binds from
 * `src/groth16/gpu.rs` (binding shown in INTEGRATION.md).  Every entry point cites the
 * reference interface it replaces (file:line into the reference tree).
 *
 * Conventions
 *   - Return value: 0 (ZK_OK) or a negative zk_status; nothing aborts or throws across the ABI.
 *     The reference panics instead (fr.rs:54,69; field/mod.rs:440); the Rust shim turns a
 *     non-zero status back into the same panic.
 *   - Fr / Fq element: uint64_t[4], little-endian limbs, CANONICAL integer < modulus
 *     (not Montgomery).  Conversions to the device's Montgomery form happen on the GPU.
 *   - G1 affine point: uint64_t[8]  = x[4] | y[4];                 infinity = all zero.
 *   - G2 affine point: uint64_t[16] = x.c0 | x.c1 | y.c0 | y.c1;   infinity = all zero.
 *     (Fq2 = Fq[i]/(i^2+1), element c0 + c1*i.)
 *   - Proof bytes (build-defined canonical encoding): 259 bytes
 *       A (G1, 65 B) | B (G2, 129 B) | C (G1, 65 B)
 *       G1: 0x04 | x | y                          (32-byte big-endian each)
 *       G2: 0x04 | x.c1 | x.c0 | y.c1 | y.c0      (EIP-197 order)
 *       infinity: 0x00 followed by zero bytes (same total length).
 *   - Compressed proof bytes (zk_proof_compress and the calls next to it): 128 bytes
 *       A (G1, 32 B) | B (G2, 64 B) | C (G1, 32 B)
 *       G1: x, 32-byte big-endian.  G2: x.c1 | x.c0, 32-byte big-endian each (EIP-197 order, as above).
 *       q < 2^254, so the two top bits of a coordinate's first byte are free; bits 7..6 of a block's byte 0 hold a flag:
 *         10  finite point; y is the SMALLER of {y, q - y}
 *         11  finite point; y is the LARGER
 *         01  infinity; every other bit of the block must be 0
 *         00  never valid (all-zero blocks included)
 *       x = the value with the flag bits cleared and must be < q (G2: both halves; the two top bits of byte 32, x.c0's first
 *       byte, must be 0).  "Larger" is decided on the CANONICAL INTEGER y in [0, q), never on a Montgomery residue:
 *       y > (q - 1) / 2; for G2: if y.c1 != 0 then y.c1 > (q - 1) / 2, else y.c0 > (q - 1) / 2.
 *       One byte string per point: x in range and x^3 + 3 (x^3 + b' on the twist) a square.  y = 0 cannot occur (both curve
 *       orders are odd: r, and r (2q - r), so there is no 2-torsion); were it ever met, only flag 10 would be accepted.
 *       Decompression checks encoding and curve membership only, NOT the order-r subgroup of B: that test stays behind every
 *       verify call, which rejects a twist point outside G2 whichever form carried it.
 *   - A zk_ctx is bound to one HIP device and must be used from one thread at a time.
 *   - All `const uint64_t*` inputs are HOST pointers unless the parameter name starts with d_.
 */
#ifndef ZKGPU_H
#define ZKGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;
typedef struct zk_crs zk_crs;   /* device-resident SigmaG1 + SigmaG2 (groth16/mod.rs:105-121) */
typedef struct zk_qap zk_qap;   /* device-resident QAP (groth16/mod.rs:60-67) */

typedef enum {
    ZK_OK = 0,
    ZK_ERR_ARG = -1,          /* null pointer / inconsistent sizes */
    ZK_ERR_HIP = -2,          /* HIP runtime error (see zk_last_error) */
    ZK_ERR_NO_DEVICE = -3,    /* no gfx950 device visible: the product path has NO CPU fallback */
    ZK_ERR_SIZE = -4,         /* size outside the supported range */
    ZK_ERR_DIV_BY_ZERO = -5,  /* "Dividend must be non-zero" (field/mod.rs:440) / Fr inverse of 0 (fr.rs:54,69) */
    ZK_ERR_RANGE = -6,        /* an Fr/Fq input is >= its modulus */
    ZK_ERR_UNSUPPORTED = -7,
    ZK_ERR_IO = -8,           /* file missing, truncated, altered or not in the expected format */
    ZK_ERR_COMM = -9          /* a collective failed (RCCL error or the caller's transport returned non-zero) */
} zk_status;

#define ZK_PROOF_BYTES 259
#define ZK_PROOF_COMPRESSED_BYTES 128
#define ZK_MAX_IN_FLIGHT 4   /* proofs one context can have submitted and not yet waited for */
#define ZK_FR_WORDS 4
#define ZK_G1_WORDS 8
#define ZK_G2_WORDS 16

/* ------------------------------------------------------------------------------------------
 * Context
 * ---------------------------------------------------------------------------------------- */
int zk_ctx_create(int device_ordinal, zk_ctx** out);
void zk_ctx_destroy(zk_ctx* ctx);
const char* zk_strerror(int status);
const char* zk_last_error(const zk_ctx* ctx);          /* detail of the last failing call */
/* Options of the product build: "msm_window_bits" (Pippenger c of the fixed-base tables; 0 = automatic, c = the same for every table,
 * 100 * big + small = `big` for tables of 2^21 points and more, + 10000 * g2 = its own window for the G2 table), "msm_shard_points"
 * (zk_prove_partial: 0 = a rank owns Pippenger windows, 1 = a rank owns a range of the points, 2 = a rank owns 1 / world of the BUCKET
 * range of every product -- the fixed-base tables share one bucket set over all windows, so this divides entries, accumulation and
 * the per-bucket reduction tail by world where 13 windows over 8 ranks leave 2 : 1; world a power of two, otherwise as 0), "rank_tables" (multi-GPU exchange:
 * 1 = window tables of the rank's own point ranges only), "dense_long_division" (1: the dense form always divides by t with the
 * reference's long division; default 0 = power-series inverse above 512 quotient coefficients), "msm_quad_buckets" (inner products of
 * at most this many buckets run their reduction tail with four lanes per point addition: shorter dependency chains for small
 * circuits; default 65536, 0 = never), "interp_large_log" (arbitrary-roots interpolation: trees of at least 2^value coefficients per
 * level take the form that re-uses the children's transforms; default 20; both forms give the same coefficients), "comm_cu_reserve"
 * (zk_mgpu_create over an RCCL communicator of more than one rank: compute units per XCD that the inner-product streams leave to the
 * collectives' kernels; default 0 = none: measured on one GPU it costs 4 % of the rate and shortens the p90 wait of an all-to-all only
 * from 2.7 to 2.2 ms, profiles/r4_rccl_starvation.txt), "basis_tree_min" (see zk_crs_upload), "merge_lh" (default 1: the witness
 * product L = sum a_i sum_delta_i and H + r B1 + s A, which only occur added together in the proof element c, are ONE inner product
 * over the table xi_t | xi | sum_delta with one set of buckets and one reduction tail; 0 = two products as in round 4; same proof
 * bytes, +1.3 % proofs/s at 2^20 gates, profiles/r5_experiments.txt item 2), "witgen_scratch_kib" (read by zk_witgen_create: how much
 * device memory, in KiB, that generator may hold for slot values; default 8388608 = 8 GiB), "boolgen_scratch_kib",
 * "boolgen_group_words" and "boolgen_expand_form" (see zk_boolgen_run), "qap_check_chunk" and
 * "qap_check_by_instance" (see zk_qap_check), "vk_table_kib" (see zk_vk_verify_batch).  Each is exercised by a -m gpu test.  Unknown keys are
 * answered with ZK_ERR_UNSUPPORTED.  Measurement entry points and switches -- kernel event timing, the tuning keys of bench.py --opt /
 * --serialize -- are NOT part of this header: include/zkgpu_measure.h. */
int zk_set_option(zk_ctx* ctx, const char* key, long value);
long zk_get_option(const zk_ctx* ctx, const char* key);

/* ------------------------------------------------------------------------------------------
 * Building blocks (individually parity-tested against the oracle)
 * ---------------------------------------------------------------------------------------- */
/* Radix-2 NTT over Fr, natural order in and out, in place on a host buffer of 2^log_n elements.
 *   inverse=0: out[k] = sum_j in[j] * w^(jk)            == field::dft   (field/mod.rs:508-520)
 *   inverse=1: w^-1 and scaling by n^-1                 == field::idft  (field/mod.rs:524-537)
 * with w = 5^((r-1)/2^log_n).  coset=1 evaluates on / interpolates from the coset g*<w> with
 * g = 5^((r-1)/2^(log_n+1)) (forward: in[j] *= g^j first; inverse: out[j] *= g^-j last).  log_n <= 24 (23 with coset). */
int zk_ntt_fr(zk_ctx* ctx, uint64_t* data, unsigned log_n, int inverse, int coset);
/* Interpolation through ARBITRARY distinct nodes: coeffs[0..n) = the coefficients of the polynomial of degree < n with
 * p(roots[k]) = values[k] -- what QAP::from does per wire polynomial with Lagrange sums (fr.rs:140-173, coefficient_poly.rs:159-200;
 * O(n^2) each) and the prover of an arbitrary-roots QAP (zk_qap_upload_sparse_roots) does per proof for U and V,
 * by a sub-product tree over batched NTTs in O(n log^2 n) (csrc/interp.hip).  1 <= n <= 2^23; ZK_ERR_ARG when two roots
 * coincide. */
int zk_interpolate_fr(zk_ctx* ctx, const uint64_t* roots, const uint64_t* values, size_t n, uint64_t* coeffs);

/* sum_i scalars[i] * points[i]: the SigmaG1/SigmaG2 inner products of groth16::prove
 * (groth16/mod.rs:255-272,279-290), i.e. n x exp_encrypted_g1/g2 (fr.rs:114-119) folded with
 * Sum for G1Local/G2Local (fr.rs:191-198,217-223).  window_bits = 0 picks automatically.  zk_msm_g1 only: window_bits in
 * [-9, -2] runs the Pippenger form BASELINE.json's north_star words with c = -window_bits -- one wavefront per (window, chunk),
 * buckets in LDS, a wave-level fold of the partial sums (csrc/msm_lds.hpp) -- a measured comparator, never used by zk_prove. */
/* Window size c (bits) the fixed-base tables of a product of `count` points are built with when the option msm_window_bits
 * is 0: the outcome of the sweeps in DESIGN.md 4c (G1: 17 from 2^17 points, 20 from 2^21; the G2 table: 20 from 2^20).  Host code, no
 * device needed.  (The reference has no such notion: fr.rs:114-119 is one double-and-add per term.) */
int zk_msm_auto_window(size_t count);
int zk_msm_auto_window_g2(size_t count);
int zk_msm_g1(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, int window_bits, uint64_t out_affine[ZK_G1_WORDS]);
int zk_msm_g2(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, size_t n, int window_bits, uint64_t out_affine[ZK_G2_WORDS]);

/* Element-wise field / group kernels (diagnostic entry points used by the parity tests).
 * op: 0 add, 1 sub, 2 mul, 3 inverse of a (b ignored; ZK_ERR_DIV_BY_ZERO if any a == 0), 4 the same inverse by the
 * binary extended Euclid (ff.cuh inv_euclid), 5 by division steps in batches of 30 (inv_divsteps: what closes a proof)
 * FrLocal Add/Sub/Mul/Div: fr.rs:18-71 */
int zk_fr_batch(zk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int zk_fq_batch(zk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* out[i] = scalars[i] * points[i]  (exp_encrypted_g1 / exp_encrypted_g2, fr.rs:114-119) */
int zk_g1_mul_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n);
int zk_g2_mul_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n);
/* out[i] = scalar * points[i], one canonical scalar < r for the whole array (0 allowed: every output is infinity).
 * Same contract as zk_g1_mul_batch otherwise (canonical in / out, coordinate >= q or scalar >= r: ZK_ERR_RANGE); infinity entries
 * (all-zero words) stay infinity, n = 0 does nothing, out may be points.  This is the routine zk_crs_contribute rescales the resident
 * arrays with (csrc/crs_contribute.hip): the host splits the scalar by the curve's endomorphism and recodes both halves
 * once, every lane walks the same digits, and a lane's four points share one field inversion.  Points are expected on the curve (as
 * every CRS array is); for other input the output is unspecified. */
int zk_g1_scale_batch(zk_ctx* ctx, const uint64_t* points, const uint64_t scalar[4], uint64_t* out, size_t n);
/* out[i] = scalars[i] * points[i] through the kernel zk_powers_contribute multiplies a transcript with (k_mul_each, csrc/powers.hip,
 * DESIGN 4n), so that it can be tested on chosen scalars.  Same contract as zk_g1_mul_batch / zk_g2_mul_batch: canonical in and out,
 * ZK_ERR_RANGE for a scalar >= r or a coordinate >= q, scalar 0 gives infinity, infinity stays infinity, out may be points.  Points
 * are expected in the group of order r.  The option "powers_mul_form" (zk_set_option; 0 = k_mul_each, the default; 1 = a plain
 * kernel over gb_mul, the per-lane non-adjacent form) selects the kernel for these calls and for zk_powers_contribute;
 * "powers_mul_ppl" (0 = chosen from the array's length, the default; 1, 2, 4) fixes how many points a lane of k_mul_each owns and
 * inverts together -- the results do not depend on either. */
int zk_g1_mul_each(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n);
int zk_g2_mul_each(zk_ctx* ctx, const uint64_t* points, const uint64_t* scalars, uint64_t* out, size_t n);
/* out[i] = a[i] + b[i]  (Add for G1Local/G2Local, fr.rs:175-215) */
int zk_g1_add_batch(zk_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
int zk_g2_add_batch(zk_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);

/* ------------------------------------------------------------------------------------------
 * QAP  (QAP<CoefficientPoly<FrLocal>>, groth16/mod.rs:60-67; built by fr.rs:140-173)
 * ---------------------------------------------------------------------------------------- */
/* One of u, v, w in root representation (circuit::RootRepresentation, circuit/mod.rs:201-214;
 * DummyRep rows, dummy_rep.rs:6-13): CSR by WIRE, entry k of wire i = (gate index, value),
 * meaning polynomial_i(root[gate]) = value.  Duplicate (wire, gate) entries add up, as the
 * reference's Lagrange sum does (coefficient_poly.rs:159-171). */
typedef struct {
    const uint64_t* ptr;   /* m+1 offsets */
    const uint32_t* gate;  /* nnz gate indices in [0, n) */
    const uint64_t* val;   /* nnz Fr values (4 words each) */
} zk_sparse_rows;

/* Sparse QAP on the domain roots[j] = w^j, w = 5^((r-1)/n), n = 2^log_n gates: the large-circuit
 * form.  Equivalent to QAP::from(root_rep) (fr.rs:140-173) with those roots; the dense
 * per-wire polynomials are never materialised. t(x) = x^n - 1. */
typedef struct {
    unsigned log_n;
    size_t m;       /* wires; wire 0 is the constant 1 */
    size_t input;   /* l = number of verifier-supplied wires (qap.input) */
    zk_sparse_rows u, v, w;
} zk_qap_sparse_desc;
int zk_qap_upload_sparse(zk_ctx* ctx, const zk_qap_sparse_desc* desc, zk_qap** out);
/* The same rows over the roots ASTParser emits, the integers 1..n (circuit/mod.rs:517: `roots: (1..=n)`), for any
 * n <= 2^23 (desc->log_n is ignored).  Equivalent to QAP::from(root_rep) (fr.rs:140-173) followed by the reference's
 * coefficient-form prove (mod.rs:199-290) -- the proofs are byte-identical to the dense form's -- but nothing is ever
 * interpolated: the prover keeps U, V as values on {1..n}, the quotient as values on {n+1..2n-1}, and takes its inner
 * products with the CRS in those Lagrange bases, which zk_setup emits next to the reference's [x^i] arrays.  Costs
 * O(nnz + n log n) per proof where the dense form is O(m n); SURVEY.md 8-f4.  With a CRS that carries only the reference's arrays
 * (zk_crs_upload, a ZKCRSv1 file) the first proof derives the Lagrange-basis points from [x^i], once per CRS: from 16384 gates on
 * (option "basis_tree_min") by the transpose of the interpolation tree run over curve points, O(n log^2 n) point operations (2.2 s at
 * 2^16 gates, 40 s at 2^20, n <= 2^22; csrc/gbasis.hip), below by n^2 inner products (csrc/basis.hip).  With basis_tree_min < 0 a
 * CRS of more than 2^16 + 2^10 gates is served through the form of zk_qap_upload_sparse_roots with the roots 1..n instead (same
 * bytes, 0.6 x the rate).
 * Batches and the multi-GPU entry points take both sparse forms. */
int zk_qap_upload_sparse_integers(zk_ctx* ctx, const zk_qap_sparse_desc* desc, size_t n, zk_qap** out);
/* The same rows over ANY distinct roots r_0 .. r_{n-1} the caller supplies (RootRepresentation::roots() is caller data,
 * circuit/mod.rs:201-214, dummy_rep.rs:47): gate j = root roots[j] (4 words each, canonical), 1 <= n <= 2^22.  Equivalent to
 * QAP::from(root_rep) (fr.rs:140-173) followed by the reference's coefficient-form prove -- byte-identical proofs -- but the 3 m wire
 * polynomials are never interpolated: the prover interpolates U = sum a_i u_i and V per proof from their values on the roots by a
 * sub-product tree (csrc/interp.hip, O(n log^2 n)), divides U V by t (the remainder is dropped) and takes its inner products with the
 * reference's own [x^i] arrays, so ANY CRS for the circuit serves (zk_setup, zk_crs_upload, a file).  The tables of a root set (the tree,
 * the weights 1 / N'(r_k) by a scaled remainder tree) are O(n log^2 n) too: 0.14 s at 2^20 gates.  ZK_ERR_ARG when two roots coincide.  One proof at a time or pipelined on one GPU, or
 * window-sharded (zk_prove_partial); batches and the scalar exchange take the two forms above (ZK_ERR_UNSUPPORTED). */
int zk_qap_upload_sparse_roots(zk_ctx* ctx, const zk_qap_sparse_desc* desc, const uint64_t* roots, size_t n, zk_qap** out);

/* Dense coefficient form, exactly the fields of QAP<CoefficientPoly<FrLocal>>: u, v, w are
 * m x n row-major (coefficient k of wire i at [i*n + k], zero padded), t has n+1 coefficients
 * (any roots; e.g. ASTParser's 1..n, circuit/mod.rs:517) and is expected to have degree exactly n: t[n] != 0, monic or not.  The
 * CRS of this library has n powers of x and n - 1 of x^i t(x), where the reference sizes them by deg t (groth16/mod.rs:134-197), so
 * only for deg t = n are the proof bytes pinned to the reference's (tests/test_gpu_quotient.py); what a t of lower degree gives is
 * not part of the contract. */
int zk_qap_upload_dense(zk_ctx* ctx, const uint64_t* u, const uint64_t* v, const uint64_t* w, const uint64_t* t,
                        size_t m, size_t n, size_t input, zk_qap** out);
void zk_qap_free(zk_qap* qap);

/* Dimensions of a device QAP, and its dense coefficient matrices back on the host (dense form only;
 * any pointer may be NULL = skip).  Layout as zk_qap_upload_dense. */
int zk_qap_dims(const zk_qap* qap, size_t* n, size_t* m, size_t* input, int* dense);
/* Which device form a QAP handle holds (a container read by zk_qap_load does not say otherwise): 0 = sparse rows over the roots of
 * unity w^j, n = 2^k (zk_qap_upload_sparse); 1 = the dense m x n coefficient matrices of QAP<CoefficientPoly<FrLocal>>
 * (groth16/mod.rs:60-67; zk_qap_upload_dense, zk_circuit_qap); 2 = sparse rows over the integers 1..n, the roots ASTParser emits
 * (circuit/mod.rs:517; zk_qap_upload_sparse_integers); 3 = sparse rows over the caller's roots (zk_qap_upload_sparse_roots). */
int zk_qap_kind(const zk_qap* qap);
/* The first stage of groth16::prove on its own (diagnostic entry point of the parity tests): u_sum = sum_i qap.u[i] * weights[i]
 * (groth16/mod.rs:233-253 -- zip with the weights, CoefficientPoly: Mul<T> coefficient_poly.rs:132-146, Sum :75-91); which = 0 / 1 / 2
 * for u / v / w.  Dense form: out = the n coefficients of the sum.  Sparse forms: out = its n values on the QAP's domain (w^j or
 * j + 1, j < n), u and v only (the prover never evaluates W).  4 words per element, canonical; weights beyond m_qap are ignored. */
int zk_qap_weighted_sum(zk_ctx* ctx, const zk_qap* qap, const uint64_t* weights, size_t m, int which, uint64_t* out);
int zk_qap_download_dense(zk_ctx* ctx, const zk_qap* qap, uint64_t* u, uint64_t* v, uint64_t* w, uint64_t* t);

/* Does a witness satisfy the QAP, and if not, where?  groth16::prove drops the remainder of (U V - W) / t (mod.rs:233-253,277), so a
 * witness that breaks a constraint still yields 259 well-formed bytes that zk_verify rejects; this is the is_satisfied /
 * which_is_unsatisfied the reference lacks, as a call of its own -- no zk_prove* entry point runs it.
 *  - Gate values: U_j = sum_i a_i u_i(root_j) over the entries of gate j (0-based gate index = row of the root representation),
 *    V_j and W_j alike; duplicate (wire, gate) entries add up, as everywhere else.  Gate j is bad when U_j V_j != W_j (mod r).
 *  - Only wires i < min(m, m_qap) contribute, because zip(weights) truncates (mod.rs:233-253): the answer is about what zk_prove* does
 *    with exactly these arguments.  A short witness is legal, its missing wires count as 0.  Words behind min(m, m_qap) and the
 *    padding between instances (stride > m) are never read and may hold anything.
 *  - Satisfied means bad_gates == 0 && flags == 0.  ZK_QAP_CHECK_WIRE0: the constant wire is not 1 (or there is no weight at all); then
 *    every gate may hold and zk_verify still rejects the proof.
 *  - The three sparse forms (zk_qap_kind 0, 2, 3) are supported; the roots never enter, only the rows by gate.  The dense form (kind 1)
 *    gives ZK_ERR_UNSUPPORTED: it holds coefficients and t, not its roots, so no gate can be named -- zk_circuit_qap_sparse is the
 *    way in for .zk circuits.
 *  - An element >= r among the min(m, m_qap) read of any instance: ZK_ERR_RANGE, found on the device; zk_last_error names the LOWEST
 *    such instance and `out` is unspecified.
 *  - count == 0: ZK_OK, nothing touched.  Null ctx / qap / out, null weights with m > 0, stride < m, a QAP of another context:
 *    ZK_ERR_ARG.
 *  - Synchronous, on a stream of its own as the batch verifiers are, no device-wide synchronisation: an outstanding
 *    zk_prove_submit ticket is neither waited for nor disturbed.  U, V and W are never written to memory.  The first check of a QAP
 *    builds W's rows by gate (36 bytes per entry of w; the prover never needs them) and keeps them with the handle.
 *  - Any count: the instances go through the device in chunks of at most "qap_check_chunk" (instance, gate) pairs per launch (option,
 *    default ZK_QAP_CHECK_CHUNK_LANES; at least one instance per launch); the results do not depend on the chunking.  Option
 *    "qap_check_by_instance" (default 0: consecutive lanes take consecutive gates of one instance; 1: consecutive lanes take the same
 *    gate of consecutive instances -- the other mapping of the A/B in DESIGN 4h, kept as the cross-check of the first). */
#define ZK_QAP_CHECK_NONE 0xFFFFFFFFu
#define ZK_QAP_CHECK_WIRE0 1u    /* flags: weights[0] != 1 (or no weights at all) */
#define ZK_QAP_CHECK_CHUNK_LANES (1u << 28)
typedef struct {
    uint32_t bad_gates;   /* number of gates j with U_j * V_j != W_j (mod r) */
    uint32_t first_bad;   /* lowest such j, ZK_QAP_CHECK_NONE if none */
    uint32_t flags;       /* ZK_QAP_CHECK_WIRE0 */
} zk_qap_check_result;
/* one witness in host memory */
int zk_qap_check(zk_ctx* ctx, const zk_qap* qap, const uint64_t* weights, size_t m, zk_qap_check_result* out);
/* `count` witnesses in DEVICE memory, witness j at d_weights + j * stride * 32 bytes, m elements each (stride >= m; stride == m is
 * zk_witgen_run's output layout); out: `count` results in HOST memory.  Complete on return. */
int zk_qap_check_dev(zk_ctx* ctx, const zk_qap* qap, const void* d_weights, size_t m, size_t stride, size_t count,
                     zk_qap_check_result* out);

/* ------------------------------------------------------------------------------------------
 * .zk front end (the input side of the path; host code, as in the reference)
 * ---------------------------------------------------------------------------------------- */
typedef struct zk_circuit zk_circuit;   /* DummyRep<FrLocal> (circuit/dummy_rep.rs:6-13) + the parsed program */
/* ASTParser::try_parse (circuit/mod.rs:224-527; tokenizer/AST: circuit/ast.rs).  On a parse error
 * returns ZK_ERR_ARG and writes the ParseErr text ("SyntaxErr(line, ..)" / "StructureErr(gate, ..)")
 * to err.  Wire 0 is the constant 1, then the `verify` variables, then first appearance; gate k
 * (1-based) sits at root k (circuit/mod.rs:517). */
int zk_circuit_parse(const char* code, zk_circuit** out, char* err, size_t err_len);
void zk_circuit_free(zk_circuit* c);
int zk_circuit_dims(const zk_circuit* c, size_t* m, size_t* n, size_t* input, size_t* n_in);
/* Root representation rows (RootRepresentation::u/v/w, circuit/mod.rs:201-214): which = 0 u, 1 v, 2 w;
 * ptr[m+1], gate[nnz] (0-based gate index = root - 1), val[nnz*4].  NULL arrays are skipped. */
int zk_circuit_rows(const zk_circuit* c, int which, uint64_t* ptr, uint32_t* gate, uint64_t* val, size_t* nnz);
/* circuit::weights (circuit/mod.rs:529-637): inputs in `in` order -> [1] ++ wire values (m x 4 words) */
int zk_circuit_weights(const zk_circuit* c, const uint64_t* inputs, size_t n_in, uint64_t* weights_out, size_t m);
const char* zk_circuit_last_error(const zk_circuit* c);
/* zk_circuit_parse also compiles circuit::weights into a flat tape: field operations dst = a (*|+) b or dst = a over numbered slots
 * (slot 0 = the constant 1, slot i + 1 = the i-th variable of the witness, behind them unused `in` variables and temporaries), operands
 * a slot or a literal of the constant pool, no slot written twice, sorted by level (1 + the highest level read; inputs and constants
 * are level 0).  A program whose weights fail for EVERY input (assignment to an assigned variable, an unbound variable, a variable
 * order that does not cover the wires) still parses; the calls below then return that error, status and text as zk_circuit_weights'. */
/* assignments-level shape of the program: depth = number of levels when each `=` is one node, width = most `=` in one level;
 * ops / slots / consts = what the compiled tape holds (any pointer may be NULL).  Returns the stored static error if the program has one. */
int zk_circuit_tape_dims(const zk_circuit* c, size_t* ops, size_t* slots, size_t* consts, size_t* depth, size_t* width);
/* zk_circuit_weights through the tape: same arguments, same words out, same status and text on every error; nothing is parsed, no
 * name is looked up and nothing recurses per call. */
int zk_circuit_weights_tape(const zk_circuit* c, const uint64_t* inputs, size_t n_in, uint64_t* weights_out, size_t m);
/* QAP<CoefficientPoly<FrLocal>>::from(root_rep) (fr.rs:140-173; Lagrange interpolation
 * coefficient_poly.rs:159-200) on the GPU for the circuit's roots 1..n -> dense device QAP. */
int zk_circuit_qap(zk_ctx* ctx, const zk_circuit* c, zk_qap** out);
/* The same QAP through zk_qap_upload_sparse_integers: no interpolation, no 16384-gate limit, identical proofs. */
int zk_circuit_qap_sparse(zk_ctx* ctx, const zk_circuit* c, zk_qap** out);

/* Witness generation for a whole batch on the GPU: the tape run with one instance per lane (csrc/witgen.hip). */
typedef struct zk_witgen zk_witgen;
/* uploads the circuit's tape and constant pool; the circuit may be freed afterwards, the context must outlive the generator.
 * Static program error -> that error (zk_last_error has the text). */
int zk_witgen_create(zk_ctx* ctx, const zk_circuit* c, zk_witgen** out);
void zk_witgen_free(zk_witgen* w);     /* NULL is a no-op */
/* circuit::weights for `count` input sets at once.  d_inputs: count x n_in x 4 words, canonical, instance-major (instance j's block is
 * what zk_circuit_weights takes); d_weights_out: count x m x 4 words, canonical, instance-major, so d_weights_out + j*m*4 words is a
 * valid d_weights[j] of zk_prove_batch_submit / d_weights of zk_prove_dev.  Both device pointers.  Complete on return.  count == 0:
 * ZK_OK, nothing touched.  n_in or m not the program's: ZK_ERR_ARG with zk_circuit_weights' text.  An input word pattern >= r in any
 * instance (unused `in` variables included, as on the host): ZK_ERR_RANGE, found on the device; zk_last_error names the LOWEST such
 * instance and the contents of d_weights_out are unspecified.  Scratch: slots x 2 KiB per 64 instances in flight, at most the option
 * "witgen_scratch_kib" -- `count` is not limited by memory (the instances run in chunks), a program of which 64 instances do not fit
 * gives ZK_ERR_SIZE. */
int zk_witgen_run(zk_witgen* w, const void* d_inputs, size_t n_in, size_t count, void* d_weights_out, size_t m);

/* ------------------------------------------------------------------------------------------
 * Gate-level circuit builder (the reference's second front end: circuit/builder/mod.rs, types.rs; host code, no context)
 * ---------------------------------------------------------------------------------------- */
/* Circuit<T> (builder/mod.rs:56-64).  Wires are numbered from 2 in creation order; wire 0 is the constant 0 and wire 1 the constant 1
 * (Circuit::new, zero_wire, unity_wire: mod.rs:91-114).  Every call below returns ZK_ERR_ARG with text (zk_builder_last_error) for a
 * wire id that was never handed out and for any call but zk_builder_free after zk_builder_finish.
 * Deviations from the reference, all deliberate:
 *   - wire and witness order are deterministic (creation order; the reference iterates a HashMap);
 *   - the constant-zero wire is NOT a witness wire: a wire meant to be 0 that no constraint fixes would let the prover put anything
 *     there, so its entries are dropped from every sub-circuit at zk_builder_finish (they contribute 0 either way);
 *   - the reference's builder -> DummyRep conversion prepends num_wires empty rows and is not reproduced: sub-circuit k
 *     is gate k;
 *   - zk_builder_assert_bit and zk_builder_pack exist (see there). */
typedef struct zk_builder zk_builder;
#define ZK_WIRE_ZERO 0u
#define ZK_WIRE_ONE 1u
#define ZK_WIRE_BIT 0     /* an input that must be 0 or 1: new_word8 / new_word64 are 8 / 64 of them, least significant bit first (mod.rs:151-190) */
#define ZK_WIRE_FIELD 1   /* an input that is any field element (new_wire, mod.rs:120-125); the circuit is then not boolean */
int zk_builder_create(zk_builder** out);
void zk_builder_free(zk_builder* b);     /* NULL is a no-op */
const char* zk_builder_last_error(const zk_builder* b);
/* wires handed out so far (the two constants included) and sub-circuits = gates so far; either pointer may be NULL */
int zk_builder_dims(const zk_builder* b, size_t* wires, size_t* gates);
/* `count` new input wires, ids to out[0..count).  The circuit's inputs are these wires in creation order. */
int zk_builder_new_wires(zk_builder* b, int kind, size_t count, uint32_t* out);
/* new_sub_circuit (mod.rs:491-557): (sum left_weights[i] * left_wires[i]) * (sum right_weights[i] * right_wires[i]) = *out, a new wire.
 * Weights are 4 canonical words each (>= r: ZK_ERR_RANGE).  The circuit is then not boolean. */
int zk_builder_sub_circuit(zk_builder* b, const uint64_t* left_weights, const uint32_t* left_wires, size_t nl, const uint64_t* right_weights,
                           const uint32_t* right_wires, size_t nr, uint32_t* out);
/* new_bit_checker, new_not, new_and, new_or, new_xor, new_nand, new_nor, new_xnor (mod.rs:723-798), new_less_than, new_greater_than
 * (mod.rs:939-950): exactly the reference's sub-circuits with its weights -- OR, NAND and NOR are two, the intermediate AND wire
 * included -- and no constant folding: a gate on ZK_WIRE_ZERO or ZK_WIRE_ONE is still a gate.  y is ignored by BIT_CHECK and NOT.
 * The bit checker's output x (x - 1) is an ordinary, unconstrained wire, as in the reference. */
#define ZK_GATE_BIT_CHECK 0
#define ZK_GATE_NOT 1
#define ZK_GATE_AND 2
#define ZK_GATE_OR 3
#define ZK_GATE_XOR 4
#define ZK_GATE_NAND 5
#define ZK_GATE_NOR 6
#define ZK_GATE_XNOR 7
#define ZK_GATE_LESS 8
#define ZK_GATE_GREATER 9
int zk_builder_gate(zk_builder* b, int kind, uint32_t x, uint32_t y, uint32_t* out);
/* bitwise_op (mod.rs:817-827): out[i] = gate(x[i], y[i]), i ascending; y may be NULL for the unary kinds */
int zk_builder_bitwise(zk_builder* b, int kind, const uint32_t* x, const uint32_t* y, size_t n, uint32_t* out);
/* fan_in (mod.rs:801-814): the left fold gate(.. gate(gate(x[0], x[1]), x[2]) .., x[n-1]); n >= 1, n == 1 emits nothing; binary kinds only */
int zk_builder_fan_in(zk_builder* b, int kind, const uint32_t* x, size_t n, uint32_t* out);
/* is_equal, is_equal_zero, less_than, less_than_eq, greater_than, greater_than_eq (mod.rs:995-1241) over two arrays of n_bits >= 1 bit
 * wires, least significant first, in the reference's composition.  EQUAL_ZERO ignores `right`.  At n_bits == 1 the reference's
 * greater_than panics (a fan_in over no equalities); here it is the single new_greater_than gate. */
#define ZK_CMP_EQUAL 0
#define ZK_CMP_EQUAL_ZERO 1
#define ZK_CMP_LESS 2
#define ZK_CMP_LESS_EQ 3
#define ZK_CMP_GREATER 4
#define ZK_CMP_GREATER_EQ 5
int zk_builder_compare(zk_builder* b, int kind, const uint32_t* left, const uint32_t* right, size_t n_bits, uint32_t* out);
/* The sponge of keccakf_1600 / absorb / xorin / pad / squeeze (mod.rs:1247-1398) in general form: in_wires are 8 * n_bytes bit wires
 * (byte k = wires 8k .. 8k+7, least significant first), out_wires receives 8 * out_bytes.  Absorb is XOR into the state, the padding
 * XORs `delim` at the offset and 0x80 at rate_bytes - 1; theta is 5 x 5 XORs from the zero word and a 3-input XOR fan-in, rho / pi
 * rename, chi is NOT, AND, XOR, iota XORs a constant word.  keccak256 (mod.rs:1428-1439) is (136, 0x01, 24), SHA3-256 (136, 0x06, 24).
 * rounds in 1..24 runs the first `rounds` rounds of the permutation (short forms for tests and demonstrations): 9664 gates per round,
 * 8 k + 16 + 9664 rounds for a one-block message of k bytes.  rate_bytes in 1..200. */
int zk_builder_keccak(zk_builder* b, const uint32_t* in_wires, size_t n_bytes, unsigned rate_bytes, unsigned delim, unsigned rounds,
                      uint32_t* out_wires, size_t out_bytes);
/* The gate w (w - 1) = 0 with NO output wire (an empty W entry).  The reference's bit checker only produces an unconstrained wire,
 * so without this call a verifier has no way to force an input to be 0 or 1. */
int zk_builder_assert_bit(zk_builder* b, uint32_t wire);
/* out = sum_i 2^i * bits[i], as ONE sub-circuit (sum 2^i bits[i]) * (1) = out.  1 <= n_bits <= ZK_PACK_MAX_BITS (253), so the sum of
 * 0/1 operands is < 2^253 < r and distinct bit strings give distinct elements.  Operands may be any known wire, ZK_WIRE_ONE (adds 2^i)
 * and ZK_WIRE_ZERO (dropped at finish, like everywhere) included, and a wire may occur at several positions.  n_bits of 0 or above
 * 253: ZK_ERR_ARG with text.  The output is a PACKED wire: an ordinary witness index, a field element instead of a bit; it may be a
 * verify wire -- a 256-bit digest is then two public inputs of 128 bits instead of 256.  The circuit stays bit-sliceable
 * (zk_circuit_is_boolean) iff every pack operand is a constant, a ZK_WIRE_BIT input or the output of a gate, comparator or sponge
 * sub-circuit, and no packed wire is an operand of anything; a packed wire fed into a gate, another pack, zk_builder_assert_bit, a
 * comparator or the sponge is legal and sends the circuit to the tape (zk_witgen_*), as zk_builder_sub_circuit does. */
#define ZK_PACK_MAX_BITS 253
int zk_builder_pack(zk_builder* b, const uint32_t* bits, size_t n_bits, uint32_t* out);
/* *out = Poseidon(in_wires[0 .. arity)) (see "Poseidon" below), arity 1, 2 or 4.  The state is t = arity + 1 linear forms over wires
 * (one term per wire, weights mod r, the constant on ZK_WIRE_ONE); an S-box on a form L is three sub-circuits L * L = a, a * a = c,
 * c * L = e; round constants and the mix are folded into the forms and cost no gate; one closing sub-circuit (state[0]) * 1 = out
 * makes the digest a wire.  Exactly 3 (8 t + R_P) + 1 gates: 217, 244, 301 for arity 1, 2, 4; a side has at most t + R_P + 1 terms.
 * Inputs may be any known wire, constants and bit wires included, and a wire may repeat.  The output is field-class: the circuit is
 * not boolean and goes to the tape or the mixed path, as zk_builder_sub_circuit does.  ZK_ERR_ARG with text: another arity, an
 * unknown wire, a null pointer. */
int zk_builder_poseidon(zk_builder* b, const uint32_t* in_wires, size_t arity, uint32_t* out);
/* *out = the root of the Merkle path from `leaf` through siblings[0 .. depth) (the sibling of level k) with direction wires
 * dirs[0 .. depth) (1: the path's node is the RIGHT child at level k), over Poseidon of arity 2: what zk_poseidon_tree_paths hands
 * out.  Per level: zk_builder_assert_bit(dir), one gate dir * (sib - cur) = d, and Poseidon of the forms (cur + d, sib - d) -- 246
 * gates.  depth == 0: *out = leaf, nothing is emitted.  ZK_ERR_ARG with text: an unknown wire, a null array. */
int zk_builder_merkle_root(zk_builder* b, uint32_t leaf, const uint32_t* siblings, const uint32_t* dirs, size_t depth, uint32_t* out);
/* Baby Jubjub gadgets (see "Baby Jubjub" below).  A point is THREE wires (X, Y, Z), projective: x = X / Z, y = Y / Z; an affine point
 * is (x, y, ZK_WIRE_ONE).  The tape cannot divide, so the gadgets evaluate the projective formulas forward and never return affine
 * wires; where a statement needs affine coordinates the caller supplies them as wires (typically ZK_WIRE_FIELD inputs computed by
 * zk_babyjub_mul or zk_babyjub_mul_batch) and zk_builder_babyjub_affine pins them.  The Z of every gadget's result is a product of the
 * addition law's denominators, which do not vanish on curve points, so x Z = X determines x.  All gates are general sub-circuits over
 * linear forms (field-class, as zk_builder_poseidon).  ZK_ERR_ARG with text: an unknown wire, a null array, n_bits outside 1..256; a
 * refused call emits nothing.  Output arrays may alias input arrays.
 * The gates x x = u, y y = v, u v = w and the assertion (a u + v - 1 - d w) * 1 = 0 without output: 4 gates. */
int zk_builder_babyjub_assert_on_curve(zk_builder* b, const uint32_t xy[2]);
/* out = p + q by add-2008-bbjlp: Z1 Z2 = A, A A = B, X1 X2 = C, Y1 Y2 = D, C D = E, (X1 + Y1)(X2 + Y2) = H, A (B - d E), A (B + d E),
 * then X3, Y3, Z3: 11 gates, 10 when q[2] is ZK_WIRE_ONE (A = Z1 is then no gate).  The law is complete: the result is right for ALL
 * pairs of curve points, equal, opposite and of low order included.  It does NOT assert that p or q lie on the curve. */
int zk_builder_babyjub_add(zk_builder* b, const uint32_t p[3], const uint32_t q[3], uint32_t out[3]);
/* out = [sum_i 2^i bits[i]] Base8, 1 <= n_bits <= 256.  zk_builder_assert_bit on every bit first; then windows of 3 bits from the least
 * significant: the window's point j 8^k Base8 (j = 0: the identity) as two forms, multilinear in the bits, over the 4 product gates
 * b0 b1, b0 b2, b1 b2, (b0 b1) b2 (a last window of two bits: 1, of one bit: 0); the first window is the accumulator, every further
 * one costs a mixed addition of 10 gates.  n_bits <= 3: two closing gates (form) * 1 make X and Y wires and out[2] = ZK_WIRE_ONE.
 * Gates: n_bits + 4 floor(n_bits / 3) + [n_bits mod 3 = 2] + 10 (windows - 1), or + 2 for one window: 1414 for 251 bits, 1446 for 256. */
int zk_builder_babyjub_mul_fixed(zk_builder* b, const uint32_t* bits, size_t n_bits, uint32_t out[3]);
/* out = [sum_i 2^i bits[i]] P for the affine point P = (p_xy[0], p_xy[1]), 1 <= n_bits <= 256.  zk_builder_babyjub_assert_on_curve(P)
 * and zk_builder_assert_bit on every bit first; then from the most significant bit: the selection b Px, b (Py - 1) of P or the identity
 * (2 gates), and per further bit a doubling (7 gates), the selection and a mixed addition (10).  Gates: 4 + n_bits + 2 + 19 (n_bits - 1);
 * n_bits = 1: one closing gate makes Y a wire (8 gates) and out[2] = ZK_WIRE_ONE. */
int zk_builder_babyjub_mul(zk_builder* b, const uint32_t p_xy[2], const uint32_t* bits, size_t n_bits, uint32_t out[3]);
/* Pins the existing wires xy as the affine form of p: x Z = t, (t - X) * 1 = 0, and the same for y: 4 gates, no new point. */
int zk_builder_babyjub_affine(zk_builder* b, const uint32_t p[3], const uint32_t xy[2]);
/* The statement "the owner of A signed M" (see "EdDSA-Poseidon" below): [S] Base8 = R8 + [8] ([hm] A) with hm = H6(R8.x, R8.y, A.x, A.y, M),
 * over the affine wires a_xy and r8_xy, the message wire, and the 251 bits of S and the 254 bits of hm, least significant first.  The
 * hm bits are inputs the caller supplies, because the tape cannot decompose an element; zk_eddsa_verify_batch produces them on the
 * device.  Emitted from the existing gadgets, in this order:
 *   zk_builder_babyjub_assert_on_curve(R8)                                                                       4 gates
 *   zk_builder_compare(ZK_CMP_LESS, s_bits, the bits of l as ZK_WIRE_ONE / ZK_WIRE_ZERO, 251), then (lt - 1) * 1 = 0    32881
 *   the same for hm_bits against the bits of r over 254 bits: circomlib's alias check -- without it a prover may use
 *   hm + r wherever that is below 2^254                                                                          33655
 *   H6 over the five forms: 3 (8 * 6 + 60) + 1                                                                   325
 *   (sum_i 2^i hm_bits[i] - digest) * 1 = 0, one assertion over 254 bits (zk_builder_pack stops at 253)            1
 *   zk_builder_babyjub_mul(A, hm_bits, 254), which asserts A on the curve and every hm bit                        5067
 *   three doublings (7 each) and the mixed addition of R8 (10)                                                    31
 *   zk_builder_babyjub_mul_fixed(s_bits, 251), which asserts every S bit                                          1414
 *   per coordinate X1 Z2 = t1, X2 Z1 = t2, (t1 - t2) * 1 = 0: an assertion has no output, so a product costs a gate
 *   on either side                                                                                                6
 * 73384 gates.  The two comparators are nine tenths of that: the reference's greater_than folds its equalities anew for every bit
 * (n^2 / 2 AND gates).  They are boolean-class gates, so zk_mixgen_* runs them in the bit-sliced core; the rest is the field tail.
 * No affine wire and no division.  Not offered: circomlib's `enabled` input, and its rejection of keys with 8 A = identity (that
 * needs an inverse hint the tape cannot compute; zk_eddsa_verify has no such check either).  ZK_ERR_ARG with text: an unknown wire, a
 * null array; a refused call emits nothing. */
int zk_builder_eddsa_verify(zk_builder* b, const uint32_t a_xy[2], const uint32_t r8_xy[2], uint32_t msg, const uint32_t s_bits[251],
                            const uint32_t hm_bits[254]);
/* The circuit as an ordinary zk_circuit (free it with zk_circuit_free; the builder may be freed before or after).  Witness order: the
 * constant 1, the verify wires in the order given (qap.input = n_verify), the remaining input wires in creation order, the remaining
 * wires by id.  Sub-circuit k is gate k (0-based), at root k + 1 of zk_circuit_qap / _qap_sparse.  ZK_ERR_ARG with text: a verify wire
 * named twice or equal to a constant.  Every zk_circuit_* call and zk_witgen_create work on the result: zk_circuit_weights evaluates
 * the sub-circuits in creation order (what the reference's memoised evaluate, mod.rs:559-595, computes), zk_circuit_weights_tape and
 * zk_witgen_run a tape compiled from them; n_in is the number of input wires, inputs are field elements in creation order, and a
 * value other than 0 or 1 on a ZK_WIRE_BIT input is ZK_ERR_RANGE with instance, input and wire named. */
int zk_builder_finish(zk_builder* b, const uint32_t* verify_wires, size_t n_verify, zk_circuit** out);
/* 1: zk_boolgen_create takes the circuit -- every input is a bit wire and every sub-circuit came from a gate, a comparator, the sponge,
 * zk_builder_assert_bit or a zk_builder_pack over bit-valued wires whose output nothing reads (see there); 0: anything else, every
 * parsed circuit included */
int zk_circuit_is_boolean(const zk_circuit* c);
/* *count = the number of packed wires (zk_builder_pack calls); 0 for parsed circuits and for built circuits without packs */
int zk_circuit_packed_wires(const zk_circuit* c, size_t* count);
/* witness index of a builder wire in a built circuit (ZK_WIRE_ONE -> 0).  ZK_ERR_ARG: a parsed circuit, an unknown id, ZK_WIRE_ZERO. */
int zk_circuit_wire_index(const zk_circuit* c, uint32_t wire, size_t* index);
/* The circuit's rows through zk_qap_upload_sparse: gate k at w^k, n padded to the next power of two by empty gates (t = x^n - 1).  For
 * parsed and built circuits alike; the reference's builder leaves the points to the caller, and this is the faster prover here. */
int zk_circuit_qap_sparse_unity(zk_ctx* ctx, const zk_circuit* c, zk_qap** out);

/* Bit-sliced witness generation for boolean circuits (csrc/boolgen.hip): one 64-bit word holds a wire's value for 64 instances. */
typedef struct zk_boolgen zk_boolgen;
/* uploads the circuit's boolean tape; the circuit may be freed afterwards, the context must outlive the generator.  A circuit that is
 * not boolean (zk_circuit_is_boolean) -> ZK_ERR_UNSUPPORTED with text: such circuits go through zk_witgen_*. */
int zk_boolgen_create(zk_ctx* ctx, const zk_circuit* c, zk_boolgen** out);
void zk_boolgen_free(zk_boolgen* g);     /* NULL is a no-op */
/* The witnesses of `count` input sets.  d_in_bits: packed, instance-major: input i of instance j is bit i % 8 of the byte i / 8 at
 * d_in_bits + j * in_stride_bytes (a Keccak message is simply its bytes); bits past n_in in the last byte are ignored.
 * d_weights_out: exactly zk_witgen_run's, count x m x 4 words, canonical, instance-major, so d_weights_out + j*m*4 words is a valid
 * d_weights[j] of zk_prove_batch_submit / d_weights of zk_prove_dev / zk_qap_check_dev.  Both device pointers.  Complete on return.
 * count == 0: ZK_OK, nothing touched.  m not the circuit's or in_stride_bytes < ceil(n_in / 8): ZK_ERR_ARG.  Scratch: (m + 1) x 8
 * bytes per 64 instances in flight, at most the option "boolgen_scratch_kib" (read by zk_boolgen_create; default 4194304 = 4 GiB) --
 * `count` is not limited by memory (the instances run in chunks and the results do not depend on the chunking), a circuit of which
 * 64 instances do not fit gives ZK_ERR_SIZE.  Option "boolgen_group_words" (read by zk_boolgen_create): how many 64-instance words one
 * workgroup of the evaluation owns, 1, 2, 4 or 8; 0 = the default rule.  Option "boolgen_expand_form" (read by zk_boolgen_create): how
 * the witnesses are written out, 0 = a lane per wire, 1 = a lane pair per wire; the same bytes (DESIGN 4o has the measurement). */
int zk_boolgen_run(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, void* d_weights_out, size_t m);
/* The same evaluation, returning only the named witness indices, packed as the inputs are: wire wires[i] of instance j is bit i % 8
 * of the byte i / 8 at d_out_bits + j * out_stride_bytes (unused bits of the last byte are 0, bytes behind it untouched).  This is how
 * a caller gets a digest -- the public inputs -- without 32 bytes per wire.  wires is a host array of witness indices < m.
 * Errors as zk_boolgen_run; out_stride_bytes < ceil(n_wires / 8), an index >= m or the index of a packed wire (no bit: use
 * zk_boolgen_eval_fields): ZK_ERR_ARG. */
int zk_boolgen_eval(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, const uint32_t* wires, size_t n_wires,
                    void* d_out_bits, size_t out_stride_bytes);
/* wires[i] (witness indices < m, bit wires and packed wires alike) of instance j -> 4 canonical words at
 * d_out_words + (j * n_wires + i) * 4: with wires = 1..l this is exactly the `inputs` array of zk_verify_batch / zk_vk_verify_batch.
 * Nothing else is written.  Errors as zk_boolgen_eval. */
int zk_boolgen_eval_fields(zk_boolgen* g, const void* d_in_bits, size_t in_stride_bytes, size_t count, const uint32_t* wires,
                           size_t n_wires, void* d_out_words);

/* Mixed circuits on the bit-sliced path (csrc/mixgen.hip).  zk_builder_finish splits EVERY built circuit into a boolean core and a
 * field tail.  A witness index is bit-class if it is the constant 1, a ZK_WIRE_BIT input or the output of a gate (bit checker .. greater
 * than, the sub-circuits of comparators and the sponge included) whose operands are bit-class; every other index is field-class: a
 * ZK_WIRE_FIELD input, the output of zk_builder_sub_circuit, a packed wire, and whatever reads one of these.  Nothing bit-class reads
 * anything field-class.  The core is one boolean operation per bit-class sub-circuit (for a boolean circuit: the tape of
 * zk_boolgen_*); a pack whose operands are all bit-class is gathered from their bits; every other sub-circuit with an output is a
 * tail operation, compiled from its weights like the tape of zk_witgen_* (an XOR gate on a field wire is (x - y)(x - y)).
 * *n_bit_inputs / *n_field_inputs: the ZK_WIRE_BIT / ZK_WIRE_FIELD inputs; *core_ops, *core_levels: the boolean tape;
 * *tail_ops, *tail_levels: the field tape (a core pack that the tail reads costs one copy); *tail_slots: field elements the tail
 * keeps per instance (field inputs, field-class wires it computes, temporaries).  Any pointer may be NULL.  A parsed circuit:
 * ZK_ERR_UNSUPPORTED with text.  zk_builder_finish answers ZK_ERR_SIZE for a circuit with 2^30 or more witness indices, packs, tail
 * slots, tail operations or constants: a tail operand keeps two bits of its 32 to say what it names. */
int zk_circuit_mixed_dims(const zk_circuit* c, size_t* n_bit_inputs, size_t* n_field_inputs, size_t* core_ops, size_t* core_levels,
                          size_t* tail_ops, size_t* tail_levels, size_t* tail_slots);
/* One witness through the split on the host: what the kernels of zk_mixgen_run compute for one instance, the way
 * zk_circuit_weights_tape is zk_witgen_run's model.  in_bits: the ZK_WIRE_BIT inputs packed, bit k % 8 of byte k / 8 = the k-th such
 * input in input order, n_bit_bytes = ceil(n_bit_inputs / 8) (bits past the last input are ignored); in_fields: the ZK_WIRE_FIELD
 * inputs in input order, 4 canonical words each.  weights_out: m x 4 words, those of zk_circuit_weights on the same values.  Status and
 * text as zk_circuit_weights: a wrong n_bit_bytes, n_field or m is ZK_ERR_ARG "StructureErr(...)", a field input >= r ZK_ERR_RANGE;
 * a parsed circuit is ZK_ERR_UNSUPPORTED. */
int zk_circuit_weights_mixed(const zk_circuit* c, const uint8_t* in_bits, size_t n_bit_bytes, const uint64_t* in_fields, size_t n_field,
                             uint64_t* weights_out, size_t m);
typedef struct zk_mixgen zk_mixgen;
/* uploads the core tape, the core packs, the tail tape with its constants and the tail's slot -> witness index table; the circuit
 * may be freed afterwards, the context must outlive the generator.  Takes any built circuit, boolean ones included (the tail is then
 * empty and zk_mixgen_run writes the bytes of zk_boolgen_run); a parsed circuit -> ZK_ERR_UNSUPPORTED with text.  Options, read here:
 * "boolgen_group_words" and "boolgen_expand_form" as for zk_boolgen_create; "boolgen_scratch_kib" caps state plus tail scratch, and a
 * word of 64 instances needs (m + 1) x 8 + tail_slots x 64 x 32 bytes: a circuit of which one word does not fit gives ZK_ERR_SIZE
 * naming the option. */
int zk_mixgen_create(zk_ctx* ctx, const zk_circuit* c, zk_mixgen** out);
void zk_mixgen_free(zk_mixgen* g);       /* NULL is a no-op */
/* The witnesses of `count` input sets.  d_in_bits: the ZK_WIRE_BIT inputs, packed as for zk_boolgen_run (bit k = the k-th such input
 * in input order) at d_in_bits + j * in_stride_bytes; d_in_fields: the ZK_WIRE_FIELD inputs, 4 canonical words each, n_field_inputs
 * per instance, instance-major (may be NULL where the circuit has none).  d_weights_out: exactly zk_witgen_run's, count x m x 4 words,
 * canonical, instance-major: zk_prove_batch_submit and zk_qap_check_dev take it unchanged.  All device pointers.  Complete on return.
 * count == 0: ZK_OK, nothing touched.  m not the circuit's or in_stride_bytes < ceil(n_bit_inputs / 8): ZK_ERR_ARG.  A field input
 * whose word pattern is >= r: ZK_ERR_RANGE with text naming the LOWEST such instance, as zk_witgen_run; the output is then
 * unspecified.  The instances run in chunks under the scratch cap and the result does not depend on the chunking. */
int zk_mixgen_run(zk_mixgen* g, const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count, void* d_weights_out,
                  size_t m);
/* wires[i] (witness indices < m of either class: bits, packed wires, tail wires, field inputs) of instance j -> 4 canonical words at
 * d_out_words + (j * n_wires + i) * 4, the layout of zk_boolgen_eval_fields: with wires = 1..l the `inputs` array of zk_verify_batch.
 * Nothing is expanded and nothing else is written.  Errors as zk_mixgen_run; an index >= m: ZK_ERR_ARG. */
int zk_mixgen_eval_fields(zk_mixgen* g, const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count,
                          const uint32_t* wires, size_t n_wires, void* d_out_words);

/* ------------------------------------------------------------------------------------------
 * Poseidon over the BN254 scalar field (csrc/poseidon.hpp, csrc/poseidon.hip): host hash, circuit gadgets, GPU batch hashing and a
 * device-resident Merkle tree.  S-box x^5, state width t = arity + 1, arity 1, 2 or 4; R_F = 8 full rounds, R_P = 56 / 57 / 60
 * partial rounds: circomlib's parameter sets, so digests are those of circom, snarkjs and Semaphore.
 *   hash(inputs): state = [0, inputs...]; per round rho: add C[rho * t + i] to element i; x^5 on every element if rho < 4 or
 *   rho >= 4 + R_P, else on element 0 only; state = M * state.  The digest is element 0 after the last round.
 * C and M are generated in code from the Poseidon paper's Grain LFSR (csrc/poseidon.hpp has the procedure).  Any other arity:
 * ZK_ERR_ARG (with text where the call has a handle that keeps one).
 * ---------------------------------------------------------------------------------------- */
/* One hash on the host, no context.  inputs: arity x 4 canonical words; out: 4 canonical words.  ZK_ERR_ARG: a null pointer, an
 * arity other than 1, 2, 4.  ZK_ERR_RANGE: an input >= r. */
int zk_poseidon_hash(const uint64_t* inputs, size_t arity, uint64_t out[4]);
/* The parameters of one arity, canonical words: *rf = 8, *rp, round_constants[(rf + rp) * t * 4] (C[rho * t + i] at element
 * rho * t + i), mds[t * t * 4] (M[i][j] at element i * t + j), t = arity + 1.  Any pointer may be NULL.  ZK_ERR_ARG: the arity. */
int zk_poseidon_params(size_t arity, unsigned* rf, unsigned* rp, uint64_t* round_constants, uint64_t* mds);
/* `count` hashes on the GPU, one per lane.  d_inputs: count x arity x 4 canonical words, instance-major; d_out: count x 4 canonical
 * words.  Both device pointers, 16-byte aligned.  Complete on return.  count == 0: ZK_OK, nothing touched.  ZK_ERR_ARG: the arity, a
 * null or misaligned pointer.  An input word pattern >= r: ZK_ERR_RANGE, found on the device; zk_last_error names the LOWEST such
 * instance and the contents of d_out are unspecified.  The parameters are uploaded once per context and arity. */
int zk_poseidon_hash_batch(zk_ctx* ctx, const void* d_inputs, size_t arity, size_t count, void* d_out);
/* A binary Merkle tree (arity 2) that stays on the device.  Level 0 is the leaves, level k holds ceil(n_leaves / 2^k) nodes, at
 * least one from level 1 up, level `depth` is the root.  A child that does not exist counts as the zero hash of its level: z_0 = 0,
 * z_{k+1} = hash(z_k, z_k) -- so a tree of depth 20 over 1000 leaves stores about 2000 nodes, not 2^21, and n_leaves == 0 gives
 * root = z_depth.  d_leaves: n_leaves x 4 canonical words on the device (copied; may be NULL when n_leaves == 0).  One kernel launch
 * per level; complete on return.  The context must outlive the tree.  ZK_ERR_ARG with text: depth > 32, n_leaves > 2^depth, a null
 * pointer.  ZK_ERR_RANGE with text naming the lowest such leaf: a leaf >= r.  *out is NULL on every failure.  The tree changes
 * through zk_poseidon_tree_update and zk_poseidon_tree_append below; n_leaves == 0 followed by appends starts a tree that grows. */
typedef struct zk_poseidon_tree zk_poseidon_tree;
int zk_poseidon_tree_build(zk_ctx* ctx, const void* d_leaves, size_t n_leaves, unsigned depth, zk_poseidon_tree** out);
void zk_poseidon_tree_free(zk_poseidon_tree* t);     /* NULL is a no-op */
/* the root, 4 canonical words (kept on the host by zk_poseidon_tree_build, _update and _append) */
int zk_poseidon_tree_root(const zk_poseidon_tree* t, uint64_t out[4]);
/* either pointer may be NULL */
int zk_poseidon_tree_dims(const zk_poseidon_tree* t, size_t* n_leaves, unsigned* depth);
/* downloads the stored nodes of one level to the host: out[size x 4] canonical words, size = n_leaves for level 0 and
 * max(1, ceil(n_leaves / 2^level)) above.  ZK_ERR_ARG with text: level > depth. */
int zk_poseidon_tree_nodes(const zk_poseidon_tree* t, unsigned level, uint64_t* out);
/* Authentication paths of `count` leaves, in the layout zk_mixgen_run reads.  d_indices: count uint64 leaf indices on the device.
 * For instance j, at d_fields_out + j * field_stride_words words: the leaf, then the siblings of levels 0 .. depth - 1,
 * (1 + depth) x 4 canonical words (a sibling the tree does not store is z_k); at d_bits_out + j * bits_stride_bytes bytes: the
 * direction bits, bit k = (index >> k) & 1 (1: the path's node is the RIGHT child at level k), packed as zk_mixgen_run takes bit
 * inputs, ceil(depth / 8) bytes -- the index's own low bytes.  For a circuit whose inputs were created in the order leaf, siblings,
 * directions (zk_builder_merkle_root) the two outputs are d_in_fields and d_in_bits of zk_mixgen_run with no host step between.
 * All device pointers, 8-byte aligned (d_bits_out: any; may be NULL at depth 0).  One gather kernel; complete on return.
 * count == 0: ZK_OK.  ZK_ERR_ARG with text: field_stride_words < (1 + depth) * 4, bits_stride_bytes < ceil(depth / 8), a null
 * pointer.  ZK_ERR_RANGE with text naming the lowest such instance: an index >= n_leaves; the outputs are then unspecified. */
int zk_poseidon_tree_paths(zk_poseidon_tree* t, const void* d_indices, size_t count, void* d_fields_out, size_t field_stride_words,
                           void* d_bits_out, size_t bits_stride_bytes);
/* Sets leaf indices[j] = values[j] for j < count and rehashes every node with a changed leaf under it, up to the root; afterwards the
 * root, every level and every path are what zk_poseidon_tree_build over the edited leaves gives, word for word.  d_indices: count
 * uint64 leaf indices, d_values: count x 4 canonical words, both on the device, 8-byte aligned.  One checking kernel, one scatter and
 * one launch per level over the list of that level's changed nodes, each parent hashed once; on the context's stream, complete on
 * return (the root on the host is refreshed).  count == 0: ZK_OK, nothing touched.  Every refusal is found before anything is written and leaves the tree
 * as it was; where several hold, the first of: ZK_ERR_ARG: a null or misaligned pointer.  ZK_ERR_RANGE with text naming the lowest
 * such instance j: an index >= n_leaves.  ZK_ERR_RANGE with text naming the lowest such instance j: a value >= r.  ZK_ERR_ARG with
 * text naming the lowest such LEAF: an index that occurs more than once in the call, equal values or not -- there is no
 * last-wins rule. */
int zk_poseidon_tree_update(zk_poseidon_tree* t, const void* d_indices, const void* d_values, size_t count);
/* Appends `count` leaves, which become leaves n_leaves .. n_leaves + count - 1; zk_poseidon_tree_dims reports the new size and the
 * tree is what zk_poseidon_tree_build over all the leaves gives.  d_leaves: count x 4 canonical words on the device, 8-byte aligned
 * (copied).  The node buffer has a capacity that at least doubles when an append exceeds it (the levels are copied device to
 * device), so a run of small appends copies a linear total.  One checking kernel and one launch per level over the nodes above the
 * new leaves; complete on return.  count == 0: ZK_OK.  Every refusal leaves the tree as it was: ZK_ERR_ARG with text:
 * n_leaves + count > 2^depth, a null or misaligned pointer.  ZK_ERR_RANGE with text naming the lowest such position in d_leaves: a
 * leaf >= r. */
int zk_poseidon_tree_append(zk_poseidon_tree* t, const void* d_leaves, size_t count);

/* ------------------------------------------------------------------------------------------
 * Baby Jubjub (csrc/babyjub.hpp, csrc/babyjub.hip): the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over the BN254 scalar field
 * with a = 168700, d = 168696 -- circomlib's, iden3's and Semaphore's curve.  The identity is (0, 1); Base8 generates the subgroup of
 * prime order l (251 bits), Generator the whole group of order 8 l, Base8 = 8 Generator.  a is a square and d is not, so the addition
 * law is complete and no point is a special case.  A point is 8 canonical words, x then y.  Refusals: a coordinate >= r is
 * ZK_ERR_RANGE, and so is a point off the curve -- the status zk_crs_upload gives a CRS point off its curve; the range check comes first.
 * ---------------------------------------------------------------------------------------- */
/* a, d, the order l of Base8, Base8 and Generator as canonical words.  Any pointer may be NULL.  Always ZK_OK. */
int zk_babyjub_params(uint64_t a[4], uint64_t d[4], uint64_t order[4], uint64_t base8[8], uint64_t generator[8]);
/* 1: p is on the curve, 0: it is not.  ZK_ERR_ARG: a null pointer.  ZK_ERR_RANGE: a coordinate >= r. */
int zk_babyjub_on_curve(const uint64_t p[8]);
/* out = p + q on the host, no context; out may alias p or q.  ZK_ERR_ARG: a null pointer.  ZK_ERR_RANGE: see above. */
int zk_babyjub_add(const uint64_t p[8], const uint64_t q[8], uint64_t out[8]);
/* out = [scalar] p on the host, no context; p == NULL means Base8.  The scalar is an integer of 256 bits, taken as an integer and NOT
 * reduced (points outside the subgroup of order l see the difference).  ZK_ERR_ARG: scalar or out null.  ZK_ERR_RANGE: see above. */
int zk_babyjub_mul(const uint64_t scalar[4], const uint64_t* p, uint64_t out[8]);
/* `count` scalar multiplications on the GPU, one per lane: instance j computes [scalars[j]] points[j], or [scalars[j]] Base8 where
 * d_points is NULL.  d_scalars: count x 4 words, any 256-bit integers; d_points: count x 8 canonical words; the result, affine and
 * canonical (x, y), goes to the 8 words at d_out + j * out_stride_words (words of 64 bits) and nothing else is written.
 * out_stride_words 0 or 8: packed, which is d_inputs of zk_poseidon_hash_batch(ctx, d_out, 2, count, ...); a larger stride lands a
 * result inside a row of zk_mixgen_run's d_in_fields.  All device pointers, 8-byte aligned.  Complete on return.  count == 0: ZK_OK,
 * nothing touched.  Fixed base: additions only, over a table of j 16^k Base8 (ZK_BABYJUB_FIXED_WINDOW bits a window) uploaded once
 * per context.  Variable base: windows of ZK_BABYJUB_VAR_WINDOW bits over P, 2 P, 3 P in registers.  Both kernels run the same
 * instruction stream in every lane whatever the scalars and points.  ZK_ERR_ARG with text: a null or misaligned pointer, a stride in
 * 1..7.  Variable base only, found on the device BEFORE anything is written, d_out untouched, the text naming the LOWEST such
 * instance: a coordinate >= r (ZK_ERR_RANGE); if there is none, a point off the curve (ZK_ERR_RANGE). */
#define ZK_BABYJUB_FIXED_WINDOW 4
#define ZK_BABYJUB_VAR_WINDOW 2
int zk_babyjub_mul_batch(zk_ctx* ctx, const void* d_scalars, const void* d_points, size_t count, void* d_out, size_t out_stride_words);

/* ------------------------------------------------------------------------------------------
 * EdDSA-Poseidon on Baby Jubjub (csrc/eddsa.hpp, csrc/eddsa.hip).  The scheme, the same in every layer:
 *   curve, generator     those above; l is the order of Base8
 *   secret key           a scalar k, 0 < k < l;  public key A = [k] Base8;  nonce key: a field element n < r
 *   H6(a, b, c, d, e)    Poseidon of width 6 over the state [0, a, b, c, d, e]: R_F = 8, R_P = 60, x^5, element 0 is the digest; the
 *                        round structure and the Grain procedure of the three public widths.  H6(1, 2, 3, 4, 5) =
 *                        0x0dab9449e4a1398a15224c0b15a49d598b2174d305a316c918125f8feeb123c0, the value circomlibjs and
 *                        go-iden3-crypto publish.  Width 6 is reachable through the zk_eddsa_* calls only: zk_poseidon_* refuse arity 5.
 *   Sign(k, n, M), M < r rho = H6(n, M, 0, 0, 0) mod l;  R8 = [rho] Base8;  hm = H6(R8.x, R8.y, A.x, A.y, M);  S = (rho + 8 hm k) mod l.
 *                        The signature is (R8, S), 12 words.  Signing is deterministic.
 *   Verify(A, M, R8, S)  valid when all six words of A, R8, M, S are canonical (< r), A and R8 are on the curve, S < l, and
 *                        [S] Base8 = R8 + [8] ([hm] A) with hm taken as the full integer below r, NOT reduced mod l.  8 hm can reach
 *                        2^257: [hm] A is computed and doubled three times; 8 hm is never a scalar.
 * This is the equation of circomlibjs' verifyPoseidon: a signature made by circomlib verifies here, its key given as k = pruned >> 3.
 * Not offered: circomlib's key derivation from 32 bytes by Blake-512 (its rho comes from Blake-512, ours from H6; a verifier cannot
 * tell), and a rejection of keys of small order: with A = (0, 1) every S with R8 = [S] Base8 is valid, as in verifyPoseidon.
 * One status per signature, the lowest applicable: */
#define ZK_EDDSA_VALID 0
#define ZK_EDDSA_RANGE 1           /* a word pattern of A, R8, M or S is >= r */
#define ZK_EDDSA_KEY_OFF_CURVE 2
#define ZK_EDDSA_R_OFF_CURVE 3
#define ZK_EDDSA_S_RANGE 4         /* S >= l */
#define ZK_EDDSA_MISMATCH 5
/* out = H6(r8.x, r8.y, a.x, a.y, msg) on the host, no context.  A range check only and deliberately NO curve check: any five elements
 * hash.  ZK_ERR_ARG: a null pointer.  ZK_ERR_RANGE: a word pattern >= r. */
int zk_eddsa_challenge(const uint64_t r8[8], const uint64_t a[8], const uint64_t msg[4], uint64_t out[4]);
/* out = [k] Base8.  ZK_ERR_ARG: a null pointer.  ZK_ERR_RANGE: k == 0 or k >= l. */
int zk_eddsa_public_key(const uint64_t k[4], uint64_t out[8]);
/* (r8_out, s_out) = Sign(k, nonce_key, msg) on the host, no context; k, rho and the nonce key are wiped from the call's locals before
 * it returns.  ZK_ERR_ARG: a null pointer.  ZK_ERR_RANGE: k == 0, k >= l, nonce_key >= r or msg >= r; nothing is written then. */
int zk_eddsa_sign(const uint64_t k[4], const uint64_t nonce_key[4], const uint64_t msg[4], uint64_t r8_out[8], uint64_t s_out[4]);
/* *status = ZK_EDDSA_* for one signature on the host, no context.  Returns ZK_OK for every signature: a malformed one is a verdict, not
 * an error.  ZK_ERR_ARG: a null pointer. */
int zk_eddsa_verify(const uint64_t a[8], const uint64_t msg[4], const uint64_t r8[8], const uint64_t s[4], int* status);
/* `count` verdicts on the GPU, one signature per lane.  d_points_msg: count x 20 words, (A.x, A.y, R8.x, R8.y, M) per signature --
 * the five ZK_WIRE_FIELD inputs of zk_builder_eddsa_verify's circuit in zk_mixgen_run's d_in_fields layout; d_s: count x 4 words;
 * d_status: count x uint32, ZK_EDDSA_*.  d_bits_out may be NULL; otherwise row j, at d_bits_out + j * bits_stride_bytes, receives 64
 * bytes: the 251 low bits of S, then the 254 bits of hm, least significant first, then 7 zero bits -- zk_mixgen_run's d_in_bits for a
 * circuit whose bit inputs were made in that order -- and bytes of a row past the 64th are not written.  A row is all zero where the
 * status is ZK_EDDSA_RANGE.  The chain zk_eddsa_verify_batch -> zk_mixgen_run -> zk_prove_batch_submit runs device to device.
 * Two launches: the range, curve and S < l checks with H6 (32 bytes a signature in a context buffer), then [hm] A by windows of 2
 * bits in registers, three doublings, + R8, [S] Base8 over the table of zk_babyjub_mul_batch, and the comparison by cross
 * multiplication: no inversion, no LDS.  Every lane runs the same instruction stream whatever its data; a defective signature
 * changes its own status only.  All device pointers, 8-byte aligned (d_status: 4-byte).  Complete on return.  count == 0: ZK_OK,
 * nothing touched.  ZK_ERR_ARG with text: a null or misaligned pointer; with d_bits_out, a stride below 64 or no multiple of 8.
 * Per-signature defects are statuses and never refuse the call. */
int zk_eddsa_verify_batch(zk_ctx* ctx, const void* d_points_msg, const void* d_s, size_t count, void* d_status, void* d_bits_out,
                          size_t bits_stride_bytes);
/* `count` signatures on the GPU, one per lane: instance j is signed exactly as zk_eddsa_sign(k_j, n_j, M_j) signs it (the scheme
 * above).  d_keys, d_nonce_keys, d_msgs: count x 4 words each, k, n and M of instance j.  d_points_msg_out: count x 20 words,
 * (A.x, A.y, R8.x, R8.y, M) per instance -- d_points_msg of zk_eddsa_verify_batch and d_in_fields of the gadget's circuit.  A = [k] Base8
 * is computed in the call and never taken from the caller: signing under a public key that is not the key's own leaks k.  d_s_out:
 * count x 4 words, S -- d_s of zk_eddsa_verify_batch.  d_bits_out may be NULL; otherwise row j, at d_bits_out + j *
 * bits_stride_bytes, receives the 64 bytes zk_eddsa_verify_batch writes there: the 251 bits of S, then the 254 bits of hm as the full
 * integer below r, least significant first, then 7 zero bits; bytes of a row past the 64th are not written.  With it the chain
 * zk_eddsa_sign_batch -> zk_mixgen_run -> zk_prove_batch_submit runs with no verify call and no host step.  Every word written equals
 * what zk_eddsa_public_key, zk_eddsa_sign and zk_eddsa_challenge give on the host.
 * Three launches: the range checks with rho = H6(n, M, 0, 0, 0) mod l; A and R8 by two walks over the table of zk_babyjub_mul_batch
 * and ONE Fermat inversion for both; hm = H6(R8, A, M) and S = (rho + 8 (hm mod l) k) mod l (arithmetic mod l: csrc/eddsa_modl.hpp).
 * No LDS.  Secrets: rho lives in a context buffer (32 bytes an instance) between the launches; the last launch that reads it
 * overwrites it with zeros, and a refused call wipes what it wrote there.  k is read from the caller's array and kept nowhere else.
 * The instruction stream is the same in every lane whatever the data -- no lane returns early, no loop bound or branch depends on
 * a secret -- but, as in the fixed-base kernel of zk_babyjub_mul_batch, the table entry is addressed by four bits of a secret scalar
 * (k, then rho): the addresses a lane reads depend on its secrets.
 * All device pointers, 8-byte aligned.  Complete on return.  count == 0: ZK_OK, nothing touched.  Refusals are those of
 * zk_babyjub_mul_batch, not statuses: a bad secret key is the caller's error, not a verdict.  ZK_ERR_ARG with text: a null or
 * misaligned pointer; with d_bits_out, a stride below 64 or no multiple of 8.  ZK_ERR_RANGE, found on the device BEFORE anything is
 * written to the three outputs, the text naming the LOWEST such instance and which input it is -- within one instance the key, then
 * the nonce key, then the message: k == 0, k >= l, n >= r, M >= r. */
int zk_eddsa_sign_batch(zk_ctx* ctx, const void* d_keys, const void* d_nonce_keys, const void* d_msgs, size_t count,
                        void* d_points_msg_out, void* d_s_out, void* d_bits_out, size_t bits_stride_bytes);

/* ------------------------------------------------------------------------------------------
 * CRS  (SigmaG1 / SigmaG2, groth16/mod.rs:105-121)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    size_t n, m, input;
    const uint64_t *alpha_g1, *beta_g1, *delta_g1;   /* 8 words each */
    const uint64_t* xi_g1;          /* n       points  [x^i]_1            */
    const uint64_t* sum_gamma_g1;   /* input+1 points  (wires 0..l)       */
    const uint64_t* sum_delta_g1;   /* m-l-1   points  (wires l+1..m-1)   */
    const uint64_t* xi_t_g1;        /* n-1     points  [x^i t(x)/delta]_1 */
    const uint64_t *beta_g2, *gamma_g2, *delta_g2;   /* 16 words each */
    const uint64_t* xi_g2;          /* n       points  [x^i]_2            */
} zk_crs_desc;
int zk_crs_upload(zk_ctx* ctx, const zk_crs_desc* desc, zk_crs** out);

/* groth16::setup (groth16/mod.rs:134-197) on the GPU with the five random draws injected:
 * trapdoor = alpha | beta | gamma | delta | x (4 canonical words each).  Every element is non-zero and < r: a zero element gives
 * ZK_ERR_DIV_BY_ZERO (Random for FrLocal never yields one, fr.rs:90-99), an element >= r ZK_ERR_RANGE; *out is NULL on every failure
 * and the context and the QAP stay usable.
 * x on a root of t:
 *   - integer-roots form (zk_qap_upload_sparse_integers): x in 1..2n-1 -- the roots 1..n and the second node set n+1..2n-1 of the
 *     Lagrange-basis H points -- gives ZK_ERR_UNSUPPORTED (draw another x); 2n and everything above is accepted;
 *   - arbitrary-roots form (zk_qap_upload_sparse_roots): x equal to one of the roots gives ZK_ERR_UNSUPPORTED;
 *     (the reference would emit a CRS in both cases: a deliberate deviation)
 *   - roots-of-unity form (zk_qap_upload_sparse) and dense form: accepted, and the CRS is the reference's for that x: t(x) = 0, so
 *     every xi_t_g1 point is infinity, and so is every sum_gamma / sum_delta point of a wire with no entry at the gate at x.  On
 *     such a CRS zk_verify checks the gate at x only: a witness that fails any other gate proves and verifies.  Never use one
 *     outside tests. */
int zk_setup(zk_ctx* ctx, const zk_qap* qap, const uint64_t trapdoor[20], zk_crs** out);

/* Copy a device CRS back into caller-provided host buffers (any pointer may be NULL = skip). */
typedef struct {
    uint64_t *alpha_g1, *beta_g1, *delta_g1, *xi_g1, *sum_gamma_g1, *sum_delta_g1, *xi_t_g1;
    uint64_t *beta_g2, *gamma_g2, *delta_g2, *xi_g2;
} zk_crs_out;
int zk_crs_dims(const zk_crs* crs, size_t* n, size_t* m, size_t* input);
int zk_crs_download(zk_ctx* ctx, const zk_crs* crs, const zk_crs_out* out);
void zk_crs_free(zk_crs* crs);

/* Is this CRS a Groth16 CRS for THIS QAP?  zk_crs_upload and zk_crs_load take arrays from anywhere (a ceremony, the reference, a file,
 * another machine) and check ranges, curves and the G2 subgroup only; a wrong sum_delta point, an xi_t array off by one power or the
 * CRS of another circuit of the same dimensions still yields 259 well-formed bytes that zk_verify rejects.  This is the check a
 * receiver of a CRS runs once, without the trapdoor (what bellman's phase-2 verify and `snarkjs zkey verify` do): a handful of inner
 * products over the resident arrays and fewer than twenty pairings.
 * Notation: G = xi_g1[0], H = xi_g2[0]; s = the challenge, 1 <= s < r; rho_k = s^k; t(X) = X t'(X) + t_0 (deg t' = n - 1; roots of
 * unity: t' = X^(n-1), t_0 = -1); sums run over the CRS's own arrays.  A relation that does not hold sets its bit in out->failed:
 *   GENERATORS   xi_g1[0] and xi_g2[0] are the bases zk_setup encrypts with (69 G1::one(), 96 G2::one(): fr.rs:106-113).
 *   POWERS_G1    (n >= 2) P = sum_{k<=n-2} rho_k xi_g1[k], Q = sum_{k<=n-2} rho_k xi_g1[k+1]:  e(P, xi_g2[1]) = e(Q, H).
 *   POWERS_G2    e(sum_{k<n} rho_k xi_g1[k], H) = e(G, sum_{k<n} rho_k xi_g2[k]).
 *   TWINS        e(beta_g1, H) = e(G, beta_g2) and e(delta_g1, H) = e(G, delta_g2).
 *   XI_T         (n >= 2) e(sum_{k<=n-2} rho_k xi_t_g1[k], delta_g2) = e(Q, [t'(x)]_2) e(t_0 P, H), [t'(x)]_2 = sum_j t'_j xi_g2[j]
 *                (the CRS holds n powers, so [t(x)] itself cannot be formed in either group: hence the split of t).
 *   WIRES        rho_i = s^i over ALL wires i < m; U = [sum_i rho_i u_i(x)]_1, V = [sum_i rho_i v_i(x)]_2, W = [sum_i rho_i w_i(x)]_1
 *                formed from xi_g1 / xi_g2:  e(sum_{i<=l} rho_i sum_gamma_g1[i], gamma_g2) e(sum_{i>l} rho_i sum_delta_g1[i-l-1], delta_g2)
 *                = e(U, beta_g2) e(alpha_g1, V) e(W, H).  One relation for both arrays; only when it fails it is repeated over the
 *                wires i <= l alone and over the rest, and WIRES_GAMMA / WIRES_DELTA (or both) say which array to look at.
 *   LAGRANGE     (only with ZK_CRS_CHECK_LAGRANGE_PRESENT) S_d(z) = sum_{k<d} (s z)^k:  sum_k S_n(k+1) lag1[k] = sum_{k<n} rho_k xi_g1[k],
 *                the same for lag2 against xi_g2, and sum_j S_{n-1}(n+1+j) lagS_t1[j] = sum_{k<=n-2} rho_k xi_t_g1[k] -- point
 *                equalities, no pairing (lag1, lag2, lagS_t1: the Lagrange-basis arrays zk_setup makes for an integer-roots QAP and a
 *                ZKCRSv2 file carries).
 *   DEGENERATE   gamma_g2, delta_g2, delta_g1, alpha_g1, beta_g1 or beta_g2 is the point at infinity.
 * out->flags: ZK_CRS_CHECK_LAGRANGE_PRESENT, and ZK_CRS_CHECK_T_ZERO when xi_t_g1[0] is infinity: x is a root of t, every relation
 * holds and the CRS is consistent but UNSOUND (see zk_setup).  "The CRS is good" means failed == 0 && !(flags & ZK_CRS_CHECK_T_ZERO).
 * What a good CRS is: the CRS of SOME trapdoor (alpha, beta, gamma, delta, x) for this QAP.  x is known to nobody, so that is the whole
 * claim; a CRS byte-equal to zk_setup's for any trapdoor passes for every challenge.
 * Soundness: each relation is a polynomial identity in s of degree below max(n, m); one wrong entry makes the polynomial
 * non-zero, so at most max(n, m) of the r values of s let it pass: error <= 2^23 / r -- for an s the maker of the CRS could NOT
 * PREDICT.  Knowing s, two entries of one array can be altered so that they cancel (xi_t[0] += D, xi_t[1] -= D / s).  So, as for the
 * z_j of zk_verify_batch_all: a fixed `challenge` is for tests; challenge = NULL draws 256 bits from the OS and reduces them mod r.
 *  - All four QAP forms (zk_qap_kind 0..3) and every CRS however it arrived (zk_setup, zk_crs_upload, zk_crs_load of either version).
 *  - Read-only on the CRS: the prover's window tables are neither built, used nor replaced and no Lagrange-basis array is attached; a
 *    proof made before the check and one made after it are byte-equal.  On the QAP handle the first check builds what the first
 *    zk_qap_check builds (W's rows by gate) and, for the integer-roots form, the interpolation tree of 1..n.
 *  - Synchronous, on a stream of its own; an outstanding zk_prove_submit ticket is not disturbed (the one-off tables of the check are
 *    freed before the call returns, which lets the device drain first).  Device memory: the window tables of the five arrays, about
 *    what the prover's tables take.
 *  - ZK_ERR_ARG: null ctx / crs / qap / out, a CRS whose (n, m, input) differ from the QAP's, a handle of another context,
 *    challenge = 0.  ZK_ERR_RANGE: challenge >= r.  On every error *out is untouched. */
#define ZK_CRS_CHECK_GENERATORS 0x001u
#define ZK_CRS_CHECK_POWERS_G1 0x002u
#define ZK_CRS_CHECK_POWERS_G2 0x004u
#define ZK_CRS_CHECK_TWINS 0x008u
#define ZK_CRS_CHECK_XI_T 0x010u
#define ZK_CRS_CHECK_WIRES 0x020u
#define ZK_CRS_CHECK_WIRES_GAMMA 0x040u
#define ZK_CRS_CHECK_WIRES_DELTA 0x080u
#define ZK_CRS_CHECK_LAGRANGE 0x100u
#define ZK_CRS_CHECK_DEGENERATE 0x200u
#define ZK_CRS_CHECK_T_ZERO 1u             /* flags */
#define ZK_CRS_CHECK_LAGRANGE_PRESENT 2u   /* flags */
typedef struct {
    uint32_t failed;   /* ZK_CRS_CHECK_GENERATORS .. ZK_CRS_CHECK_DEGENERATE: the relations that do not hold */
    uint32_t flags;    /* ZK_CRS_CHECK_T_ZERO | ZK_CRS_CHECK_LAGRANGE_PRESENT */
} zk_crs_check_result;
int zk_crs_check(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const uint64_t challenge[4] /* NULL = drawn from the OS */,
                 zk_crs_check_result* out);

/* A delta contribution: the other half of the workflow zk_crs_check belongs to (bellman's phase 2, `snarkjs zkey contribute`).  A
 * party that receives a CRS multiplies delta by a secret factor d of its own: delta' = d delta.  Whoever ran zk_setup then no longer
 * knows delta', and nobody has to trust them or run a whole setup again: one honest contributor in a chain is enough.
 * zk_crs_contribute makes, on the same context, the CRS zk_setup would have made for the trapdoor (alpha, beta, gamma, delta d, x)
 * -- byte for byte, for all four QAP forms:
 *   delta_g1' = d delta_g1, delta_g2' = d delta_g2 (two points, host code);
 *   sum_delta_g1' = d^-1 sum_delta_g1, xi_t_g1' = d^-1 xi_t_g1 and, when the source carries the Lagrange-basis arrays,
 *   lagS_t1' = d^-1 lagS_t1: every point of a resident array times ONE scalar (k_g1_scale, csrc/crs_contribute.hip: the scalar is
 *   split and recoded once on the host, every lane walks the same digits, four points share an inversion);
 *   every other array (lag1 and lag2 included) is copied device to device.  The new CRS has no window tables: its first proof builds
 *   them, as after zk_crs_upload.  zk_crs_save writes it as ZKCRSv1 / ZKCRSv2 like any CRS.
 *  - d: canonical, 1 <= d < r; NULL draws it from the OS -- it is then never returned, and d, d^-1, the nonce and the recoded digits
 *    are wiped before the call returns.  d = 0: ZK_ERR_DIV_BY_ZERO; d >= r: ZK_ERR_RANGE.  d = 1 gives an equal CRS.
 *  - The source is read only (its tables and arrays are neither touched nor rebuilt): proofs over it before and after the call are
 *    byte-equal, and an outstanding zk_prove_submit ticket is not disturbed.  Synchronous, on a stream of its own, complete on return.
 *  - ZK_ERR_ARG: a null pointer (tag and d excepted) or a CRS of another context.  On every failure *out is NULL and *contribution is
 *    untouched.
 * The record is a Schnorr proof of knowledge of d, so that a contributor cannot merely cancel the contributions before theirs, bound
 * to a 32-byte tag of the caller's (the hash of the transcript so far, or of whatever the ceremony publishes; NULL = 32 zero bytes):
 *   T = k delta_before (k: a nonce from the OS),  c = SHA-256("ZKCONTRv1\0" | tag | delta_before | delta_after | T) read as a
 *   big-endian integer and reduced mod r,  z = k + c d mod r;  it verifies iff z delta_before = T + c delta_after.
 * A point enters the hash as its 64 bytes: the eight canonical little-endian words, x then y.  The struct's memory image (224 bytes,
 * little-endian words) is its byte form.  zk_crs_contribution_prove / _verify are host code and take no context (as zk_vk_verify /
 * zk_pairing).  prove: `nonce` NULL = drawn from the OS; a fixed nonce is for tests ONLY (two records with one nonce reveal d).
 * ZK_ERR_RANGE for d or nonce >= r or a delta_before that is out of range, off the curve or infinity, ZK_ERR_DIV_BY_ZERO for d = 0.
 * verify: a malformed field (coordinate >= q, off-curve point, response >= r, infinity delta_before or delta_after) gives *ok = 0
 * with ZK_OK, like any record that does not verify. */
typedef struct {
    uint64_t delta_before_g1[8], delta_after_g1[8];   /* canonical affine */
    uint64_t commit_g1[8];                            /* T = k * delta_before_g1 */
    uint64_t response[4];                             /* z = k + c d mod r */
} zk_crs_contribution;
int zk_crs_contribution_prove(const uint64_t delta_before_g1[8], const uint64_t d[4], const uint64_t nonce[4] /* NULL = OS; fixed: tests only */,
                              const uint8_t tag[32] /* NULL = 32 zero bytes */, zk_crs_contribution* out);
int zk_crs_contribution_verify(const zk_crs_contribution* c, const uint8_t tag[32], int* ok);
int zk_crs_contribute(zk_ctx* ctx, const zk_crs* crs, const uint64_t d[4] /* NULL = drawn from the OS, wiped, never returned */,
                      const uint8_t tag[32], zk_crs** out, zk_crs_contribution* contribution);

/* Is `after` the CRS `before` with only delta re-keyed, by someone who knew the factor?  A bit of out->failed per relation that
 * does not hold (G = xi_g1[0], H = xi_g2[0] of `after`; rho_i = s^i over an array's own indices, s the challenge as in zk_crs_check):
 *   UNCHANGED    alpha_g1, beta_g1, beta_g2, gamma_g2, xi_g1, xi_g2, sum_gamma_g1 are word for word the same (one compare kernel).
 *   RECORD       the record's delta_before_g1 / delta_after_g1 are the two CRSs' delta_g1.
 *   KNOWLEDGE    zk_crs_contribution_verify accepts the record for this tag.
 *   DELTA_TWINS  e(delta_g1', H) = e(G, delta_g2').
 *   SUM_DELTA    e(sum_i rho_i sum_delta_g1'[i], delta_g2') = e(sum_i rho_i sum_delta_g1[i], delta_g2).
 *   XI_T         (n >= 2) the same over xi_t_g1.
 *   DEGENERATE   delta_g1' or delta_g2' is infinity.
 * Six pairings on the host; the random sums go through the MSM launcher over one-off tables on a stream of the call's own; both
 * CRSs are read only.  The Lagrange-basis arrays are NOT looked at: zk_crs_check(after, qap) ties them to xi_g1, xi_g2 and xi_t_g1
 * through its LAGRANGE relation.  "after is a valid successor of before" means failed == 0; "after is a good CRS" is then
 * zk_crs_check(before, qap) once, for the head of the chain (the relations of zk_crs_check are invariant under delta -> d delta with
 * sum_delta and xi_t divided by d, which is exactly what failed == 0 establishes).
 * Soundness: as for zk_crs_check -- SUM_DELTA and XI_T are polynomial identities in s of degree below max(n, m), error <= max(n, m) / r
 * for an s the maker of `after` could not predict; a fixed `challenge` is for tests, NULL draws 256 bits from the OS.
 * ZK_ERR_ARG: a null pointer (tag and challenge excepted), CRSs that differ in (n, m, input), a handle of another context,
 * challenge = 0.  ZK_ERR_RANGE: challenge >= r.  On every error *out is untouched. */
#define ZK_CONTRIB_UNCHANGED 0x01u
#define ZK_CONTRIB_RECORD 0x02u
#define ZK_CONTRIB_KNOWLEDGE 0x04u
#define ZK_CONTRIB_DELTA_TWINS 0x08u
#define ZK_CONTRIB_SUM_DELTA 0x10u
#define ZK_CONTRIB_XI_T 0x20u
#define ZK_CONTRIB_DEGENERATE 0x40u
typedef struct {
    uint32_t failed;   /* ZK_CONTRIB_UNCHANGED .. ZK_CONTRIB_DEGENERATE: the relations that do not hold */
    uint32_t flags;    /* reserved, 0 */
} zk_crs_contribution_result;
int zk_crs_contribution_check(zk_ctx* ctx, const zk_crs* before, const zk_crs* after, const zk_crs_contribution* c, const uint8_t tag[32],
                              const uint64_t challenge[4] /* NULL = OS */, zk_crs_contribution_result* out);

/* The head of such a chain WITHOUT a trapdoor: derive the circuit's CRS from a universal powers-of-tau transcript by group operations
 * only (what bellman's MPCParameters::new and `snarkjs zkey new` do), with gamma = delta = 1.  zk_setup takes (alpha, beta, gamma,
 * delta, x) as an argument, so whoever runs it knows x, alpha and beta for good, and a delta contribution removes delta only.
 * The result is the CRS zk_setup(qap, (alpha, beta, 1, 1, x)) would make -- byte for byte in every array zk_crs_download returns and,
 * for the integer-roots form, in the Lagrange-basis arrays a ZKCRSv2 file carries -- for the (alpha, beta, x) of the transcript:
 *   alpha_g1 = alpha_tau_g1[0], beta_g1 = beta_tau_g1[0], beta_g2 copied; delta_g1 = tau_g1[0]; gamma_g2 = delta_g2 = tau_g2[0];
 *   xi_g1 = tau_g1[0..n), xi_g2 = tau_g2[0..n);
 *   wire i: sum_j u_ij [beta L_j]_1 + v_ij [alpha L_j]_1 + w_ij [L_j]_1 (L_j: the Lagrange polynomial of gate j), wires 0..l to
 *   sum_gamma_g1 and the rest to sum_delta_g1 (k_wire_points, csrc/crs_from_powers.hip: a sparse matrix times a vector of points);
 *   xi_t_g1[k] = [x^k t(x)]_1, k <= n - 2.
 * QAP forms:
 *   roots of unity (zk_qap_upload_sparse)            the three arrays [L_j], [alpha L_j], [beta L_j] are inverse transforms over n points
 *                                                    of tau_g1, alpha_tau_g1, beta_tau_g1; xi_t_g1[k] = tau_g1[n + k] - tau_g1[k].
 *   integer roots (zk_qap_upload_sparse_integers)    the three arrays come from the transposed interpolation tree (csrc/gbasis.hip);
 *                                                    xi_t_g1[k] = sum_{j<=n} t_j tau_g1[k + j], a cyclic convolution of 2^ceil(log2(2n-1))
 *                                                    points; the Lagrange-basis arrays of the result are attached (n <= 2^22).
 *   arbitrary roots, dense                           ZK_ERR_UNSUPPORTED (zk_last_error says which form was given).
 * Points are canonical affine host arrays as in zk_crs_desc; the point at infinity (all words zero) is accepted anywhere.  Powers
 * beyond the first 2n - 1 of tau_g1 and the first n of the other arrays are ignored.
 * The call does NOT check that the arrays are a powers-of-tau sequence (tau_g1[k+1] = x tau_g1[k], the same x in G2, alpha and beta
 * the same in every entry): run zk_crs_check(result, qap), which covers every array derived here (POWERS_G1, POWERS_G2, TWINS, XI_T,
 * WIRES, LAGRANGE), before anyone contributes to or proves with the result -- or check the transcript itself, once for all circuits
 * and over every power it holds, with zk_powers_check below.
 *  - Synchronous, on a stream of its own; an outstanding zk_prove_submit ticket is not disturbed.  The new CRS has no window tables:
 *    its first proof builds them, as after zk_crs_upload.
 *  - ZK_ERR_ARG: a null pointer (arrays of the desc included), a QAP of another context, n_tau_g1 < 2n - 1, n_rest < n.
 *    ZK_ERR_RANGE: a coordinate >= q, a point off its curve, a G2 point outside the subgroup of order r (zk_crs_upload's statuses).
 *    On every failure *out is NULL and the context and the QAP stay usable. */
typedef struct {
    size_t n_tau_g1;               /* number of tau_g1 points, >= 2n-1 for a QAP of n gates */
    size_t n_rest;                 /* number of points in each of the other three arrays, >= n */
    const uint64_t* tau_g1;        /* [x^k]_1        k < n_tau_g1 */
    const uint64_t* tau_g2;        /* [x^k]_2        k < n_rest   */
    const uint64_t* alpha_tau_g1;  /* [alpha x^k]_1  k < n_rest   */
    const uint64_t* beta_tau_g1;   /* [beta  x^k]_1  k < n_rest   */
    const uint64_t* beta_g2;       /* [beta]_2 */
} zk_powers_desc;
int zk_crs_from_powers(zk_ctx* ctx, const zk_qap* qap, const zk_powers_desc* powers, zk_crs** out);

/* Phase 1: the transcript itself (bellman's `powersoftau`, `snarkjs powersoftau contribute` / `verify`).  zk_crs_from_powers takes
 * whatever arrays it is given; the calls below check a universal transcript ONCE (not per circuit, and over every power, used or not),
 * add a party's own randomness to it, and check that others did so knowingly -- so that x, alpha and beta are known to nobody as long
 * as one contributor of the chain was honest.  A zk_powers is the five arrays of zk_powers_desc resident on the device (affine,
 * Montgomery form, as the arrays of a CRS).
 *  - zk_powers_upload: the range, curve and G2-subgroup checks and statuses of zk_crs_from_powers; n_rest >= 2 and n_tau_g1 >= n_rest
 *    (anything else: ZK_ERR_ARG).  Infinity entries are accepted here; zk_powers_check flags them.
 *  - zk_powers_initial: the head of a ceremony, x = alpha = beta = 1: every G1 entry is the library's generator G (xi_g1[0] of any
 *    zk_setup CRS), every G2 entry and beta_g2 its generator H.
 *  - zk_powers_download: canonical affine words into caller buffers, any pointer may be NULL (as zk_crs_download).  The arrays can be
 *    handed to zk_crs_from_powers as a zk_powers_desc.
 * On every failure of upload / initial *out is NULL. */
typedef struct zk_powers zk_powers;
typedef struct {
    uint64_t *tau_g1, *tau_g2, *alpha_tau_g1, *beta_tau_g1, *beta_g2;
} zk_powers_out;
int zk_powers_upload(zk_ctx* ctx, const zk_powers_desc* desc, zk_powers** out);
int zk_powers_initial(zk_ctx* ctx, size_t n_tau_g1, size_t n_rest, zk_powers** out);
int zk_powers_dims(const zk_powers* powers, size_t* n_tau_g1, size_t* n_rest);
int zk_powers_download(zk_ctx* ctx, const zk_powers* powers, const zk_powers_out* out);
void zk_powers_free(zk_powers* powers);

/* Are these arrays a powers-of-tau transcript?  A bit of out->failed per relation that does not hold.  G = tau_g1[0], H = tau_g2[0],
 * N1 = n_tau_g1, N2 = n_rest, rho_k = c^k for the challenge c:
 *   GENERATORS   G and H are the library's generators.
 *   POWERS_G1    P = sum_{k<=N1-2} rho_k tau_g1[k], Q = sum_{k<=N1-2} rho_k tau_g1[k+1]:  e(P, tau_g2[1]) = e(Q, H).
 *   POWERS_G2    e(sum_{k<N2} rho_k tau_g1[k], H) = e(G, S2),  S2 = sum_{k<N2} rho_k tau_g2[k]  (one G2 sum for this and the next two).
 *   ALPHA        e(sum_{k<N2} rho_k alpha_tau_g1[k], H) = e(alpha_tau_g1[0], S2).
 *   BETA         the same over beta_tau_g1.
 *   BETA_TWINS   e(beta_tau_g1[0], H) = e(G, beta_g2).
 *   DEGENERATE   tau_g1[1], tau_g2[1], alpha_tau_g1[0], beta_tau_g1[0] or beta_g2 is infinity (x, alpha or beta is 0).
 * With GENERATORS, POWERS_G1 says tau_g1[k] = x^k G for the x of tau_g2[1]; POWERS_G2 carries the same x^k to tau_g2; ALPHA and BETA
 * say the entries are alpha x^k, beta x^k for ONE alpha, ONE beta.  The sums go through the MSM launcher over one-off tables on a
 * stream of the call's own (freed before return); about a dozen pairings on the host.  The handle is read only; synchronous; an
 * outstanding zk_prove_submit ticket is not disturbed.
 * Soundness: each relation is a polynomial identity in c of degree below N1, so a transcript that violates one passes with
 * probability below N1 / r over a challenge its maker could not predict.  NULL draws 256 bits from the OS; a fixed challenge is for
 * tests ONLY.
 * ZK_ERR_ARG: a null pointer (challenge excepted), a handle of another context, challenge = 0.  ZK_ERR_RANGE: challenge >= r.  On every
 * error *out is untouched. */
#define ZK_POWERS_CHECK_GENERATORS 0x001u
#define ZK_POWERS_CHECK_POWERS_G1 0x002u
#define ZK_POWERS_CHECK_POWERS_G2 0x004u
#define ZK_POWERS_CHECK_ALPHA 0x008u
#define ZK_POWERS_CHECK_BETA 0x010u
#define ZK_POWERS_CHECK_BETA_TWINS 0x020u
#define ZK_POWERS_CHECK_DEGENERATE 0x040u
#define ZK_POWERS_CHECK_RECORD 0x100u      /* zk_powers_contribution_check only */
#define ZK_POWERS_CHECK_KNOWLEDGE 0x200u   /* zk_powers_contribution_check only */
typedef struct {
    uint32_t failed;
    uint32_t flags;    /* reserved, 0 */
} zk_powers_check_result;
int zk_powers_check(zk_ctx* ctx, const zk_powers* powers, const uint64_t challenge[4] /* NULL = OS */, zk_powers_check_result* out);

/* A contribution: the transcript of (alpha a, beta b, x s) from the transcript of (alpha, beta, x), for secrets s, a, b of the
 * caller's -- byte for byte the arrays a transcript built from those three products holds:
 *   tau_g1[k] *= s^k (k < N1), tau_g2[k] *= s^k, alpha_tau_g1[k] *= a s^k, beta_tau_g1[k] *= b s^k (k < N2), beta_g2 *= b.
 * Every point takes a DIFFERENT scalar: the scalars are made and kept on the device (canonical), and k_mul_each (csrc/powers.hip)
 * multiplies one point per lane with an instruction stream that is the same for every lane of a wave: endomorphism split, regular
 * signed windows (every digit non-zero), a per-point table of odd multiples in LDS, one constant-time inversion per four points.
 *  - secrets: s, a, b as 3 x 4 canonical words, each 1 <= v < r; NULL draws all three from the OS -- they are then never returned.
 *    The device scalar arrays and every host copy are wiped before the call returns.  0: ZK_ERR_DIV_BY_ZERO; >= r: ZK_ERR_RANGE.
 *    (1, 1, 1) gives an equal transcript.
 *  - `before` is read only; synchronous, on a stream of its own.  ZK_ERR_ARG: a null pointer (secrets and tag excepted), a handle of
 *    another context.  On every failure *out is NULL and *record is untouched.  A degenerate `before` (an infinity among tau_g1[1],
 *    alpha_tau_g1[0], beta_tau_g1[0]) is multiplied like any other -- infinities stay infinities -- but no proof of knowledge exists
 *    over an infinity: that part of the record is all zero and never verifies.
 * The record holds three of the Schnorr records of zk_crs_contribution_prove, one per secret:
 *   tau    knowledge of s with tau_g1[1]' = s tau_g1[1];   alpha   of a with alpha_tau_g1[0]' = a alpha_tau_g1[0];
 *   beta   of b with beta_tau_g1[0]' = b beta_tau_g1[0]
 * each bound to tag_role = SHA-256("ZKPOWv1\0" | role byte (1 tau, 2 alpha, 3 beta) | tag) (tag NULL = 32 zero bytes), so that a
 * record cannot stand in another role or another ceremony step.  Nonces come from the OS.  zk_powers_contribution_prove is the host
 * side alone (no context): `before` = the three before-points (8 words each: tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0]); fixed
 * nonces (3 x 4 words) are for tests ONLY.  zk_powers_contribution_verify: *ok = 1 iff all three verify under their role tags. */
typedef struct {
    zk_crs_contribution tau, alpha, beta;
} zk_powers_contribution;
int zk_powers_contribution_prove(const uint64_t before[24], const uint64_t secrets[12], const uint64_t nonces[12] /* NULL = OS */,
                                 const uint8_t tag[32], zk_powers_contribution* out);
int zk_powers_contribution_verify(const zk_powers_contribution* c, const uint8_t tag[32], int* ok);
int zk_powers_contribute(zk_ctx* ctx, const zk_powers* before, const uint64_t secrets[12] /* s, a, b; NULL = OS */, const uint8_t tag[32],
                         zk_powers** out, zk_powers_contribution* record);

/* Is `after` a transcript, and is it `before` re-keyed by someone who knew the factors?  out->failed carries the ZK_POWERS_CHECK_* bits
 * of zk_powers_check(after), and
 *   RECORD       the six points of the record are not tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] of the two transcripts;
 *   KNOWLEDGE    one of the three zk_crs_contribution_verify calls, under its role tag, fails;
 *   DEGENERATE   (also) an after-point of the record is infinity.
 * `before` is NOT checked again: the head of a chain is zk_powers_initial or one zk_powers_check, and every later link is this call
 * (failed == 0 says `after` is a transcript in its own right, and the record ties its x, alpha, beta to those of `before`).
 * Soundness and the challenge as for zk_powers_check.  ZK_ERR_ARG: a null pointer (tag and challenge excepted), transcripts of
 * different dims or another context, challenge = 0; ZK_ERR_RANGE: challenge >= r.  On every error *out is untouched. */
int zk_powers_contribution_check(zk_ctx* ctx, const zk_powers* before, const zk_powers* after, const zk_powers_contribution* record,
                                 const uint8_t tag[32], const uint64_t challenge[4] /* NULL = OS */, zk_powers_check_result* out);

/* On-disk CRS container. The reference has no serialisation of SigmaG1/SigmaG2
 * (groth16/mod.rs:105-121), and setup (mod.rs:134-197) draws a fresh trapdoor on every call, so a CRS must be
 * written down to be reused.  Format: "ZKCRSv1\0", n, m, input, FNV-1a-64 of the payload, then the arrays of
 * zk_crs_desc in declaration order as canonical little-endian words.  A CRS that zk_setup made for an integer-roots QAP
 * (zk_qap_upload_sparse_integers) is written as "ZKCRSv2\0": the same, followed by its Lagrange-basis arrays, so that the
 * reloaded CRS serves that QAP form again.  zk_crs_load reads both, range- and curve-checks every point
 * and returns ZK_ERR_IO for a missing, truncated or altered file. */
int zk_crs_save(zk_ctx* ctx, const zk_crs* crs, const char* path);
int zk_crs_load(zk_ctx* ctx, const char* path, zk_crs** out);
/* The same for a QAP ("ZKQAPv1": the sparse rows over the roots w^j, or the dense coefficient matrices -- what
 * zk_qap_upload_sparse / zk_qap_upload_dense take; QAP<P> has no serialisation in the reference, groth16/mod.rs:60-67) and for a
 * proof ("ZKPRFv1": versioned magic | the 259 canonical bytes | checksum; Proof has no encoding in the reference, mod.rs:124-128).
 * ZK_ERR_IO for missing, truncated, altered or foreign files; values are range-checked by the upload path. */
int zk_qap_save(zk_ctx* ctx, const zk_qap* qap, const char* path);
int zk_qap_load(zk_ctx* ctx, const char* path, zk_qap** out);
int zk_proof_save(const uint8_t proof[ZK_PROOF_BYTES], const char* path);
int zk_proof_load(const char* path, uint8_t proof_out[ZK_PROOF_BYTES]);
/* The 259-byte proof <-> the compressed 128-byte form ("Compressed proof bytes" above; Proof has no encoding in the reference,
 * mod.rs:124-128).  Host code, no context (as zk_pairing / zk_proof_save).
 * zk_proof_compress: ZK_OK iff every block of `proof` has a legal tag (0x00 followed by zeros, or 0x04), coordinates < q and
 * lies on its curve; it does not run the subgroup test of B.  Otherwise ZK_ERR_RANGE and `out` = 128 zero bytes (flag 00, which
 * no decoder accepts).  zk_proof_decompress: ZK_OK iff all three blocks are valid encodings; otherwise ZK_ERR_RANGE and
 * `proof_out` = 259 bytes of 0xFF (tag 0xFF is refused by every decoder; 259 zero bytes would be a VALID proof of three
 * infinities).  decompress(compress(p)) == p for every p that compresses and compress(decompress(c)) == c for every c that
 * decompresses.  A null pointer: ZK_ERR_ARG, nothing written. */
int zk_proof_compress(const uint8_t proof[ZK_PROOF_BYTES], uint8_t out[ZK_PROOF_COMPRESSED_BYTES]);
int zk_proof_decompress(const uint8_t in[ZK_PROOF_COMPRESSED_BYTES], uint8_t proof_out[ZK_PROOF_BYTES]);
/* The same for n proofs in host memory on the GPU, one lane per point: entry j of the output and ok[j] are what the single form
 * writes and whether it returns ZK_OK, for every j < n (an invalid entry: ok[j] = 0 and the 0xFF / zero fill above).  The return
 * value is ZK_OK unless the call itself fails.  n == 0: ZK_OK, nothing touched.  Null ctx / input / output / ok: ZK_ERR_ARG.  Any n:
 * the proofs go through the device ZK_VERIFY_BATCH_CHUNK at a time and the results do not depend on the chunking.  Synchronous, on
 * zk_verify_batch's stream: no device-wide synchronisation, an outstanding zk_prove_submit ticket is neither waited for nor
 * disturbed. */
int zk_proof_compress_batch(zk_ctx* ctx, const uint8_t* proofs, size_t n, uint8_t* out, int* ok);
int zk_proof_decompress_batch(zk_ctx* ctx, const uint8_t* in, size_t n, uint8_t* proofs_out, int* ok);

/* ------------------------------------------------------------------------------------------
 * prove  (groth16::prove, groth16/mod.rs:213-296) with (r, s) injected (mod.rs:231)
 * ---------------------------------------------------------------------------------------- */
int zk_prove(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const uint64_t* weights, size_t m,
             const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[ZK_PROOF_BYTES]);
/* Same with the witness already resident in HBM (m x 4 words, canonical form). */
int zk_prove_dev(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                 const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[ZK_PROOF_BYTES]);

/* Pipelined form of zk_prove_dev for a stream of proofs: zk_prove_submit enqueues the whole proof
 * and returns at once with a ticket; zk_prove_wait blocks until that proof's bytes are ready.  At most
 * ZK_MAX_IN_FLIGHT proofs may be in flight per context (a further submit returns ZK_ERR_ARG until one is waited
 * for); the next proof's witness products and NTT stage then run under the previous one's reduction tail.  Two
 * in flight saturate one GPU on whole proofs; the short per-rank shares of a sharded proof profit from four.
 * The witness buffer must stay valid and unmodified until the matching wait.  Errors that are only
 * detected on the device (witness element >= r) are reported by zk_prove_wait. */
int zk_prove_submit(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                    const uint64_t r[4], const uint64_t s[4], int* ticket);
int zk_prove_wait(zk_ctx* ctx, int ticket, uint8_t* proof_out /* ZK_PROOF_BYTES; may be NULL for a partial ticket */);
/* zk_prove_submit with the witness in HOST memory (what a caller of groth16::prove holds, mod.rs:213-217): the 32 m
 * bytes are copied into a device buffer owned by the ticket, on the stream the proof starts on.  With page-locked
 * memory from zk_host_alloc the copy is asynchronous and the transfer of one proof overlaps the inner products of the
 * previous one (PCIe-inclusive rate of a stream of proofs = resident rate); with pageable memory the call blocks for
 * the copy.  The buffer must stay valid and unmodified until the matching zk_prove_wait. */
int zk_prove_submit_host(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const uint64_t* weights, size_t m,
                         const uint64_t r[4], const uint64_t s[4], int* ticket);
int zk_host_alloc(size_t bytes, void** out);   /* page-locked host memory (hipHostMalloc); no counterpart in the reference, whose
                                                * weights live in a Vec<FrLocal> (lib.rs:107) */
void zk_host_free(void* p);

/* Batches (roots-of-unity QAP form): what `count` calls of groth16::prove (groth16/mod.rs:213-296) over the same QAP and
 * CRS compute -- `count` proofs with their own witnesses and (r, s) -- as one unit of work -- the SpMV / NTT stages follow each other, the inner products of all proofs run as one grouped MSM per
 * product, two launches assemble them.  For circuits of 2^16 gates and fewer a single proof is bound by the latency
 * of its ~100 dependent launches; a batch spreads that chain over `count` proofs (2^16 gates: 2.6 ms per proof alone).
 * d_weights[j]: device pointer to proof j's witness (m[j] x 4 words, canonical); r, s: count x 4 words;
 * proofs_out: count x ZK_PROOF_BYTES.  A batch ticket counts as one proof in flight; a witness element >= r fails
 * the whole batch (ZK_ERR_RANGE from zk_prove_batch_wait). */
#define ZK_MAX_BATCH 64
int zk_prove_batch_submit(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, int count, const void* const* d_weights, const size_t* m,
                          const uint64_t* r, const uint64_t* s, int* ticket);
int zk_prove_batch_wait(zk_ctx* ctx, int ticket, int count, uint8_t* proofs_out);

/* Multi-GPU: every rank holds the CRS and recomputes the NTT stage; rank g owns
 * Pippenger windows w = g (mod world) of each inner product and writes its partial sums
 * (Jacobian, device Montgomery limbs) to d_partial_out (ZK_PARTIAL_BYTES).  The caller all-gathers
 * the blobs (RCCL, as bytes) and any rank finishes with zk_prove_combine.  (r, s) are needed here
 * because B in G1 enters the proof only as r*B1 and is folded into the H product as scalars r*v_i. */
#define ZK_PARTIAL_BYTES 768   /* 4 G1 Jacobian slots (96 B) + 1 G2 Jacobian (192 B), padded to 768 */
int zk_prove_partial(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                     const uint64_t r[4], const uint64_t s[4], int rank, int world, void* d_partial_out);
int zk_prove_combine(zk_ctx* ctx, const zk_crs* crs, const void* d_partials, int world,
                     const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[ZK_PROOF_BYTES]);
/* Pipelined form of zk_prove_partial (same in-flight rule as zk_prove_submit); finish with
 * zk_prove_wait(ctx, ticket, NULL), after which d_partial_out holds the rank's partial sums. */
int zk_prove_partial_submit(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                            const uint64_t r[4], const uint64_t s[4], int rank, int world, void* d_partial_out, int* ticket);

/* Multi-GPU, scalar exchange (roots-of-unity QAP form only).  Instead of repeating the SpMV / NTT
 * stage on every rank, the ranks take turns: in a round of `world` proofs rank j runs that stage for proof j
 * (zk_prove_scalars_submit) and writes the scalars of the four inner products (groth16/mod.rs:255-290: L over
 * sum_delta, V over [x^i]_2, U over [x^i]_1, h | r v + s u over [x^i t/delta]_1 | [x^i]_1) as `world` equal
 * chunks each -- chunk g multiplies the points rank g owns, [g c, (g+1) c) with c = ceil(count / world), zero
 * scalars behind the last point.  One all-to-all per array (RCCL, equal splits) hands every rank its chunk of
 * every proof of the round; zk_prove_msm_submit accumulates them over the rank's points (partial sums of proof j
 * at d_partials_out + j * ZK_PARTIAL_BYTES), a second all-to-all returns the blobs to the proofs' owners, and
 * zk_prove_combine finishes.  Each array has elems_out[k] elements of 32 bytes (k = L, V, U, H). */
int zk_prove_exchange_elems(const zk_qap* qap, int world, size_t elems_out[4]);
int zk_prove_scalars_submit(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                            const uint64_t r[4], const uint64_t s[4], int world,
                            void* d_l, void* d_v, void* d_u, void* d_h, int* ticket);
/* the same from a host witness (see zk_prove_submit_host) */
int zk_prove_scalars_submit_host(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, const uint64_t* weights, size_t m,
                                 const uint64_t r[4], const uint64_t s[4], int world,
                                 void* d_l, void* d_v, void* d_u, void* d_h, int* ticket);
/* d_l .. d_h: `sets` chunks each, as delivered by the all-to-all (chunk j = proof j's scalars for this rank's points).
 * One ticket for the batch; finish with zk_prove_wait(ctx, ticket, NULL). */
int zk_prove_msm_submit(zk_ctx* ctx, const zk_crs* crs, const zk_qap* qap, int sets, int rank, int world,
                        const void* d_l, const void* d_v, const void* d_u, const void* d_h, void* d_partials_out, int* ticket);

/* ------------------------------------------------------------------------------------------
 * Several GPUs ("one context owns 1..8 devices"; 8e).  The reference's groth16::prove
 * (groth16/mod.rs:213-217) is one call on one thread; its inner products (mod.rs:255-272,279-290) are sums of
 * independent terms and shard over GPUs.  One process per GPU, each with its own zk_ctx; a zk_comm joins them: RCCL over
 * xGMI (libzkgpu.so links librccl), or a transport supplied by the caller as function pointers.
 * ---------------------------------------------------------------------------------------- */
int zk_device_count(void);
#define ZK_COMM_ID_BYTES 128
typedef struct zk_comm zk_comm;
/* Rank 0 draws the id (ncclGetUniqueId) and ships the bytes to the other ranks by any channel (file, TCP store, MPI). */
int zk_comm_unique_id(uint8_t id_out[ZK_COMM_ID_BYTES]);
/* Collective: every rank calls it with the same id and its own rank (ncclCommInitRank on ctx's device).  world == 1
 * needs no id and no RCCL.  The set-up is bounded like every other wait on a peer (ZK_COMM_TIMEOUT_MS): ncclCommInitRank runs on a
 * helper thread, and when a peer never arrives the call returns ZK_ERR_COMM while that thread stays inside RCCL's bootstrap.  After
 * such a time-out do NOT retry with the same id in this process and do not unload the library: report the failure and let the
 * process end (bench.py's `degraded` path does exactly that). */
int zk_comm_init(zk_ctx* ctx, const uint8_t id[ZK_COMM_ID_BYTES], int rank, int world, zk_comm** out);
/* Caller-supplied transport.  Buffers are the ones the prover allocated (device memory with the GPU backend); the calls
 * are blocking: complete on return.  all_to_all: chunk g of `send` (bytes_per_rank bytes) goes to rank g, chunk j of `recv`
 * comes from rank j.  all_gather: `send` (bytes_per_rank) from every rank, in rank order, into `recv`.  barrier / max_f64
 * may be NULL (zk_comm_barrier / zk_comm_max_f64 then return ZK_ERR_UNSUPPORTED).  Non-zero return = failure. */
typedef struct {
    void* user;
    int (*all_to_all)(void* user, const void* send, void* recv, size_t bytes_per_rank);
    int (*all_gather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
    int (*barrier)(void* user);
    int (*max_f64)(void* user, double* value);
} zk_comm_ops;
int zk_comm_init_custom(zk_ctx* ctx /* may be NULL */, const zk_comm_ops* ops, int rank, int world, zk_comm** out);
/* A communicator outlives the zk_mgpu provers created over it.  Destroying it while a prover still holds it is safe all the same:
 * the call then only marks it, and the last zk_mgpu_destroy frees it. */
void zk_comm_destroy(zk_comm* comm);
int zk_comm_rank(const zk_comm* comm);
int zk_comm_world(const zk_comm* comm);
/* ranks of the RCCL communicator behind this zk_comm as RCCL counts them (ncclCommCount); 0 = none (one rank, a caller's transport,
 * aborted).  Evidence for the bench line that a world-N run really went through an N-rank RCCL communicator. */
int zk_comm_rccl_ranks(const zk_comm* comm);
/* Every host wait for a collective (zk_comm_barrier / _max_f64 / _all_to_all / _all_gather, zk_mgpu_pop) is bounded: after `ms`
 * milliseconds (default 120000, or ZK_COMM_TIMEOUT_MS at zk_comm_init; 0 = unbounded) the RCCL communicator is aborted and the call
 * returns ZK_ERR_COMM, as does every later one.  The reference's prove (mod.rs:213-217) cannot hang on a peer; neither may this. */
int zk_comm_set_timeout(zk_comm* comm, long ms);
/* Gives up on the peers now (ncclCommAbort): callable from another thread while a collective is being waited for OR enqueued -- an
 * enqueue that is under way finishes its RCCL calls first (the abort waits for it, 200 ms at most); every later call answers
 * ZK_ERR_COMM. */
int zk_comm_abort(zk_comm* comm);
int zk_comm_barrier(zk_comm* comm);
int zk_comm_max_f64(zk_comm* comm, double* value);      /* *value = max over the ranks (timing of the slowest rank) */
int zk_comm_all_to_all(zk_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);   /* complete on return */
int zk_comm_all_gather(zk_comm* comm, const void* d_send, void* d_recv, size_t bytes_per_rank);

/* Latency form -- ONE groth16::prove over all ranks: every rank holds the same witness, recomputes the SpMV / NTT stage,
 * accumulates its share of the inner products (three with merge_lh; zk_prove_partial: Pippenger windows w = rank (mod world), or point
 * ranges with the option msm_shard_points), one 768-byte all-gather, and every rank assembles the same 259 bytes. */
int zk_mgpu_prove_sharded(zk_ctx* ctx, zk_comm* comm, const zk_crs* crs, const zk_qap* qap, const void* d_weights, size_t m,
                          const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[ZK_PROOF_BYTES]);

/* Throughput form -- the scalar exchange of zk_prove_scalars_submit / zk_prove_msm_submit as a software pipeline inside the
 * library.  A ROUND is `world` proofs, one per rank: zk_mgpu_push hands in THIS rank's proof of the next round (its own
 * witness and (r, s)), zk_mgpu_pop returns THIS rank's proof of the oldest round.  Both are collective: every rank makes
 * the same sequence of push / pop calls.  At most three rounds may be pushed and not yet popped; pushing two rounds ahead
 * of every pop (push, push, push, pop, push, pop, ...) keeps the SpMV / NTT stage two rounds ahead of the inner products, so
 * that neither the exchanges nor the host waits leave a GPU idle; push / pop strictly alternating is the one-round-at-a-time
 * (latency) schedule.  Per-GPU work per round is one whole proof's worth whatever `world` is.  Sparse QAP forms only
 * (roots of unity or integer roots). */
typedef struct zk_mgpu zk_mgpu;
int zk_mgpu_create(zk_ctx* ctx, zk_comm* comm, const zk_crs* crs, const zk_qap* qap, zk_mgpu** out);
int zk_mgpu_push(zk_mgpu* p, const void* d_weights, size_t m, const uint64_t r[4], const uint64_t s[4]);
/* The same with the witness in host memory, as the reference's prove(&[T]) hands it over (mod.rs:213-217): copied into a
 * device buffer owned by the round on the stream the proof starts on (page-locked memory from zk_host_alloc: asynchronously). */
int zk_mgpu_push_host(zk_mgpu* p, const uint64_t* weights, size_t m, const uint64_t r[4], const uint64_t s[4]);
int zk_mgpu_pop(zk_mgpu* p, uint8_t proof_out[ZK_PROOF_BYTES]);
void zk_mgpu_destroy(zk_mgpu* p);
const char* zk_mgpu_last_error(const zk_mgpu* p);
/* The pipeline over caller-supplied stages (tests: CPU stand-ins + a gloo transport exercise the schedule and the order of
 * the collectives without a GPU).  elems: sizes of the four exchange arrays in 32-byte elements (multiples of world);
 * scalars_submit writes `world` equal chunks into send[0..3]; msm_submit consumes recv[0..3] (chunk j = proof j) and writes
 * `sets` blobs of ZK_PARTIAL_BYTES; wait completes a ticket; combine assembles from the `world` blobs returned to the owner. */
typedef struct {
    void* user;
    int (*elems)(void* user, int world, size_t elems_out[4]);
    void* (*alloc)(void* user, size_t bytes);
    void (*free)(void* user, void* p);
    int (*scalars_submit)(void* user, const void* weights, size_t m, const uint64_t r[4], const uint64_t s[4], int world, void* const send[4], int* ticket);
    int (*msm_submit)(void* user, int sets, int rank, int world, void* const recv[4], void* partials_out, int* ticket);
    int (*wait)(void* user, int ticket);
    int (*combine)(void* user, const void* partials, int world, const uint64_t r[4], const uint64_t s[4], uint8_t proof_out[ZK_PROOF_BYTES]);
} zk_mgpu_backend;
int zk_mgpu_create_custom(zk_comm* comm, const zk_mgpu_backend* backend, zk_mgpu** out);

/* ------------------------------------------------------------------------------------------
 * verify  (groth16::verify, groth16/mod.rs:299-320) -- host code, as in the reference
 * ---------------------------------------------------------------------------------------- */
/* *ok = 1 iff e(alpha,beta) e(sum_i x_i sum_gamma_i, gamma) e(C,delta) == e(A,B) with x = (1, inputs...).
 * inputs: n_inputs Fr values (the `verify` wires, without the leading 1).  A malformed proof gives *ok = 0: the
 * decoder accepts exactly one byte string per point (tag 0x00 followed by zeros only = infinity; tag 0x04 + coordinates
 * < q on the curve, never (0, 0)) and B must lie in the order-r subgroup G2 of the twist ([r]B = infinity is checked:
 * the twist's cofactor has small factors and the pairing is bilinear only on G2). */
int zk_verify(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t proof[ZK_PROOF_BYTES], int* ok);
/* Batch verify on the GPU: ok[j] = what zk_verify(ctx, crs, inputs + 4 n_inputs j, n_inputs, proofs + ZK_PROOF_BYTES j, &ok)
 * writes, for every j < n_proofs.  proofs: n_proofs x ZK_PROOF_BYTES bytes; inputs: n_proofs rows of n_inputs Fr values
 * (4 words each), the same count for every proof; as in zk_verify only the first min(l, n_inputs) of a row are read.
 * n_proofs == 0: ZK_OK, nothing written.  Null ctx / crs / proofs / ok, or null inputs with n_inputs > 0: ZK_ERR_ARG.  An input
 * >= r among those read: ZK_ERR_RANGE and every ok[j] = 0, decided on the host before anything is launched.  A CRS point off
 * its curve or outside G2: ZK_ERR_ARG.  Any n_proofs: the proofs go through the device ZK_VERIFY_BATCH_CHUNK at a time
 * (device memory ~1.2 KB + 32 min(l, n_inputs) bytes per proof of a chunk); the verdicts do not depend on the chunking.
 * Synchronous: returns when the verdicts are in host memory.  It runs on a stream of its own and waits only on that stream
 * (no device-wide synchronisation): a zk_prove_submit ticket outstanding on the same context is neither waited for nor
 * disturbed. */
#define ZK_VERIFY_BATCH_CHUNK 65536
int zk_verify_batch(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs, int* ok);
/* zk_verify_batch over compressed proofs: proofs = n_proofs x ZK_PROOF_COMPRESSED_BYTES bytes, decompressed on the GPU in front
 * of the same kernels; ok[j] = 1 iff entry j decompresses (zk_proof_decompress) AND zk_verify accepts the result.  Arguments,
 * statuses, chunking and stream are exactly zk_verify_batch's.  Not offered: a compressed form of zk_verify_batch_all (call
 * zk_proof_decompress_batch first), a compressed ZKPRFv1 file, compressed CRS points. */
int zk_verify_batch_compressed(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                               size_t n_proofs, int* ok);
/* One verdict for a whole batch on the GPU, by a random linear combination: *ok = 1 iff every proof passes zk_verify's
 * decoder (tag rules, coordinates < q, on the curve, [r]B = infinity) and
 *     prod_j e(A_j, B_j)^{z_j} = e(alpha, beta)^{t_0} e(T_S, gamma) e(T_C, delta),
 *     t_0 = sum_j z_j, t_i = sum_j z_j x_ji (mod r), T_S = sum_{i=0..k} t_i sum_gamma_i, T_C = sum_j z_j C_j.
 * inputs and proofs as in zk_verify_batch (only the first min(l, n_inputs) entries of a row are read); z: n_proofs
 * multipliers of 2 words each, little-endian 128-bit integers, every one non-zero.
 *  - If zk_verify accepts every proof, *ok = 1 for every admissible z (deterministic).
 *  - A proof that fails to decode gives *ok = 0 (deterministic).
 *  - Otherwise *ok = 0 unless z falls in a set of density at most 1 / (2^128 - 1): z must be unpredictable to whoever made
 *    the proofs (draw it from a secure random source after the proofs are fixed).
 *  - Which proofs are bad: call zk_verify_batch.
 * Null ctx / crs / proofs / z / ok, or null inputs with n_inputs > 0: ZK_ERR_ARG.  Any z_j = 0: ZK_ERR_ARG and *ok = 0; an
 * input >= r among those read: ZK_ERR_RANGE and *ok = 0; both decided on the host before anything is launched.  A CRS point
 * off its curve or outside G2: ZK_ERR_ARG.  n_proofs == 0: ZK_OK and *ok = 1.  Any n_proofs: the proofs go through the
 * device ZK_VERIFY_BATCH_CHUNK at a time, partial products and sums carry across chunks on the device, and one final
 * exponentiation runs per call; the verdict does not depend on the chunking.  Synchronous, on the same stream of its own as
 * zk_verify_batch: no device-wide synchronisation, an outstanding zk_prove_submit ticket is neither waited for nor disturbed.
 * Below about one wave per SIMD (N < 65536) both batch calls are bound by one lane's serial chain. */
int zk_verify_batch_all(zk_ctx* ctx, const zk_crs* crs, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                        size_t n_proofs, const uint64_t* z, int* ok);
/* EllipticEncryptable::pairing (fr.rs:120-122): the optimal ate pairing e(P, Q) as 12 Fq coefficients
 * (48 words) in the order c0.a0.c0, c0.a0.c1, c0.a1.c0, ..., c1.a2.c1 of the tower
 * Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9+i)).  Host only; needs no context.  ZK_ERR_RANGE when a coordinate
 * is >= q, a point is off its curve or g2 is outside the order-r subgroup. */
int zk_pairing(const uint64_t g1[ZK_G1_WORDS], const uint64_t g2[ZK_G2_WORDS], uint64_t out[48]);

/* ------------------------------------------------------------------------------------------
 * verifying key: what groth16::verify reads of (SigmaG1, SigmaG2) (groth16/mod.rs:299-320: alpha, beta, gamma, delta and the
 * l + 1 points of sum_gamma), as an object of its own -- a verifier needs neither the proving key nor, for one proof, a GPU.
 * The reference has no such type: its verify takes the whole (SigmaG1, SigmaG2).
 * ---------------------------------------------------------------------------------------- */
typedef struct zk_vk zk_vk;
typedef struct {
    size_t input;                  /* l */
    const uint64_t* alpha_g1;      /* 8 words */
    const uint64_t *beta_g2, *gamma_g2, *delta_g2;   /* 16 words each */
    const uint64_t* sum_gamma_g1;  /* (l + 1) x 8 words, wires 0..l */
} zk_vk_desc;
/* The object is host data; the calls of this first group need no context (as zk_pairing / zk_proof_compress).
 * zk_vk_create: every point goes through zk_verify's readers (coordinates < q, on the curve, G2 points in the order-r subgroup;
 * infinity = all zero is legal); a failing point: ZK_ERR_RANGE and *out = NULL; an l the host has no memory for: ZK_ERR_SIZE.  What depends only on the points -- the lines of
 * beta, gamma and delta and ml(alpha, beta) -- is computed here, once.
 * Byte form (zk_vk_to_bytes and the file of zk_vk_save are the same bytes): "ZKVKv1\0\0" | l as u64 LE | FNV-1a-64 of the payload
 * as u64 LE (the checksum of ZKCRSv1) | payload = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | sum_gamma_g1[0..l] as canonical
 * little-endian words; zk_vk_bytes(l) = 24 + 8 (56 + 8 (l + 1)).  zk_vk_to_bytes needs len >= zk_vk_bytes(l) and writes exactly
 * that many.  zk_vk_from_bytes / zk_vk_load: ZK_ERR_IO for a wrong length, magic or checksum or a missing file, ZK_ERR_RANGE for a
 * point zk_vk_create would refuse; to_bytes(from_bytes(b)) == b.
 * zk_vk_verify: *ok and the status are zk_verify's for every proof and input row (the row is truncated to min(l, n_inputs) the
 * same way, an input >= r among those read gives ZK_ERR_RANGE), without a context and without a GPU.
 * A null pointer: ZK_ERR_ARG, nothing written.  zk_vk_free(NULL) is a no-op. */
int zk_vk_create(const zk_vk_desc* desc, zk_vk** out);
void zk_vk_free(zk_vk* vk);
int zk_vk_dims(const zk_vk* vk, size_t* input);
size_t zk_vk_bytes(size_t input);
int zk_vk_to_bytes(const zk_vk* vk, uint8_t* out, size_t len);
int zk_vk_from_bytes(const uint8_t* in, size_t len, zk_vk** out);
int zk_vk_save(const zk_vk* vk, const char* path);
int zk_vk_load(const char* path, zk_vk** out);
int zk_vk_verify(const zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t proof[ZK_PROOF_BYTES], int* ok);
/* The key of a device CRS: the points are copied on zk_verify_batch's stream (an outstanding zk_prove_submit ticket is neither
 * waited for nor disturbed) and go through zk_vk_create. */
int zk_vk_from_crs(zk_ctx* ctx, const zk_crs* crs, zk_vk** out);
/* Batch verification over a key: zk_verify_batch, zk_verify_batch_compressed and zk_verify_batch_all with the key in the place of
 * the CRS.  Verdicts, statuses, error texts, chunking, stream and device buffers are exactly those calls' (see there); only the
 * re-check of the CRS points has no counterpart, a key's points were checked when it was made.
 * On its first batch call a key BINDS to that context: its constants are uploaded once, on the verify stream, and stay resident;
 * a later batch call with another context (or after that context was destroyed) gives ZK_ERR_ARG.  zk_vk_free and
 * zk_ctx_destroy are safe in either order.  The device memory of a key freed first (constants and tables) is parked, not freed --
 * freeing would wait for an outstanding proof ticket -- and goes with the context: a long-lived context that binds and frees
 * many keys should re-use keys, or be re-created now and then.  The input sums S_j = sum_gamma_0 + sum_i x_ji sum_gamma_i are formed from per-key
 * window tables (4-bit unsigned digits: 60 KiB of device memory per input, built on the first call that may use them) unless
 * the tables would exceed the option "vk_table_kib" (KiB; default 65536; 0 = never), the device has no memory for them, or l = 0: then zk_verify_batch's kernel
 * runs on the key's resident bases.  That is a memory condition; the verdicts never depend on it. */
int zk_vk_verify_batch(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs, int* ok);
int zk_vk_verify_batch_compressed(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs,
                                  size_t n_proofs, int* ok);
int zk_vk_verify_batch_all(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t* proofs, size_t n_proofs,
                           const uint64_t* z, int* ok);
/* The input sums on their own (the building block behind the batch calls, as zk_msm_g1 is behind zk_prove): out[j] = S_j for
 * j < n, 8 canonical words each (infinity = all zero); inputs: n rows of n_inputs Fr values, of which the first min(l, n_inputs)
 * are read.  tables = 0 runs zk_verify_batch's bit-serial kernel, tables = 1 the table kernel; the words are the same.
 * tables = 1 on a key whose tables exceed "vk_table_kib" (or found no device memory): ZK_ERR_SIZE.  An input >= r: ZK_ERR_RANGE.  n == 0: ZK_OK. */
int zk_vk_input_sums(zk_ctx* ctx, zk_vk* vk, const uint64_t* inputs, size_t n_inputs, size_t n, int tables, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKGPU_H */
