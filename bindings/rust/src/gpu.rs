// src/groth16/gpu.rs -- binding of libzkgpu.so inside the reference crate.
//
// NOT compiled in this repository: the image has no Rust toolchain and the crate `bn 0.4.3` is not vendored.  What CAN
// be executed here is: every C-ABI call sequence below, in the same order and with the same argument conventions, by
// tests/cpp/rust_shim_sequence.c (run on the GPU by tests/test_cpp_api.py), and the byte-level conversions of module
// `bn_bytes` (big-endian coordinates <-> little-endian words, the Fq2 packing c1*q + c0), restated in C in the same file
// and checked against the public alt_bn128 vectors of tests/golden/alt_bn128.json.
//
// The module must live INSIDE the crate (src/groth16/gpu.rs, `pub mod gpu;` in src/groth16/mod.rs) because QAP, SigmaG1,
// SigmaG2 and Proof have private fields (mod.rs:60-67,105-128).  The newtypes of fr.rs wrap private bn values
// (fr.rs:8-16), so fr.rs additionally gets the six one-line accessors listed in INTEGRATION.md 2a:
//     impl FrLocal { pub(super) fn bn(&self) -> Fr { self.0 }  pub(super) fn from_bn(x: Fr) -> Self { FrLocal(x) } }
//     (the same pair for G1Local / G1 and G2Local / G2)
// and Cargo.toml gains `rustc-serialize = "0.3"` (already a dependency of bn; it is how bn exposes coordinates).
//
//! GPU Groth16 behind the reference API: `setup`, `prove`, `verify` with the argument order, borrow pattern and by-value
//! results of groth16::{setup, prove, verify} (mod.rs:134, 213-217, 299-303).
extern crate rustc_serialize;

use super::fr::{FrLocal, G1Local, G2Local};
use super::circuit::RootRepresentation;
use super::{CoefficientPoly, Proof, Random, SigmaG1, SigmaG2, QAP};
use std::cell::RefCell;
use std::collections::HashMap;
use std::os::raw::{c_char, c_int, c_uint, c_void};

// ------------------------------------------------------------------------------------------------
// C ABI (include/zkgpu.h)
// ------------------------------------------------------------------------------------------------
#[repr(C)] pub struct ZkCtx { _p: [u8; 0] }
#[repr(C)] pub struct ZkCrs { _p: [u8; 0] }
#[repr(C)] pub struct ZkQap { _p: [u8; 0] }

#[repr(C)]
pub struct ZkCrsDesc {                                   // zk_crs_desc
    n: usize, m: usize, input: usize,
    alpha_g1: *const u64, beta_g1: *const u64, delta_g1: *const u64,
    xi_g1: *const u64, sum_gamma_g1: *const u64, sum_delta_g1: *const u64, xi_t_g1: *const u64,
    beta_g2: *const u64, gamma_g2: *const u64, delta_g2: *const u64, xi_g2: *const u64,
}
#[repr(C)]
pub struct ZkCrsOut {                                    // zk_crs_out (same field order, mutable; null = skip)
    alpha_g1: *mut u64, beta_g1: *mut u64, delta_g1: *mut u64,
    xi_g1: *mut u64, sum_gamma_g1: *mut u64, sum_delta_g1: *mut u64, xi_t_g1: *mut u64,
    beta_g2: *mut u64, gamma_g2: *mut u64, delta_g2: *mut u64, xi_g2: *mut u64,
}
#[repr(C)]
pub struct ZkSparseRows { ptr: *const u64, gate: *const u32, val: *const u64 }   // zk_sparse_rows: CSR by wire
#[repr(C)]
pub struct ZkQapSparseDesc { log_n: c_uint, m: usize, input: usize, u: ZkSparseRows, v: ZkSparseRows, w: ZkSparseRows }
#[repr(C)]
pub struct ZkQapCheckResult { pub bad_gates: u32, pub first_bad: u32, pub flags: u32 }   // zk_qap_check_result (12 bytes)
#[repr(C)]
pub struct ZkPowersDesc {                                // zk_powers_desc: a powers-of-tau transcript, canonical affine words
    n_tau_g1: usize, n_rest: usize,
    tau_g1: *const u64, tau_g2: *const u64, alpha_tau_g1: *const u64, beta_tau_g1: *const u64, beta_g2: *const u64,
}
/// A powers-of-tau transcript as GpuProver::from_powers takes it: 8 words per G1 point, 16 per G2 point, canonical affine,
/// little-endian; tau_g1 holds at least 2n - 1 points, tau_g2 / alpha_tau_g1 / beta_tau_g1 one common count of at least n.
pub struct PowersOfTau<'a> {
    pub tau_g1: &'a [u64], pub tau_g2: &'a [u64], pub alpha_tau_g1: &'a [u64], pub beta_tau_g1: &'a [u64], pub beta_g2: &'a [u64; 16],
}
#[repr(C)] pub struct ZkPowers { _p: [u8; 0] }            // zk_powers: a transcript resident on the device
#[repr(C)]
pub struct ZkPowersOut {                                 // zk_powers_out (same field order, mutable; null = skip)
    tau_g1: *mut u64, tau_g2: *mut u64, alpha_tau_g1: *mut u64, beta_tau_g1: *mut u64, beta_g2: *mut u64,
}
#[repr(C)]
pub struct ZkPowersCheckResult { pub failed: u32, pub flags: u32 }   // zk_powers_check_result: ZK_POWERS_CHECK_* bits
pub const ZK_POWERS_CHECK_GENERATORS: u32 = 0x001;
pub const ZK_POWERS_CHECK_POWERS_G1: u32 = 0x002;
pub const ZK_POWERS_CHECK_POWERS_G2: u32 = 0x004;
pub const ZK_POWERS_CHECK_ALPHA: u32 = 0x008;
pub const ZK_POWERS_CHECK_BETA: u32 = 0x010;
pub const ZK_POWERS_CHECK_BETA_TWINS: u32 = 0x020;
pub const ZK_POWERS_CHECK_DEGENERATE: u32 = 0x040;
pub const ZK_POWERS_CHECK_RECORD: u32 = 0x100;
pub const ZK_POWERS_CHECK_KNOWLEDGE: u32 = 0x200;
/// zk_powers_contribution: three ZkCrsContribution records (tau | alpha | beta), 672 bytes
#[repr(C, align(8))]
#[derive(Clone, Copy)]
pub struct ZkPowersContribution(pub [u8; 672]);
/// The five arrays of a transcript as owned vectors (what PowersOfTau::contribute returns); `view` lends them as a PowersOfTau
pub struct PowersOfTauOwned {
    pub tau_g1: Vec<u64>, pub tau_g2: Vec<u64>, pub alpha_tau_g1: Vec<u64>, pub beta_tau_g1: Vec<u64>, pub beta_g2: [u64; 16],
}
impl PowersOfTauOwned {
    pub fn view(&self) -> PowersOfTau {
        PowersOfTau { tau_g1: &self.tau_g1, tau_g2: &self.tau_g2, alpha_tau_g1: &self.alpha_tau_g1, beta_tau_g1: &self.beta_tau_g1, beta_g2: &self.beta_g2 }
    }
}
#[repr(C)]
pub struct ZkCrsCheckResult { pub failed: u32, pub flags: u32 }   // zk_crs_check_result: ZK_CRS_CHECK_* bits
pub const ZK_CRS_CHECK_T_ZERO: u32 = 1;                // flags: x is a root of t (consistent, unsound)
pub const ZK_CRS_CHECK_LAGRANGE_PRESENT: u32 = 2;      // flags: the CRS carries Lagrange-basis arrays
/// zk_crs_contribution: delta_before_g1 | delta_after_g1 | commit_g1 (8 words each) | response (4 words); its 224-byte memory image
/// is its byte form (ZkCrsContribution::to_bytes / from_bytes)
#[repr(C, align(8))]
#[derive(Clone, Copy)]
pub struct ZkCrsContribution(pub [u8; 224]);
#[repr(C)]
pub struct ZkCrsContributionResult { pub failed: u32, pub flags: u32 }   // zk_crs_contribution_result: ZK_CONTRIB_* bits
pub const ZK_CONTRIB_UNCHANGED: u32 = 0x01;
pub const ZK_CONTRIB_RECORD: u32 = 0x02;
pub const ZK_CONTRIB_KNOWLEDGE: u32 = 0x04;
pub const ZK_CONTRIB_DELTA_TWINS: u32 = 0x08;
pub const ZK_CONTRIB_SUM_DELTA: u32 = 0x10;
pub const ZK_CONTRIB_XI_T: u32 = 0x20;
pub const ZK_CONTRIB_DEGENERATE: u32 = 0x40;
#[repr(C)] pub struct ZkVk { _p: [u8; 0] }
#[repr(C)]
pub struct ZkVkDesc {                                    // zk_vk_desc
    input: usize,
    alpha_g1: *const u64,
    beta_g2: *const u64, gamma_g2: *const u64, delta_g2: *const u64,
    sum_gamma_g1: *const u64,
}
pub const ZK_QAP_CHECK_NONE: u32 = 0xFFFF_FFFF;
pub const ZK_QAP_CHECK_WIRE0: u32 = 1;

extern "C" {
    fn zk_ctx_create(device: c_int, out: *mut *mut ZkCtx) -> c_int;
    fn zk_ctx_destroy(ctx: *mut ZkCtx);
    fn zk_last_error(ctx: *const ZkCtx) -> *const c_char;
    fn zk_qap_upload_dense(ctx: *mut ZkCtx, u: *const u64, v: *const u64, w: *const u64, t: *const u64,
                           m: usize, n: usize, input: usize, out: *mut *mut ZkQap) -> c_int;
    fn zk_qap_upload_sparse(ctx: *mut ZkCtx, desc: *const ZkQapSparseDesc, out: *mut *mut ZkQap) -> c_int;
    fn zk_qap_free(q: *mut ZkQap);
    fn zk_crs_upload(ctx: *mut ZkCtx, desc: *const ZkCrsDesc, out: *mut *mut ZkCrs) -> c_int;
    fn zk_crs_download(ctx: *mut ZkCtx, crs: *const ZkCrs, out: *const ZkCrsOut) -> c_int;
    fn zk_crs_free(c: *mut ZkCrs);
    fn zk_qap_upload_sparse_integers(ctx: *mut ZkCtx, desc: *const ZkQapSparseDesc, n: usize, out: *mut *mut ZkQap) -> c_int;
    fn zk_qap_upload_sparse_roots(ctx: *mut ZkCtx, desc: *const ZkQapSparseDesc, roots: *const u64, n: usize, out: *mut *mut ZkQap) -> c_int;
    fn zk_setup(ctx: *mut ZkCtx, qap: *const ZkQap, trapdoor: *const u64, out: *mut *mut ZkCrs) -> c_int;
    fn zk_prove(ctx: *mut ZkCtx, crs: *const ZkCrs, qap: *const ZkQap, weights: *const u64, m: usize,
                r: *const u64, s: *const u64, proof_out: *mut u8) -> c_int;
    fn zk_verify(ctx: *mut ZkCtx, crs: *const ZkCrs, inputs: *const u64, n_inputs: usize, proof: *const u8, ok: *mut c_int) -> c_int;
    fn zk_verify_batch(ctx: *mut ZkCtx, crs: *const ZkCrs, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                       ok: *mut c_int) -> c_int;
    fn zk_verify_batch_all(ctx: *mut ZkCtx, crs: *const ZkCrs, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                           z: *const u64, ok: *mut c_int) -> c_int;
    fn zk_verify_batch_compressed(ctx: *mut ZkCtx, crs: *const ZkCrs, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                                  ok: *mut c_int) -> c_int;
    // the verifying key: host object (no context) + the batch calls with the key in the place of the CRS
    fn zk_vk_create(desc: *const ZkVkDesc, out: *mut *mut ZkVk) -> c_int;
    fn zk_vk_from_crs(ctx: *mut ZkCtx, crs: *const ZkCrs, out: *mut *mut ZkVk) -> c_int;
    fn zk_vk_free(vk: *mut ZkVk);
    fn zk_vk_dims(vk: *const ZkVk, input: *mut usize) -> c_int;
    fn zk_vk_bytes(input: usize) -> usize;
    fn zk_vk_to_bytes(vk: *const ZkVk, out: *mut u8, len: usize) -> c_int;
    fn zk_vk_from_bytes(input: *const u8, len: usize, out: *mut *mut ZkVk) -> c_int;
    fn zk_vk_save(vk: *const ZkVk, path: *const c_char) -> c_int;
    fn zk_vk_load(path: *const c_char, out: *mut *mut ZkVk) -> c_int;
    fn zk_vk_verify(vk: *const ZkVk, inputs: *const u64, n_inputs: usize, proof: *const u8, ok: *mut c_int) -> c_int;
    fn zk_vk_verify_batch(ctx: *mut ZkCtx, vk: *mut ZkVk, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                          ok: *mut c_int) -> c_int;
    fn zk_vk_verify_batch_compressed(ctx: *mut ZkCtx, vk: *mut ZkVk, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                                     ok: *mut c_int) -> c_int;
    fn zk_vk_verify_batch_all(ctx: *mut ZkCtx, vk: *mut ZkVk, inputs: *const u64, n_inputs: usize, proofs: *const u8, n_proofs: usize,
                              z: *const u64, ok: *mut c_int) -> c_int;
    fn zk_vk_input_sums(ctx: *mut ZkCtx, vk: *mut ZkVk, inputs: *const u64, n_inputs: usize, n: usize, tables: c_int, out: *mut u64) -> c_int;
    // the 259-byte proof <-> the compressed 128-byte form: on the host (no context), or for n proofs on the GPU
    fn zk_proof_compress(proof: *const u8, out: *mut u8) -> c_int;
    fn zk_proof_decompress(input: *const u8, proof_out: *mut u8) -> c_int;
    fn zk_proof_compress_batch(ctx: *mut ZkCtx, proofs: *const u8, n: usize, out: *mut u8, ok: *mut c_int) -> c_int;
    fn zk_proof_decompress_batch(ctx: *mut ZkCtx, input: *const u8, n: usize, proofs_out: *mut u8, ok: *mut c_int) -> c_int;
    // the .zk front end's witness as a compiled tape: one witness on the host, or a whole batch on the GPU with the witnesses left in
    // HBM where zk_prove_batch_submit takes them (d_weights_out + j * m * 32 bytes is witness j)
    fn zk_circuit_parse(code: *const c_char, out: *mut *mut ZkCircuit, err: *mut c_char, err_len: usize) -> c_int;
    fn zk_circuit_free(c: *mut ZkCircuit);
    fn zk_circuit_dims(c: *const ZkCircuit, m: *mut usize, n: *mut usize, input: *mut usize, n_in: *mut usize) -> c_int;
    fn zk_circuit_last_error(c: *const ZkCircuit) -> *const c_char;
    fn zk_circuit_tape_dims(c: *const ZkCircuit, ops: *mut usize, slots: *mut usize, consts: *mut usize, depth: *mut usize,
                            width: *mut usize) -> c_int;
    fn zk_circuit_weights_tape(c: *const ZkCircuit, inputs: *const u64, n_in: usize, weights_out: *mut u64, m: usize) -> c_int;
    fn zk_witgen_create(ctx: *mut ZkCtx, c: *const ZkCircuit, out: *mut *mut ZkWitgen) -> c_int;
    fn zk_witgen_free(w: *mut ZkWitgen);
    fn zk_witgen_run(w: *mut ZkWitgen, d_inputs: *const c_void, n_in: usize, count: usize, d_weights_out: *mut c_void, m: usize) -> c_int;
    // the gate-level circuit builder (circuit/builder/mod.rs) behind the ABI, and bit-sliced witnesses of boolean built circuits
    fn zk_builder_create(out: *mut *mut ZkBuilder) -> c_int;
    fn zk_builder_free(b: *mut ZkBuilder);
    fn zk_builder_last_error(b: *const ZkBuilder) -> *const c_char;
    fn zk_builder_dims(b: *const ZkBuilder, wires: *mut usize, gates: *mut usize) -> c_int;
    fn zk_builder_new_wires(b: *mut ZkBuilder, kind: c_int, count: usize, out: *mut u32) -> c_int;
    fn zk_builder_sub_circuit(b: *mut ZkBuilder, left_weights: *const u64, left_wires: *const u32, nl: usize, right_weights: *const u64,
                              right_wires: *const u32, nr: usize, out: *mut u32) -> c_int;
    fn zk_builder_gate(b: *mut ZkBuilder, kind: c_int, x: u32, y: u32, out: *mut u32) -> c_int;
    fn zk_builder_bitwise(b: *mut ZkBuilder, kind: c_int, x: *const u32, y: *const u32, n: usize, out: *mut u32) -> c_int;
    fn zk_builder_fan_in(b: *mut ZkBuilder, kind: c_int, x: *const u32, n: usize, out: *mut u32) -> c_int;
    fn zk_builder_compare(b: *mut ZkBuilder, kind: c_int, left: *const u32, right: *const u32, n_bits: usize, out: *mut u32) -> c_int;
    fn zk_builder_keccak(b: *mut ZkBuilder, in_wires: *const u32, n_bytes: usize, rate_bytes: c_uint, delim: c_uint, rounds: c_uint,
                         out_wires: *mut u32, out_bytes: usize) -> c_int;
    fn zk_builder_assert_bit(b: *mut ZkBuilder, wire: u32) -> c_int;
    fn zk_builder_pack(b: *mut ZkBuilder, bits: *const u32, n_bits: usize, out: *mut u32) -> c_int;
    fn zk_builder_poseidon(b: *mut ZkBuilder, in_wires: *const u32, arity: usize, out: *mut u32) -> c_int;
    fn zk_builder_merkle_root(b: *mut ZkBuilder, leaf: u32, siblings: *const u32, dirs: *const u32, depth: usize, out: *mut u32) -> c_int;
    fn zk_builder_finish(b: *mut ZkBuilder, verify_wires: *const u32, n_verify: usize, out: *mut *mut ZkCircuit) -> c_int;
    fn zk_circuit_is_boolean(c: *const ZkCircuit) -> c_int;
    fn zk_circuit_packed_wires(c: *const ZkCircuit, count: *mut usize) -> c_int;
    fn zk_circuit_wire_index(c: *const ZkCircuit, wire: u32, index: *mut usize) -> c_int;
    fn zk_circuit_qap_sparse_unity(ctx: *mut ZkCtx, c: *const ZkCircuit, out: *mut *mut ZkQap) -> c_int;
    fn zk_circuit_mixed_dims(c: *const ZkCircuit, n_bit_inputs: *mut usize, n_field_inputs: *mut usize, core_ops: *mut usize, core_levels: *mut usize,
                             tail_ops: *mut usize, tail_levels: *mut usize, tail_slots: *mut usize) -> c_int;
    fn zk_circuit_weights_mixed(c: *const ZkCircuit, in_bits: *const u8, n_bit_bytes: usize, in_fields: *const u64, n_field: usize,
                                weights_out: *mut u64, m: usize) -> c_int;
    fn zk_mixgen_create(ctx: *mut ZkCtx, c: *const ZkCircuit, out: *mut *mut ZkMixgen) -> c_int;
    fn zk_mixgen_free(g: *mut ZkMixgen);
    fn zk_mixgen_run(g: *mut ZkMixgen, d_in_bits: *const c_void, in_stride_bytes: usize, d_in_fields: *const c_void, count: usize,
                     d_weights_out: *mut c_void, m: usize) -> c_int;
    fn zk_mixgen_eval_fields(g: *mut ZkMixgen, d_in_bits: *const c_void, in_stride_bytes: usize, d_in_fields: *const c_void, count: usize,
                             wires: *const u32, n_wires: usize, d_out_words: *mut c_void) -> c_int;
    // Baby Jubjub over Fr: builder gadgets, host arithmetic, GPU batch scalar multiplication
    fn zk_builder_babyjub_assert_on_curve(b: *mut ZkBuilder, xy: *const u32) -> c_int;
    fn zk_builder_babyjub_add(b: *mut ZkBuilder, p: *const u32, q: *const u32, out: *mut u32) -> c_int;
    fn zk_builder_babyjub_mul_fixed(b: *mut ZkBuilder, bits: *const u32, n_bits: usize, out: *mut u32) -> c_int;
    fn zk_builder_babyjub_mul(b: *mut ZkBuilder, p_xy: *const u32, bits: *const u32, n_bits: usize, out: *mut u32) -> c_int;
    fn zk_builder_babyjub_affine(b: *mut ZkBuilder, p: *const u32, xy: *const u32) -> c_int;
    fn zk_babyjub_params(a: *mut u64, d: *mut u64, order: *mut u64, base8: *mut u64, generator: *mut u64) -> c_int;
    fn zk_babyjub_on_curve(p: *const u64) -> c_int;
    fn zk_babyjub_add(p: *const u64, q: *const u64, out: *mut u64) -> c_int;
    fn zk_babyjub_mul(scalar: *const u64, p: *const u64, out: *mut u64) -> c_int;
    fn zk_babyjub_mul_batch(ctx: *mut ZkCtx, d_scalars: *const c_void, d_points: *const c_void, count: usize, d_out: *mut c_void,
                            out_stride_words: usize) -> c_int;
    // EdDSA-Poseidon on Baby Jubjub: the gadget, host sign / verify, GPU batch verification
    fn zk_builder_eddsa_verify(b: *mut ZkBuilder, a_xy: *const u32, r8_xy: *const u32, msg: u32, s_bits: *const u32, hm_bits: *const u32) -> c_int;
    fn zk_eddsa_challenge(r8: *const u64, a: *const u64, msg: *const u64, out: *mut u64) -> c_int;
    fn zk_eddsa_public_key(k: *const u64, out: *mut u64) -> c_int;
    fn zk_eddsa_sign(k: *const u64, nonce_key: *const u64, msg: *const u64, r8_out: *mut u64, s_out: *mut u64) -> c_int;
    fn zk_eddsa_verify(a: *const u64, msg: *const u64, r8: *const u64, s: *const u64, status: *mut c_int) -> c_int;
    fn zk_eddsa_verify_batch(ctx: *mut ZkCtx, d_points_msg: *const c_void, d_s: *const c_void, count: usize, d_status: *mut c_void,
                             d_bits_out: *mut c_void, bits_stride_bytes: usize) -> c_int;
    fn zk_eddsa_sign_batch(ctx: *mut ZkCtx, d_keys: *const c_void, d_nonce_keys: *const c_void, d_msgs: *const c_void, count: usize,
                           d_points_msg_out: *mut c_void, d_s_out: *mut c_void, d_bits_out: *mut c_void, bits_stride_bytes: usize) -> c_int;
    // Poseidon over Fr (circomlib's parameter sets): host hash, GPU batch hashing, a device-resident Merkle tree and its paths
    fn zk_poseidon_hash(inputs: *const u64, arity: usize, out: *mut u64) -> c_int;
    fn zk_poseidon_params(arity: usize, rf: *mut c_uint, rp: *mut c_uint, round_constants: *mut u64, mds: *mut u64) -> c_int;
    fn zk_poseidon_hash_batch(ctx: *mut ZkCtx, d_inputs: *const c_void, arity: usize, count: usize, d_out: *mut c_void) -> c_int;
    fn zk_poseidon_tree_build(ctx: *mut ZkCtx, d_leaves: *const c_void, n_leaves: usize, depth: c_uint, out: *mut *mut ZkPoseidonTree) -> c_int;
    fn zk_poseidon_tree_free(t: *mut ZkPoseidonTree);
    fn zk_poseidon_tree_root(t: *const ZkPoseidonTree, out: *mut u64) -> c_int;
    fn zk_poseidon_tree_dims(t: *const ZkPoseidonTree, n_leaves: *mut usize, depth: *mut c_uint) -> c_int;
    fn zk_poseidon_tree_nodes(t: *const ZkPoseidonTree, level: c_uint, out: *mut u64) -> c_int;
    fn zk_poseidon_tree_paths(t: *mut ZkPoseidonTree, d_indices: *const c_void, count: usize, d_fields_out: *mut c_void, field_stride_words: usize,
                              d_bits_out: *mut c_void, bits_stride_bytes: usize) -> c_int;
    fn zk_poseidon_tree_update(t: *mut ZkPoseidonTree, d_indices: *const c_void, d_values: *const c_void, count: usize) -> c_int;
    fn zk_poseidon_tree_append(t: *mut ZkPoseidonTree, d_leaves: *const c_void, count: usize) -> c_int;
    fn zk_boolgen_create(ctx: *mut ZkCtx, c: *const ZkCircuit, out: *mut *mut ZkBoolgen) -> c_int;
    fn zk_boolgen_free(g: *mut ZkBoolgen);
    fn zk_boolgen_run(g: *mut ZkBoolgen, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, d_weights_out: *mut c_void,
                      m: usize) -> c_int;
    fn zk_boolgen_eval_fields(g: *mut ZkBoolgen, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, wires: *const u32, n_wires: usize,
                              d_out_words: *mut c_void) -> c_int;
    fn zk_boolgen_eval(g: *mut ZkBoolgen, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, wires: *const u32, n_wires: usize,
                       d_out_bits: *mut c_void, out_stride_bytes: usize) -> c_int;
    // does a witness satisfy the QAP (sparse forms)?  One witness on the host, or `count` of them where zk_witgen_run left them
    fn zk_qap_check(ctx: *mut ZkCtx, qap: *const ZkQap, weights: *const u64, m: usize, out: *mut ZkQapCheckResult) -> c_int;
    fn zk_qap_check_dev(ctx: *mut ZkCtx, qap: *const ZkQap, d_weights: *const c_void, m: usize, stride: usize, count: usize,
                        out: *mut ZkQapCheckResult) -> c_int;
    // is the CRS a Groth16 CRS of some trapdoor for this QAP?  challenge = null: drawn from the OS inside the library
    fn zk_crs_check(ctx: *mut ZkCtx, crs: *const ZkCrs, qap: *const ZkQap, challenge: *const u64, out: *mut ZkCrsCheckResult) -> c_int;
    // the head of a ceremony: the QAP's CRS from a powers-of-tau transcript, gamma = delta = 1, group operations only
    fn zk_crs_from_powers(ctx: *mut ZkCtx, qap: *const ZkQap, powers: *const ZkPowersDesc, out: *mut *mut ZkCrs) -> c_int;
    // delta contributions: a new CRS with delta' = d delta (d = null: drawn from the OS, wiped), the record that proves knowledge of
    // d for a 32-byte tag, and the check that `after` is `before` with only delta re-keyed
    fn zk_crs_contribute(ctx: *mut ZkCtx, crs: *const ZkCrs, d: *const u64, tag: *const u8, out: *mut *mut ZkCrs,
                         contribution: *mut ZkCrsContribution) -> c_int;
    fn zk_crs_contribution_verify(c: *const ZkCrsContribution, tag: *const u8, ok: *mut c_int) -> c_int;
    fn zk_crs_contribution_check(ctx: *mut ZkCtx, before: *const ZkCrs, after: *const ZkCrs, c: *const ZkCrsContribution, tag: *const u8,
                                 challenge: *const u64, out: *mut ZkCrsContributionResult) -> c_int;
    // phase 1: a resident powers-of-tau transcript, its check, a contribution (secrets = null: drawn from the OS, wiped) and the
    // check of a contribution; the per-point multiplication kernel behind it on chosen scalars
    fn zk_powers_upload(ctx: *mut ZkCtx, desc: *const ZkPowersDesc, out: *mut *mut ZkPowers) -> c_int;
    fn zk_powers_initial(ctx: *mut ZkCtx, n_tau_g1: usize, n_rest: usize, out: *mut *mut ZkPowers) -> c_int;
    fn zk_powers_dims(powers: *const ZkPowers, n_tau_g1: *mut usize, n_rest: *mut usize) -> c_int;
    fn zk_powers_download(ctx: *mut ZkCtx, powers: *const ZkPowers, out: *const ZkPowersOut) -> c_int;
    fn zk_powers_free(powers: *mut ZkPowers);
    fn zk_powers_check(ctx: *mut ZkCtx, powers: *const ZkPowers, challenge: *const u64, out: *mut ZkPowersCheckResult) -> c_int;
    fn zk_powers_contribution_prove(before: *const u64, secrets: *const u64, nonces: *const u64, tag: *const u8,
                                    out: *mut ZkPowersContribution) -> c_int;
    fn zk_powers_contribution_verify(c: *const ZkPowersContribution, tag: *const u8, ok: *mut c_int) -> c_int;
    fn zk_powers_contribute(ctx: *mut ZkCtx, before: *const ZkPowers, secrets: *const u64, tag: *const u8, out: *mut *mut ZkPowers,
                            record: *mut ZkPowersContribution) -> c_int;
    fn zk_powers_contribution_check(ctx: *mut ZkCtx, before: *const ZkPowers, after: *const ZkPowers, record: *const ZkPowersContribution,
                                    tag: *const u8, challenge: *const u64, out: *mut ZkPowersCheckResult) -> c_int;
    fn zk_g1_mul_each(ctx: *mut ZkCtx, points: *const u64, scalars: *const u64, out: *mut u64, n: usize) -> c_int;
    fn zk_g2_mul_each(ctx: *mut ZkCtx, points: *const u64, scalars: *const u64, out: *mut u64, n: usize) -> c_int;
    // a stream of proofs: witnesses in page-locked host memory, two tickets in flight
    fn zk_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    fn zk_host_free(p: *mut c_void);
    fn zk_prove_submit_host(ctx: *mut ZkCtx, crs: *const ZkCrs, qap: *const ZkQap, weights: *const u64, m: usize,
                            r: *const u64, s: *const u64, ticket: *mut c_int) -> c_int;
    fn zk_prove_wait(ctx: *mut ZkCtx, ticket: c_int, proof_out: *mut u8) -> c_int;
    // several GPUs, one process (or thread) per GPU: a communicator + the scalar-exchange pipeline
    fn zk_device_count() -> c_int;
    fn zk_comm_unique_id(id_out: *mut u8) -> c_int;
    fn zk_comm_init(ctx: *mut ZkCtx, id: *const u8, rank: c_int, world: c_int, out: *mut *mut ZkComm) -> c_int;
    fn zk_comm_destroy(c: *mut ZkComm);
    fn zk_comm_set_timeout(c: *mut ZkComm, ms: std::os::raw::c_long) -> c_int;
    fn zk_comm_rccl_ranks(c: *const ZkComm) -> c_int;
    fn zk_mgpu_create(ctx: *mut ZkCtx, comm: *mut ZkComm, crs: *const ZkCrs, qap: *const ZkQap, out: *mut *mut ZkMgpu) -> c_int;
    fn zk_mgpu_push_host(p: *mut ZkMgpu, weights: *const u64, m: usize, r: *const u64, s: *const u64) -> c_int;
    fn zk_mgpu_pop(p: *mut ZkMgpu, proof_out: *mut u8) -> c_int;
    fn zk_mgpu_destroy(p: *mut ZkMgpu);
    fn zk_mgpu_last_error(p: *const ZkMgpu) -> *const c_char;
}
#[repr(C)] pub struct ZkComm { _p: [u8; 0] }
#[repr(C)] pub struct ZkCircuit { _p: [u8; 0] }
#[repr(C)] pub struct ZkWitgen { _p: [u8; 0] }
#[repr(C)] pub struct ZkBuilder { _p: [u8; 0] }
#[repr(C)] pub struct ZkBoolgen { _p: [u8; 0] }
#[repr(C)] pub struct ZkMixgen { _p: [u8; 0] }
#[repr(C)] pub struct ZkPoseidonTree { _p: [u8; 0] }
#[repr(C)] pub struct ZkMgpu { _p: [u8; 0] }

fn check(ctx: *mut ZkCtx, rc: c_int) {
    // the reference panics on division by zero / zero divisor (fr.rs:54,69; field/mod.rs:440); so does the shim
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(zk_last_error(ctx)) }.to_string_lossy().into_owned();
        panic!("{}", if rc == -5 { "Dividend must be non-zero".to_string() } else { msg });
    }
}

// ------------------------------------------------------------------------------------------------
// bn values <-> the ABI's element layout.  bn 0.4.3 keeps its field and group types opaque; what it does expose is
// rustc-serialize `Encodable` / `Decodable` (the README's own example serialises G1 through them):
//     Fr, Fq : 32 bytes, big-endian canonical integer
//     G1     : 0x00                      (identity)   |  0x04, x, y                 (affine, 32 + 32 bytes)
//     G2     : 0x00                      (identity)   |  0x04, X, Y                 (64 + 64 bytes), each Fq2 coordinate
//              packed as the 512-bit big-endian integer  c1 * q + c0
// [layout from the bn sources as remembered -- SURVEY F3: to be confirmed on a machine that has the crate; the unit
//  test at the end of this file does that in one `cargo test`].
// A byte sink / source implementing rustc_serialize::{Encoder, Decoder} captures exactly those bytes without bincode.
// ------------------------------------------------------------------------------------------------
mod bn_bytes {
    use super::rustc_serialize::{Decodable, Decoder, Encodable, Encoder};

    pub struct Sink(pub Vec<u8>);
    macro_rules! refuse { ($($name:ident : $t:ty),*) => { $(fn $name(&mut self, _: $t) -> Result<(), ()> { Err(()) })* } }
    impl Encoder for Sink {
        type Error = ();
        fn emit_nil(&mut self) -> Result<(), ()> { Ok(()) }
        fn emit_u8(&mut self, v: u8) -> Result<(), ()> { self.0.push(v); Ok(()) }
        refuse!(emit_usize: usize, emit_u64: u64, emit_u32: u32, emit_u16: u16, emit_isize: isize, emit_i64: i64, emit_i32: i32,
                emit_i16: i16, emit_i8: i8, emit_bool: bool, emit_f64: f64, emit_f32: f32, emit_char: char, emit_str: &str);
        fn emit_enum<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, f: F) -> Result<(), ()> { f(self) }
        fn emit_enum_variant<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_enum_variant_arg<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_enum_struct_variant<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_enum_struct_variant_field<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_struct<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_struct_field<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_tuple<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_tuple_arg<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_tuple_struct<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: &str, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_tuple_struct_arg<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_option<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, f: F) -> Result<(), ()> { f(self) }
        fn emit_option_none(&mut self) -> Result<(), ()> { Err(()) }
        fn emit_option_some<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, f: F) -> Result<(), ()> { f(self) }
        fn emit_seq<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_seq_elt<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_map<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_map_elt_key<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
        fn emit_map_elt_val<F: FnOnce(&mut Self) -> Result<(), ()>>(&mut self, _: usize, f: F) -> Result<(), ()> { f(self) }
    }

    pub struct Source<'a> { pub bytes: &'a [u8], pub pos: usize }
    macro_rules! refuse_read { ($($name:ident : $t:ty),*) => { $(fn $name(&mut self) -> Result<$t, String> { Err("not a byte".into()) })* } }
    impl<'a> Decoder for Source<'a> {
        type Error = String;
        fn read_nil(&mut self) -> Result<(), String> { Ok(()) }
        fn read_u8(&mut self) -> Result<u8, String> {
            let b = *self.bytes.get(self.pos).ok_or_else(|| "short input".to_string())?;
            self.pos += 1;
            Ok(b)
        }
        refuse_read!(read_usize: usize, read_u64: u64, read_u32: u32, read_u16: u16, read_isize: isize, read_i64: i64, read_i32: i32,
                     read_i16: i16, read_i8: i8, read_bool: bool, read_f64: f64, read_f32: f32, read_char: char, read_str: String);
        fn read_enum<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: &str, f: F) -> Result<T, String> { f(self) }
        fn read_enum_variant<T, F: FnMut(&mut Self, usize) -> Result<T, String>>(&mut self, _: &[&str], _: F) -> Result<T, String> { Err("enum".into()) }
        fn read_enum_variant_arg<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_enum_struct_variant<T, F: FnMut(&mut Self, usize) -> Result<T, String>>(&mut self, _: &[&str], _: F) -> Result<T, String> { Err("enum".into()) }
        fn read_enum_struct_variant_field<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: &str, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_struct<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: &str, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_struct_field<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: &str, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_tuple<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_tuple_arg<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_tuple_struct<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: &str, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_tuple_struct_arg<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_option<T, F: FnMut(&mut Self, bool) -> Result<T, String>>(&mut self, mut f: F) -> Result<T, String> { f(self, true) }
        fn read_seq<T, F: FnOnce(&mut Self, usize) -> Result<T, String>>(&mut self, _: F) -> Result<T, String> { Err("seq".into()) }
        fn read_seq_elt<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_map<T, F: FnOnce(&mut Self, usize) -> Result<T, String>>(&mut self, _: F) -> Result<T, String> { Err("map".into()) }
        fn read_map_elt_key<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn read_map_elt_val<T, F: FnOnce(&mut Self) -> Result<T, String>>(&mut self, _: usize, f: F) -> Result<T, String> { f(self) }
        fn error(&mut self, err: &str) -> String { err.to_string() }
    }

    pub fn encode<T: Encodable>(v: &T) -> Vec<u8> {
        let mut s = Sink(Vec::with_capacity(129));
        v.encode(&mut s).expect("bn value that does not encode to bytes");
        s.0
    }
    pub fn decode<T: Decodable>(bytes: &[u8]) -> T {
        let mut d = Source { bytes, pos: 0 };
        let v = T::decode(&mut d).expect("bytes that bn refuses (off-curve / out of range)");
        assert_eq!(d.pos, bytes.len(), "trailing bytes");
        v
    }

    // ---- 32-byte big-endian <-> [u64; 4] little-endian words (the ABI's Fr / Fq) ----
    pub fn be32_to_words(be: &[u8]) -> [u64; 4] {
        let mut w = [0u64; 4];
        for i in 0..4 { for b in 0..8 { w[i] = (w[i] << 8) | be[(3 - i) * 8 + b] as u64; } }
        w
    }
    pub fn words_to_be32(w: &[u64], out: &mut [u8]) {
        for i in 0..4 { for b in 0..8 { out[(3 - i) * 8 + b] = (w[i] >> (8 * (7 - b))) as u8; } }
    }

    // ---- bn's Fq2 packing: the 512-bit integer c1 * q + c0  <->  (c0, c1) ----
    pub const Q: [u64; 4] = [0x3c208c16d87cfd47, 0x97816a916871ca8d, 0xb85045b68181585d, 0x30644e72e131a029];   // Fq modulus
    /// 64 bytes big-endian -> (c0, c1) by schoolbook long division of the 512-bit value by q (c1 < q because X < q^2)
    pub fn u512_to_fq2(be: &[u8]) -> ([u64; 4], [u64; 4]) {
        let mut rem = [0u64; 5];            // running remainder, < 2 q < 2^255: 4 words + guard
        let mut quo = [0u64; 4];
        for bit in 0..512 {
            let byte = be[bit / 8];
            let inb = ((byte >> (7 - bit % 8)) & 1) as u64;
            for k in (1..5).rev() { rem[k] = (rem[k] << 1) | (rem[k - 1] >> 63); }      // rem = rem * 2 + bit
            rem[0] = (rem[0] << 1) | inb;
            let ge = rem[4] != 0 || { let mut g = true; for k in (0..4).rev() { if rem[k] != Q[k] { g = rem[k] > Q[k]; break; } } g };
            for k in (1..4).rev() { quo[k] = (quo[k] << 1) | (quo[k - 1] >> 63); }
            quo[0] <<= 1;
            if ge {
                let mut borrow = 0u64;
                for k in 0..4 { let (d1, b1) = rem[k].overflowing_sub(Q[k]); let (d2, b2) = d1.overflowing_sub(borrow); rem[k] = d2; borrow = (b1 | b2) as u64; }
                rem[4] = rem[4].wrapping_sub(borrow);
                quo[0] |= 1;
            }
        }
        ([rem[0], rem[1], rem[2], rem[3]], quo)      // (c0 = X mod q, c1 = X div q)
    }
    /// (c0, c1) -> 64 bytes big-endian of c1 * q + c0
    pub fn fq2_to_u512(c0: &[u64], c1: &[u64], out: &mut [u8]) {
        let mut acc = [0u64; 8];
        for i in 0..4 {
            let mut carry = 0u128;
            for j in 0..4 {
                let t = acc[i + j] as u128 + (c1[i] as u128) * (Q[j] as u128) + carry;
                acc[i + j] = t as u64;
                carry = t >> 64;
            }
            acc[i + 4] = carry as u64;      // the row's top word is untouched so far
        }
        let mut carry = 0u128;
        for k in 0..8 { let t = acc[k] as u128 + if k < 4 { c0[k] as u128 } else { 0 } + carry; acc[k] = t as u64; carry = t >> 64; }
        for k in 0..8 { for b in 0..8 { out[(7 - k) * 8 + b] = (acc[k] >> (8 * (7 - b))) as u8; } }
    }
}

// ---- the five conversion helpers (INTEGRATION.md promised them; here they are) ----
pub fn fr_to_words(x: &FrLocal) -> [u64; 4] { bn_bytes::be32_to_words(&bn_bytes::encode(&x.bn())) }
pub fn fr_from_words(w: &[u64]) -> FrLocal {
    let mut be = [0u8; 32];
    bn_bytes::words_to_be32(w, &mut be);
    FrLocal::from_bn(bn_bytes::decode(&be))
}
/// G1 -> x | y as 2 x 4 words, identity = all zero (the ABI's convention)
pub fn g1_to_words(p: &G1Local) -> [u64; 8] {
    let b = bn_bytes::encode(&p.bn());
    let mut w = [0u64; 8];
    if b[0] == 4 {
        w[..4].copy_from_slice(&bn_bytes::be32_to_words(&b[1..33]));
        w[4..].copy_from_slice(&bn_bytes::be32_to_words(&b[33..65]));
    }
    w
}
/// G2 -> x.c0 | x.c1 | y.c0 | y.c1 as 4 x 4 words, identity = all zero
pub fn g2_to_words(p: &G2Local) -> [u64; 16] {
    let b = bn_bytes::encode(&p.bn());
    let mut w = [0u64; 16];
    if b[0] == 4 {
        let (x0, x1) = bn_bytes::u512_to_fq2(&b[1..65]);
        let (y0, y1) = bn_bytes::u512_to_fq2(&b[65..129]);
        w[0..4].copy_from_slice(&x0); w[4..8].copy_from_slice(&x1); w[8..12].copy_from_slice(&y0); w[12..16].copy_from_slice(&y1);
    }
    w
}
fn g1_from_words(w: &[u64]) -> G1Local {
    if w.iter().all(|&x| x == 0) { return G1Local::from_bn(bn_bytes::decode(&[0u8])); }
    let mut b = [0u8; 65];
    b[0] = 4;
    bn_bytes::words_to_be32(&w[0..4], &mut b[1..33]);
    bn_bytes::words_to_be32(&w[4..8], &mut b[33..65]);
    G1Local::from_bn(bn_bytes::decode(&b))
}
fn g2_from_words(w: &[u64]) -> G2Local {
    if w.iter().all(|&x| x == 0) { return G2Local::from_bn(bn_bytes::decode(&[0u8])); }
    let mut b = [0u8; 129];
    b[0] = 4;
    bn_bytes::fq2_to_u512(&w[0..4], &w[4..8], &mut b[1..65]);
    bn_bytes::fq2_to_u512(&w[8..12], &w[12..16], &mut b[65..129]);
    G2Local::from_bn(bn_bytes::decode(&b))
}
/// the 65-byte G1 block of a proof (0x04 | x | y, or 0x00 + zeros) -> G1Local.  Same bytes as bn's own encoding.
pub fn g1_from_bytes(p: &[u8]) -> G1Local {
    assert_eq!(p.len(), 65);
    if p[0] == 0 { G1Local::from_bn(bn_bytes::decode(&[0u8])) } else { G1Local::from_bn(bn_bytes::decode(p)) }
}
/// the 129-byte G2 block (0x04 | x.c1 | x.c0 | y.c1 | y.c0, EIP-197 order) -> G2Local
pub fn g2_from_bytes(p: &[u8]) -> G2Local {
    assert_eq!(p.len(), 129);
    if p[0] == 0 { return G2Local::from_bn(bn_bytes::decode(&[0u8])); }
    let mut w = [0u64; 16];
    w[4..8].copy_from_slice(&bn_bytes::be32_to_words(&p[1..33]));      // x.c1
    w[0..4].copy_from_slice(&bn_bytes::be32_to_words(&p[33..65]));     // x.c0
    w[12..16].copy_from_slice(&bn_bytes::be32_to_words(&p[65..97]));   // y.c1
    w[8..12].copy_from_slice(&bn_bytes::be32_to_words(&p[97..129]));   // y.c0
    g2_from_words(&w)
}
fn g1_to_bytes(p: &G1Local, out: &mut [u8]) {
    let w = g1_to_words(p);
    if w.iter().all(|&x| x == 0) { for b in out.iter_mut() { *b = 0; } return; }
    out[0] = 4;
    bn_bytes::words_to_be32(&w[0..4], &mut out[1..33]);
    bn_bytes::words_to_be32(&w[4..8], &mut out[33..65]);
}
fn g2_to_bytes(p: &G2Local, out: &mut [u8]) {
    let w = g2_to_words(p);
    if w.iter().all(|&x| x == 0) { for b in out.iter_mut() { *b = 0; } return; }
    out[0] = 4;
    bn_bytes::words_to_be32(&w[4..8], &mut out[1..33]);
    bn_bytes::words_to_be32(&w[0..4], &mut out[33..65]);
    bn_bytes::words_to_be32(&w[12..16], &mut out[65..97]);
    bn_bytes::words_to_be32(&w[8..12], &mut out[97..129]);
}
fn proof_from_bytes(b: &[u8; 259]) -> Proof<G1Local, G2Local> {
    Proof { a: g1_from_bytes(&b[0..65]), b: g2_from_bytes(&b[65..194]), c: g1_from_bytes(&b[194..259]) }
}
fn proof_to_bytes(p: &Proof<G1Local, G2Local>) -> [u8; 259] {
    let mut b = [0u8; 259];
    g1_to_bytes(&p.a, &mut b[0..65]);
    g2_to_bytes(&p.b, &mut b[65..194]);
    g1_to_bytes(&p.c, &mut b[194..259]);
    b
}

/// The compressed form of a proof (zkgpu.h "Compressed proof bytes"): A 32 | B 64 | C 32 bytes, x coordinates big-endian with
/// the sign of y (taken on the canonical integer) in the two top bits of each block.  Host code: no device is involved.
impl Proof<G1Local, G2Local> {
    pub fn to_compressed(&self) -> [u8; 128] {
        let (bytes, mut out) = (proof_to_bytes(self), [0u8; 128]);
        let st = unsafe { zk_proof_compress(bytes.as_ptr(), out.as_mut_ptr()) };
        assert!(st == 0, "zk_proof_compress: status {}", st);   // bn's points are on their curves: cannot fail for a Proof
        out
    }
    /// None unless all three blocks are valid encodings of points on their curves.  B's subgroup is not tested here: verify does.
    pub fn from_compressed(c: &[u8; 128]) -> Option<Self> {
        let mut bytes = [0u8; 259];
        let st = unsafe { zk_proof_decompress(c.as_ptr(), bytes.as_mut_ptr()) };
        if st == 0 { Some(proof_from_bytes(&bytes)) } else { None }
    }
}

fn g1s(ps: &[G1Local]) -> Vec<u64> { ps.iter().flat_map(|p| g1_to_words(p).to_vec()).collect() }
fn g2s(ps: &[G2Local]) -> Vec<u64> { ps.iter().flat_map(|p| g2_to_words(p).to_vec()).collect() }
fn frs(xs: &[FrLocal]) -> Vec<u64> { xs.iter().flat_map(|x| fr_to_words(x).to_vec()).collect() }

// ------------------------------------------------------------------------------------------------
// Context, device-resident QAP / CRS
// ------------------------------------------------------------------------------------------------
struct Ctx(*mut ZkCtx);
impl Ctx {
    fn new() -> Ctx {
        let mut ctx = std::ptr::null_mut();
        let dev: c_int = std::env::var("ZKGPU_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
        assert!(unsafe { zk_device_count() } > dev, "no MI355X visible (there is no CPU fallback)");
        assert_eq!(unsafe { zk_ctx_create(dev, &mut ctx) }, 0, "zk_ctx_create failed");
        Ctx(ctx)
    }
}
impl Drop for Ctx { fn drop(&mut self) { unsafe { zk_ctx_destroy(self.0) } } }

// ------------------------------------------------------------------------------------------------
// Phase 1: a powers-of-tau transcript on the device for the length of one call
// ------------------------------------------------------------------------------------------------
struct ResidentPowers<'c> { ctx: &'c Ctx, p: *mut ZkPowers }
impl<'c> Drop for ResidentPowers<'c> { fn drop(&mut self) { unsafe { zk_powers_free(self.p) } } }
impl<'c> ResidentPowers<'c> {
    fn upload(ctx: &'c Ctx, t: &PowersOfTau) -> ResidentPowers<'c> {
        let n_rest = t.tau_g2.len() / 16;
        assert!(t.tau_g1.len() % 8 == 0 && t.tau_g2.len() % 16 == 0, "a G1 point is 8 words, a G2 point 16");
        assert!(t.alpha_tau_g1.len() == 8 * n_rest && t.beta_tau_g1.len() == 8 * n_rest, "tau_g2, alpha_tau_g1, beta_tau_g1 differ in length");
        let desc = ZkPowersDesc { n_tau_g1: t.tau_g1.len() / 8, n_rest, tau_g1: t.tau_g1.as_ptr(), tau_g2: t.tau_g2.as_ptr(),
                                  alpha_tau_g1: t.alpha_tau_g1.as_ptr(), beta_tau_g1: t.beta_tau_g1.as_ptr(), beta_g2: t.beta_g2.as_ptr() };
        let mut p: *mut ZkPowers = std::ptr::null_mut();
        check(ctx.0, unsafe { zk_powers_upload(ctx.0, &desc, &mut p) });
        ResidentPowers { ctx, p }
    }
    fn download(&self) -> PowersOfTauOwned {
        let (mut n1, mut n2) = (0usize, 0usize);
        check(self.ctx.0, unsafe { zk_powers_dims(self.p, &mut n1, &mut n2) });
        let mut t = PowersOfTauOwned { tau_g1: vec![0; 8 * n1], tau_g2: vec![0; 16 * n2], alpha_tau_g1: vec![0; 8 * n2], beta_tau_g1: vec![0; 8 * n2],
                                       beta_g2: [0; 16] };
        let out = ZkPowersOut { tau_g1: t.tau_g1.as_mut_ptr(), tau_g2: t.tau_g2.as_mut_ptr(), alpha_tau_g1: t.alpha_tau_g1.as_mut_ptr(),
                                beta_tau_g1: t.beta_tau_g1.as_mut_ptr(), beta_g2: t.beta_g2.as_mut_ptr() };
        check(self.ctx.0, unsafe { zk_powers_download(self.ctx.0, self.p, &out) });
        t
    }
}
impl<'a> PowersOfTau<'a> {
    /// The head of a ceremony (zk_powers_initial): x = alpha = beta = 1, every entry a generator.
    pub fn initial(n_tau_g1: usize, n_rest: usize) -> PowersOfTauOwned {
        let ctx = Ctx::new();
        let mut p: *mut ZkPowers = std::ptr::null_mut();
        check(ctx.0, unsafe { zk_powers_initial(ctx.0, n_tau_g1, n_rest, &mut p) });
        ResidentPowers { ctx: &ctx, p }.download()
    }
    /// Is this a powers-of-tau sequence over the library's generators (zk_powers_check; the challenge is drawn from the OS inside the
    /// library)?  -> the failed ZK_POWERS_CHECK_* bits, 0 = a transcript.  Once per transcript, whatever the circuit.
    pub fn check(&self) -> u32 {
        let ctx = Ctx::new();
        let r = ResidentPowers::upload(&ctx, self);
        let mut res = ZkPowersCheckResult { failed: 0, flags: 0 };
        check(ctx.0, unsafe { zk_powers_check(ctx.0, r.p, std::ptr::null(), &mut res) });
        res.failed
    }
    /// Adds the caller's randomness (zk_powers_contribute): the transcript of (alpha a, beta b, x s) for secrets drawn from the OS
    /// inside the library, wiped and never returned, and the record that proves knowledge of them for `tag`.  The result is checked
    /// against this transcript before it is returned; a failure there is a bug and panics.
    pub fn contribute(&self, tag: &[u8; 32]) -> (PowersOfTauOwned, ZkPowersContribution) {
        let ctx = Ctx::new();
        let before = ResidentPowers::upload(&ctx, self);
        let mut rec = ZkPowersContribution([0u8; 672]);
        let mut next: *mut ZkPowers = std::ptr::null_mut();
        let mut res = ZkPowersCheckResult { failed: 0, flags: 0 };
        check(ctx.0, unsafe { zk_powers_contribute(ctx.0, before.p, std::ptr::null(), tag.as_ptr(), &mut next, &mut rec) });
        let after = ResidentPowers { ctx: &ctx, p: next };
        check(ctx.0, unsafe { zk_powers_contribution_check(ctx.0, before.p, after.p, &rec, tag.as_ptr(), std::ptr::null(), &mut res) });
        assert!(res.failed == 0, "zk_powers_contribute made a transcript its own check refuses: {:#x}", res.failed);
        (after.download(), rec)
    }
    /// Is this transcript `before` re-keyed by whoever made `record` for `tag`, and a transcript in its own right
    /// (zk_powers_contribution_check)?  -> the failed bits, 0 = a valid successor.  `before` is not checked again.
    pub fn check_contribution(&self, before: &PowersOfTau, record: &ZkPowersContribution, tag: &[u8; 32]) -> u32 {
        let ctx = Ctx::new();
        let (old, new) = (ResidentPowers::upload(&ctx, before), ResidentPowers::upload(&ctx, self));
        let mut res = ZkPowersCheckResult { failed: 0, flags: 0 };
        check(ctx.0, unsafe { zk_powers_contribution_check(ctx.0, old.p, new.p, record, tag.as_ptr(), std::ptr::null(), &mut res) });
        res.failed
    }
}
impl ZkPowersContribution {
    /// zk_powers_contribution_verify (host code, no GPU): do the three parts verify under their role tags for `tag`?
    pub fn verify(&self, tag: &[u8; 32]) -> bool {
        let mut ok: c_int = 0;
        assert_eq!(unsafe { zk_powers_contribution_verify(self, tag.as_ptr(), &mut ok) }, 0, "zk_powers_contribution_verify failed");
        ok != 0
    }
}

fn upload_dense(ctx: &Ctx, qap: &QAP<CoefficientPoly<FrLocal>>) -> *mut ZkQap {
    let (m, n) = (qap.u.len(), qap.degree);
    // dense m x n coefficient matrices, zero padded (coefficient k of wire i at [i*n + k]); CoefficientPoly derefs to [T]
    let dense = |ps: &Vec<CoefficientPoly<FrLocal>>| -> Vec<u64> {
        let mut out = vec![0u64; m * n * 4];
        for (i, p) in ps.iter().enumerate() {
            for (k, c) in p.iter().take(n).enumerate() { out[(i * n + k) * 4..][..4].copy_from_slice(&fr_to_words(c)); }
        }
        out
    };
    let (u, v, w) = (dense(&qap.u), dense(&qap.v), dense(&qap.w));
    let mut t = vec![0u64; (n + 1) * 4];
    for (k, c) in qap.t.iter().take(n + 1).enumerate() { t[4 * k..4 * k + 4].copy_from_slice(&fr_to_words(c)); }
    let mut q = std::ptr::null_mut();
    unsafe { check(ctx.0, zk_qap_upload_dense(ctx.0, u.as_ptr(), v.as_ptr(), w.as_ptr(), t.as_ptr(), m, n, qap.input, &mut q)); }
    q
}

fn upload_crs(ctx: &Ctx, s1: &SigmaG1<G1Local>, s2: &SigmaG2<G2Local>) -> (*mut ZkCrs, usize, usize, usize) {
    // dimensions as setup lays them out (mod.rs:146-194): |xi| = n, |sum_gamma| = l + 1, |sum_delta| = m - l - 1, |xi_t| = n - 1
    let (n, input) = (s1.xi.len(), s1.sum_gamma.len() - 1);
    let m = s1.sum_gamma.len() + s1.sum_delta.len();
    let (xi1, sg, sd, xt, xi2) = (g1s(&s1.xi), g1s(&s1.sum_gamma), g1s(&s1.sum_delta), g1s(&s1.xi_t), g2s(&s2.xi));
    let (a1, b1, d1) = (g1_to_words(&s1.alpha), g1_to_words(&s1.beta), g1_to_words(&s1.delta));
    let (b2, g2, d2) = (g2_to_words(&s2.beta), g2_to_words(&s2.gamma), g2_to_words(&s2.delta));
    let desc = ZkCrsDesc { n, m, input,
        alpha_g1: a1.as_ptr(), beta_g1: b1.as_ptr(), delta_g1: d1.as_ptr(),
        xi_g1: xi1.as_ptr(), sum_gamma_g1: sg.as_ptr(), sum_delta_g1: sd.as_ptr(), xi_t_g1: xt.as_ptr(),
        beta_g2: b2.as_ptr(), gamma_g2: g2.as_ptr(), delta_g2: d2.as_ptr(), xi_g2: xi2.as_ptr() };
    let mut c = std::ptr::null_mut();
    unsafe { check(ctx.0, zk_crs_upload(ctx.0, &desc, &mut c)); }   // range- and on-curve-checked on the GPU
    (c, n, m, input)
}

fn download_crs(ctx: &Ctx, crs: *const ZkCrs, n: usize, m: usize, l: usize) -> (SigmaG1<G1Local>, SigmaG2<G2Local>) {
    let (mut a1, mut b1, mut d1) = ([0u64; 8], [0u64; 8], [0u64; 8]);
    let (mut b2, mut g2, mut d2) = ([0u64; 16], [0u64; 16], [0u64; 16]);
    let (mut xi1, mut sg, mut sd, mut xt) = (vec![0u64; 8 * n], vec![0u64; 8 * (l + 1)], vec![0u64; 8 * (m - l - 1)], vec![0u64; 8 * (n - 1)]);
    let mut xi2 = vec![0u64; 16 * n];
    let out = ZkCrsOut { alpha_g1: a1.as_mut_ptr(), beta_g1: b1.as_mut_ptr(), delta_g1: d1.as_mut_ptr(),
        xi_g1: xi1.as_mut_ptr(), sum_gamma_g1: sg.as_mut_ptr(), sum_delta_g1: sd.as_mut_ptr(), xi_t_g1: xt.as_mut_ptr(),
        beta_g2: b2.as_mut_ptr(), gamma_g2: g2.as_mut_ptr(), delta_g2: d2.as_mut_ptr(), xi_g2: xi2.as_mut_ptr() };
    unsafe { check(ctx.0, zk_crs_download(ctx.0, crs, &out)); }
    let v1 = |w: &Vec<u64>| -> Vec<G1Local> { w.chunks(8).map(g1_from_words).collect() };
    (SigmaG1 { alpha: g1_from_words(&a1), beta: g1_from_words(&b1), delta: g1_from_words(&d1),
               xi: v1(&xi1), sum_gamma: v1(&sg), sum_delta: v1(&sd), xi_t: v1(&xt) },
     SigmaG2 { beta: g2_from_words(&b2), gamma: g2_from_words(&g2), delta: g2_from_words(&d2), xi: xi2.chunks(16).map(g2_from_words).collect() })
}

/// Device-resident copy of (QAP, CRS): upload once, prove many times.
pub struct GpuProver { ctx: Ctx, qap: *mut ZkQap, crs: *mut ZkCrs, n: usize, m: usize, input: usize }

impl GpuProver {
    /// from the reference's own types: dense QAP<CoefficientPoly<FrLocal>> + an existing CRS (any roots; up to 16384 gates)
    pub fn new(qap: &QAP<CoefficientPoly<FrLocal>>, sigma: (&SigmaG1<G1Local>, &SigmaG2<G2Local>)) -> Self {
        let ctx = Ctx::new();
        let q = upload_dense(&ctx, qap);
        let (crs, n, m, input) = upload_crs(&ctx, sigma.0, sigma.1);
        assert!(n == qap.degree && m == qap.u.len() && input == qap.input, "CRS and QAP dimensions differ");
        GpuProver { ctx, qap: q, crs, n, m, input }
    }

    /// Large circuits: the sparse form straight from a RootRepresentation (circuit/mod.rs:201-214) whose roots are
    /// 1, w, w^2, ... with w = 5^((r-1)/n), n = 2^log_n -- the dense QAP (3 m n field elements) is never built -- and a
    /// CRS made on the GPU (groth16::setup, mod.rs:134-197).  Returns the prover and the CRS in the reference's types.
    pub fn from_root_rep<R: RootRepresentation<FrLocal>>(rr: &R, log_n: u32) -> (Self, (SigmaG1<G1Local>, SigmaG2<G2Local>)) {
        let n = 1usize << log_n;
        let mut index: HashMap<[u64; 4], u32> = HashMap::with_capacity(n);
        // w = 5^((r-1)/n): built from the published 2^28-th root of unity by repeated squaring
        let mut w = "19103219067921713944291392827692070036145651957329286315305642004821462161904".parse::<FrLocal>().ok().expect("omega");
        for _ in log_n..28 { w = w * w; }
        let mut p = FrLocal::from(1usize);
        for (j, root) in rr.roots().enumerate() {
            assert!(j < n && root == p, "zk_qap_upload_sparse needs the roots 1, w, w^2, ... (use GpuProver::new for other roots)");
            index.insert(fr_to_words(&root), j as u32);
            p = p * w;
        }
        assert_eq!(index.len(), n, "the number of gates must be 2^log_n");
        Self::from_rows(rr, &index, n, Some(log_n), None, None)
    }

    /// The circuits the reference itself produces: a RootRepresentation over the roots 1, 2, .., n (ASTParser, circuit/mod.rs:517),
    /// any n up to 2^23, with the reference's proof bytes (zk_qap_upload_sparse_integers: nothing is interpolated).  Builder
    /// circuits (CircuitInstance, keccak) arrive here too once `From<&CircuitInstance> for DummyRep` stops pre-filling u, v, w with
    /// num_wires empty rows before pushing the real ones (circuit/mod.rs:163-165 then :186-188 -- SURVEY F8: as shipped, the
    /// first num_wires polynomials are zero and every proof verifies vacuously; `Vec::with_capacity` is the fix) and is
    /// instantiated with sub_circuit_point = |id| FrLocal::from(id + 1).
    pub fn from_root_rep_integers<R: RootRepresentation<FrLocal>>(rr: &R) -> (Self, (SigmaG1<G1Local>, SigmaG2<G2Local>)) {
        let mut index: HashMap<[u64; 4], u32> = HashMap::new();
        let mut k = FrLocal::from(1usize);
        let mut n = 0usize;
        for root in rr.roots() {
            assert!(root == k, "zk_qap_upload_sparse_integers needs the roots 1, 2, 3, ...");
            index.insert(fr_to_words(&root), n as u32);
            k = k + FrLocal::from(1usize);
            n += 1;
        }
        Self::from_rows(rr, &index, n, None, None, None)
    }

    /// ANY RootRepresentation (circuit/mod.rs:201-214: `roots()` is caller data, e.g. DummyRep's, dummy_rep.rs:47): the rows over the
    /// caller's distinct roots, at any size up to 2^22 gates, with the reference's proof bytes (zk_qap_upload_sparse_roots: the prover
    /// interpolates U and V per proof by a sub-product tree, nothing is interpolated per wire).  `sigma`: a CRS
    /// the reference's own `setup` made for the circuit, or None to make one on the GPU.
    pub fn from_root_rep_any<R: RootRepresentation<FrLocal>>(rr: &R, sigma: Option<(&SigmaG1<G1Local>, &SigmaG2<G2Local>)>)
        -> (Self, (SigmaG1<G1Local>, SigmaG2<G2Local>)) {
        let mut index: HashMap<[u64; 4], u32> = HashMap::new();
        let mut roots: Vec<u64> = Vec::new();
        for (j, root) in rr.roots().enumerate() {
            let w = fr_to_words(&root);
            assert!(index.insert(w, j as u32).is_none(), "the roots of a RootRepresentation must be distinct");
            roots.extend_from_slice(&w);
        }
        let n = index.len();
        Self::from_rows(rr, &index, n, None, sigma, Some(&roots))
    }

    /// The same circuits with a CRS the reference's own `setup` made (groth16::prove takes any (&SigmaG1, &SigmaG2), mod.rs:213-217):
    /// the library derives the Lagrange-basis points it multiplies with from [x^i]_1, [x^i]_2, [x^i t(x)/delta]_1 at the first proof
    /// (public linear combinations; once per CRS, O(n^2): n <= 2^16 + 2^10 gates); above that size it proves the same bytes
    /// through the sub-product tree of the roots 1..n.
    pub fn with_sigma_integers<R: RootRepresentation<FrLocal>>(rr: &R, sigma: (&SigmaG1<G1Local>, &SigmaG2<G2Local>)) -> Self {
        let mut index: HashMap<[u64; 4], u32> = HashMap::new();
        let mut k = FrLocal::from(1usize);
        let mut n = 0usize;
        for root in rr.roots() {
            assert!(root == k, "zk_qap_upload_sparse_integers needs the roots 1, 2, 3, ...");
            index.insert(fr_to_words(&root), n as u32);
            k = k + FrLocal::from(1usize);
            n += 1;
        }
        Self::from_rows(rr, &index, n, None, Some(sigma), None).0
    }

    fn from_rows<R: RootRepresentation<FrLocal>>(rr: &R, index: &HashMap<[u64; 4], u32>, n: usize, log_n: Option<u32>,
                                                 given: Option<(&SigmaG1<G1Local>, &SigmaG2<G2Local>)>, roots: Option<&Vec<u64>>)
        -> (Self, (SigmaG1<G1Local>, SigmaG2<G2Local>)) {
        struct Rows { ptr: Vec<u64>, gate: Vec<u32>, val: Vec<u64> }
        let collect = |rows: R::Row| -> Rows {
            let mut r = Rows { ptr: vec![0], gate: Vec::new(), val: Vec::new() };
            for col in rows {
                for (root, value) in col {
                    r.gate.push(index[&fr_to_words(&root)]);
                    r.val.extend_from_slice(&fr_to_words(&value));
                }
                r.ptr.push(r.gate.len() as u64);
            }
            r
        };
        let (u, v, wr) = (collect(rr.u()), collect(rr.v()), collect(rr.w()));
        let m = u.ptr.len() - 1;
        assert!(v.ptr.len() - 1 == m && wr.ptr.len() - 1 == m);      // fr.rs:157-158
        let raw = |r: &Rows| ZkSparseRows { ptr: r.ptr.as_ptr(), gate: r.gate.as_ptr(), val: r.val.as_ptr() };
        let desc = ZkQapSparseDesc { log_n: log_n.unwrap_or(0) as c_uint, m, input: rr.input(), u: raw(&u), v: raw(&v), w: raw(&wr) };
        let ctx = Ctx::new();
        let (mut q, mut crs) = (std::ptr::null_mut(), std::ptr::null_mut());
        let td: Vec<u64> = (0..5).flat_map(|_| fr_to_words(&FrLocal::random_elem()).to_vec()).collect();   // alpha, beta, gamma, delta, x (mod.rs:139-145)
        unsafe {
            match (log_n, roots) {
                (Some(_), _) => check(ctx.0, zk_qap_upload_sparse(ctx.0, &desc, &mut q)),
                (None, Some(r)) => check(ctx.0, zk_qap_upload_sparse_roots(ctx.0, &desc, r.as_ptr(), n, &mut q)),
                (None, None) => check(ctx.0, zk_qap_upload_sparse_integers(ctx.0, &desc, n, &mut q)),
            }
            match given {
                Some((s1, s2)) => {
                    let (c, cn, cm, cl) = upload_crs(&ctx, s1, s2);
                    assert!(cn == n && cm == m && cl == rr.input(), "CRS and circuit dimensions differ");
                    crs = c;
                }
                None => check(ctx.0, zk_setup(ctx.0, q, td.as_ptr(), &mut crs)),
            }
        }
        let sigma = download_crs(&ctx, crs, n, m, rr.input());
        (GpuProver { ctx, qap: q, crs, n, m, input: rr.input() }, sigma)
    }

    /// groth16::prove with (r, s) injected (the reference draws them inside, mod.rs:231).
    pub fn prove_with_rs(&self, weights: &[FrLocal], r: FrLocal, s: FrLocal) -> Proof<G1Local, G2Local> {
        let w = frs(weights);
        let mut bytes = [0u8; 259];
        unsafe { check(self.ctx.0, zk_prove(self.ctx.0, self.crs, self.qap, w.as_ptr(), weights.len(),
                                            fr_to_words(&r).as_ptr(), fr_to_words(&s).as_ptr(), bytes.as_mut_ptr())); }
        proof_from_bytes(&bytes)
    }
    pub fn prove(&self, weights: &[FrLocal]) -> Proof<G1Local, G2Local> {
        self.prove_with_rs(weights, FrLocal::random_elem(), FrLocal::random_elem())
    }
    /// What the reference lacks: (number of gates with U_j V_j != W_j, the lowest such gate, weights[0] == 1), decided on the GPU
    /// (zk_qap_check) before a proof is spent on the witness.  Sparse forms only (from_root_rep*): the dense form of
    /// GpuProver::new holds coefficients, not its roots, and panics with the library's "unsupported" text.
    pub fn check_witness(&self, weights: &[FrLocal]) -> (usize, Option<usize>, bool) {
        let w = frs(weights);
        let mut res = ZkQapCheckResult { bad_gates: 0, first_bad: ZK_QAP_CHECK_NONE, flags: 0 };
        unsafe { check(self.ctx.0, zk_qap_check(self.ctx.0, self.qap, w.as_ptr(), weights.len(), &mut res)); }
        (res.bad_gates as usize, if res.first_bad == ZK_QAP_CHECK_NONE { None } else { Some(res.first_bad as usize) },
         res.flags & ZK_QAP_CHECK_WIRE0 == 0)
    }
    /// true iff prove(weights) yields a proof that verify accepts: every gate holds and the constant wire is 1
    pub fn is_satisfied(&self, weights: &[FrLocal]) -> bool {
        let (bad, _, wire0_ok) = self.check_witness(weights);
        bad == 0 && wire0_ok
    }
    /// What the reference lacks as well: is the CRS this prover holds (set up here, uploaded, or read from a file) a Groth16 CRS of
    /// SOME trapdoor for its QAP?  (zk_crs_check: the relations and their bits are in include/zkgpu.h.)  The challenge is drawn from
    /// the OS inside the library -- whoever made the CRS must not be able to predict it.  -> (failed bits, flags); good means
    /// failed == 0 and flags & ZK_CRS_CHECK_T_ZERO == 0, which is what `crs_is_good` returns.
    pub fn check_crs(&self) -> (u32, u32) {
        let mut res = ZkCrsCheckResult { failed: 0, flags: 0 };
        unsafe { check(self.ctx.0, zk_crs_check(self.ctx.0, self.crs, self.qap, std::ptr::null(), &mut res)); }
        (res.failed, res.flags)
    }
    pub fn crs_is_good(&self) -> bool {
        let (failed, flags) = self.check_crs();
        failed == 0 && flags & ZK_CRS_CHECK_T_ZERO == 0
    }
    /// The head of a trustless setup (zk_crs_from_powers): the prover's CRS becomes the one setup would have made for (alpha, beta, 1,
    /// 1, x) with the (alpha, beta, x) of a powers-of-tau transcript that nobody has to know -- derived by group operations only, for
    /// a prover built by from_root_rep (roots of unity) or from_root_rep_integers; the other forms panic with the library's
    /// "unsupported" text.  The transcript is NOT checked to be a sequence of powers: the derived CRS goes through check_crs before it
    /// replaces the old one, and a transcript that fails it panics.  Then one `contribute` per party.  Returns the new CRS in the
    /// reference's types, to be published.
    pub fn from_powers(&mut self, powers: &PowersOfTau) -> (SigmaG1<G1Local>, SigmaG2<G2Local>) {
        let n_rest = powers.tau_g2.len() / 16;
        assert!(powers.tau_g1.len() % 8 == 0 && powers.tau_g2.len() % 16 == 0, "a G1 point is 8 words, a G2 point 16");
        assert!(powers.alpha_tau_g1.len() == 8 * n_rest && powers.beta_tau_g1.len() == 8 * n_rest, "tau_g2, alpha_tau_g1, beta_tau_g1 differ in length");
        let desc = ZkPowersDesc { n_tau_g1: powers.tau_g1.len() / 8, n_rest, tau_g1: powers.tau_g1.as_ptr(), tau_g2: powers.tau_g2.as_ptr(),
                                  alpha_tau_g1: powers.alpha_tau_g1.as_ptr(), beta_tau_g1: powers.beta_tau_g1.as_ptr(), beta_g2: powers.beta_g2.as_ptr() };
        let mut next: *mut ZkCrs = std::ptr::null_mut();
        let mut res = ZkCrsCheckResult { failed: 0, flags: 0 };
        unsafe {
            check(self.ctx.0, zk_crs_from_powers(self.ctx.0, self.qap, &desc, &mut next));
            check(self.ctx.0, zk_crs_check(self.ctx.0, next, self.qap, std::ptr::null(), &mut res));
            assert!(res.failed == 0 && res.flags & ZK_CRS_CHECK_T_ZERO == 0, "the transcript is no powers-of-tau sequence: zk_crs_check {:#x}", res.failed);
            zk_crs_free(self.crs);
        }
        self.crs = next;
        download_crs(&self.ctx, self.crs, self.n, self.m, self.input)
    }
    /// Re-keys delta (zk_crs_contribute): the prover's CRS becomes the one setup would have made for (alpha, beta, gamma, delta d, x)
    /// with a factor d drawn from the OS inside the library, wiped and never returned -- after which whoever made the old CRS no
    /// longer knows this one's trapdoor.  Returns the record (a proof of knowledge of d bound to `tag`, the hash of the transcript so
    /// far) and the new CRS in the reference's types, to be published.  The old CRS is checked against the new one before it is
    /// dropped (check_contribution's relations); a failure there is a bug and panics.
    pub fn contribute(&mut self, tag: &[u8; 32]) -> (ZkCrsContribution, (SigmaG1<G1Local>, SigmaG2<G2Local>)) {
        let mut rec = ZkCrsContribution([0u8; 224]);
        let mut next: *mut ZkCrs = std::ptr::null_mut();
        let mut res = ZkCrsContributionResult { failed: 0, flags: 0 };
        unsafe {
            check(self.ctx.0, zk_crs_contribute(self.ctx.0, self.crs, std::ptr::null(), tag.as_ptr(), &mut next, &mut rec));
            check(self.ctx.0, zk_crs_contribution_check(self.ctx.0, self.crs, next, &rec, tag.as_ptr(), std::ptr::null(), &mut res));
            assert!(res.failed == 0, "zk_crs_contribute made a CRS its own check refuses: {:#x}", res.failed);
            zk_crs_free(self.crs);
        }
        self.crs = next;
        (rec, download_crs(&self.ctx, self.crs, self.n, self.m, self.input))
    }
    /// Is the CRS this prover holds `before` with only delta re-keyed, by whoever made `record` for `tag`?  (zk_crs_contribution_check:
    /// the relations and their ZK_CONTRIB_* bits are in include/zkgpu.h.)  -> the failed bits, 0 = a valid successor; the prover's
    /// CRS is then as good as `before` is (check_crs, once, for the first CRS of a chain).
    pub fn check_contribution(&self, before: (&SigmaG1<G1Local>, &SigmaG2<G2Local>), record: &ZkCrsContribution, tag: &[u8; 32]) -> u32 {
        let (old, n, m, l) = upload_crs(&self.ctx, before.0, before.1);
        assert!(n == self.n && m == self.m && l == self.input, "CRS dimensions differ");
        let mut res = ZkCrsContributionResult { failed: 0, flags: 0 };
        unsafe {
            check(self.ctx.0, zk_crs_contribution_check(self.ctx.0, old, self.crs, record, tag.as_ptr(), std::ptr::null(), &mut res));
            zk_crs_free(old);
        }
        res.failed
    }
    /// the same for `count` witnesses resident on the device, m elements each, `stride` elements apart (zk_witgen_run's layout: stride == m)
    pub fn check_witnesses_dev(&self, d_weights: *const c_void, m: usize, stride: usize, count: usize) -> Vec<ZkQapCheckResult> {
        let mut out: Vec<ZkQapCheckResult> = (0..count).map(|_| ZkQapCheckResult { bad_gates: 0, first_bad: ZK_QAP_CHECK_NONE, flags: 0 }).collect();
        unsafe { check(self.ctx.0, zk_qap_check_dev(self.ctx.0, self.qap, d_weights, m, stride, count, out.as_mut_ptr())); }
        out
    }
    /// groth16::verify against the device CRS
    pub fn verify(&self, inputs: &[FrLocal], proof: &Proof<G1Local, G2Local>) -> bool {
        let (x, bytes, mut ok) = (frs(inputs), proof_to_bytes(proof), 0 as c_int);
        unsafe { check(self.ctx.0, zk_verify(self.ctx.0, self.crs, x.as_ptr(), inputs.len(), bytes.as_ptr(), &mut ok)); }
        ok == 1
    }
    /// verify for many proofs on the GPU (zk_verify_batch): entry j == verify(&inputs[j], &proofs[j]); every row has the same length
    pub fn verify_batch(&self, inputs: &[Vec<FrLocal>], proofs: &[Proof<G1Local, G2Local>]) -> Vec<bool> {
        assert!(inputs.len() == proofs.len(), "one input row per proof");
        let k = inputs.first().map_or(0, |r| r.len());
        assert!(inputs.iter().all(|r| r.len() == k), "every proof needs the same number of inputs");
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|p| proof_to_bytes(p).to_vec()).collect();
        let mut ok = vec![0 as c_int; proofs.len()];
        unsafe { check(self.ctx.0, zk_verify_batch(self.ctx.0, self.crs, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), ok.as_mut_ptr())); }
        ok.into_iter().map(|v| v == 1).collect()
    }
    /// verify_batch over compressed proofs (Proof::to_compressed), decompressed on the GPU (zk_verify_batch_compressed): entry j is
    /// true iff proofs[j] decompresses and verify accepts the result
    pub fn verify_batch_compressed(&self, inputs: &[Vec<FrLocal>], proofs: &[[u8; 128]]) -> Vec<bool> {
        assert!(inputs.len() == proofs.len(), "one input row per proof");
        let k = inputs.first().map_or(0, |r| r.len());
        assert!(inputs.iter().all(|r| r.len() == k), "every proof needs the same number of inputs");
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|p| p.to_vec()).collect();
        let mut ok = vec![0 as c_int; proofs.len()];
        unsafe { check(self.ctx.0, zk_verify_batch_compressed(self.ctx.0, self.crs, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), ok.as_mut_ptr())); }
        ok.into_iter().map(|v| v == 1).collect()
    }
    /// one verdict for many proofs on the GPU (zk_verify_batch_all): true iff every proof decodes and the random linear
    /// combination of their pairing equations holds, with secret multipliers z_j = the low 128 bits of FrLocal::random_elem()
    /// (redrawn when 0); a batch with a bad proof passes with probability at most 1 / (2^128 - 1)
    pub fn verify_batch_all(&self, inputs: &[Vec<FrLocal>], proofs: &[Proof<G1Local, G2Local>]) -> bool {
        assert!(inputs.len() == proofs.len(), "one input row per proof");
        let k = inputs.first().map_or(0, |r| r.len());
        assert!(inputs.iter().all(|r| r.len() == k), "every proof needs the same number of inputs");
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|p| proof_to_bytes(p).to_vec()).collect();
        let z: Vec<u64> = proofs.iter().flat_map(|_| loop {
            let w = fr_to_words(&FrLocal::random_elem());
            if w[0] | w[1] != 0 { break [w[0], w[1]]; }
        }).collect();
        let mut ok: c_int = 0;
        unsafe { check(self.ctx.0, zk_verify_batch_all(self.ctx.0, self.crs, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), z.as_ptr(), &mut ok)); }
        ok == 1
    }
    /// Many proofs over one circuit: the 32 m-byte transfer of witness k+1 overlaps the inner products of proof k
    /// (zk_prove_submit_host / zk_prove_wait with two tickets in flight and page-locked staging buffers).
    pub fn prove_stream<'a, I>(&self, jobs: I) -> Vec<Proof<G1Local, G2Local>>
    where I: IntoIterator<Item = (&'a [FrLocal], FrLocal, FrLocal)> {
        let mut out = Vec::new();
        let mut inflight: std::collections::VecDeque<c_int> = Default::default();
        let mut staging: [*mut c_void; 2] = [std::ptr::null_mut(); 2];
        let mut cap = [0usize; 2];
        let finish = |t: c_int, out: &mut Vec<Proof<G1Local, G2Local>>| {
            let mut bytes = [0u8; 259];
            unsafe { check(self.ctx.0, zk_prove_wait(self.ctx.0, t, bytes.as_mut_ptr())); }
            out.push(proof_from_bytes(&bytes));
        };
        for (k, (weights, r, s)) in jobs.into_iter().enumerate() {
            if inflight.len() == 2 { let t = inflight.pop_front().unwrap(); finish(t, &mut out); }
            let slot = k % 2;            // the buffer of the proof waited for two submissions ago
            let need = weights.len() * 32;
            unsafe {
                if cap[slot] < need {
                    if !staging[slot].is_null() { zk_host_free(staging[slot]); }
                    assert_eq!(zk_host_alloc(need, &mut staging[slot]), 0);
                    cap[slot] = need;
                }
                let dst = std::slice::from_raw_parts_mut(staging[slot] as *mut u64, weights.len() * 4);
                for (i, c) in weights.iter().enumerate() { dst[4 * i..4 * i + 4].copy_from_slice(&fr_to_words(c)); }
                let mut t: c_int = -1;
                check(self.ctx.0, zk_prove_submit_host(self.ctx.0, self.crs, self.qap, staging[slot] as *const u64, weights.len(),
                                                       fr_to_words(&r).as_ptr(), fr_to_words(&s).as_ptr(), &mut t));
                inflight.push_back(t);
            }
        }
        while let Some(t) = inflight.pop_front() { finish(t, &mut out); }
        unsafe { for p in staging.iter() { if !p.is_null() { zk_host_free(*p); } } }
        out
    }
    pub fn dims(&self) -> (usize, usize, usize) { (self.n, self.m, self.input) }
    /// the verifying key of the device CRS (zk_vk_from_crs)
    pub fn verifying_key(&self) -> VerifyingKey { VerifyingKey::from_crs(self) }
}

/// The verifying key (zk_vk): alpha, beta, gamma, delta and sum_gamma[0..l], all groth16::verify reads of (SigmaG1, SigmaG2).  Host
/// data: to_bytes / from_bytes / verify need no GPU.  verify_batch runs on a GpuProver's context; the first call binds the key to it.
pub struct VerifyingKey(*mut ZkVk);
impl VerifyingKey {
    pub fn from_crs(p: &GpuProver) -> Self {
        let mut k = std::ptr::null_mut();
        unsafe { check(p.ctx.0, zk_vk_from_crs(p.ctx.0, p.crs, &mut k)); }
        VerifyingKey(k)
    }
    /// from the reference's own types; panics on a point off its curve or outside G2 (ZK_ERR_RANGE)
    pub fn new(sigma: (&SigmaG1<G1Local>, &SigmaG2<G2Local>)) -> Self {
        let (a1, sg) = (g1_to_words(&sigma.0.alpha), g1s(&sigma.0.sum_gamma));
        let (b2, g2, d2) = (g2_to_words(&sigma.1.beta), g2_to_words(&sigma.1.gamma), g2_to_words(&sigma.1.delta));
        let desc = ZkVkDesc { input: sigma.0.sum_gamma.len() - 1, alpha_g1: a1.as_ptr(),
            beta_g2: b2.as_ptr(), gamma_g2: g2.as_ptr(), delta_g2: d2.as_ptr(), sum_gamma_g1: sg.as_ptr() };
        let mut k = std::ptr::null_mut();
        assert_eq!(unsafe { zk_vk_create(&desc, &mut k) }, 0, "zk_vk_create failed");
        VerifyingKey(k)
    }
    pub fn input(&self) -> usize {
        let mut l = 0usize;
        assert_eq!(unsafe { zk_vk_dims(self.0, &mut l) }, 0);
        l
    }
    /// the ZKVKv1 byte form (include/zkgpu.h)
    pub fn to_bytes(&self) -> Vec<u8> {
        let mut out = vec![0u8; unsafe { zk_vk_bytes(self.input()) }];
        assert_eq!(unsafe { zk_vk_to_bytes(self.0, out.as_mut_ptr(), out.len()) }, 0);
        out
    }
    /// Err(status): ZK_ERR_IO (-8) for a wrong length, magic or checksum, ZK_ERR_RANGE (-6) for a bad point
    pub fn from_bytes(bytes: &[u8]) -> Result<Self, c_int> {
        let mut k = std::ptr::null_mut();
        match unsafe { zk_vk_from_bytes(bytes.as_ptr(), bytes.len(), &mut k) } { 0 => Ok(VerifyingKey(k)), rc => Err(rc) }
    }
    pub fn save(&self, path: &str) -> Result<(), c_int> {
        let p = std::ffi::CString::new(path).unwrap();
        match unsafe { zk_vk_save(self.0, p.as_ptr()) } { 0 => Ok(()), rc => Err(rc) }
    }
    pub fn load(path: &str) -> Result<Self, c_int> {
        let p = std::ffi::CString::new(path).unwrap();
        let mut k = std::ptr::null_mut();
        match unsafe { zk_vk_load(p.as_ptr(), &mut k) } { 0 => Ok(VerifyingKey(k)), rc => Err(rc) }
    }
    /// groth16::verify on the host, no GPU; panics on an input >= r as the reference's FrLocal arithmetic would
    pub fn verify(&self, inputs: &[FrLocal], proof: &Proof<G1Local, G2Local>) -> bool {
        let (x, bytes, mut ok) = (frs(inputs), proof_to_bytes(proof), 0 as c_int);
        assert_eq!(unsafe { zk_vk_verify(self.0, x.as_ptr(), inputs.len(), bytes.as_ptr(), &mut ok) }, 0, "zk_vk_verify failed");
        ok == 1
    }
    /// GpuProver::verify_batch with the key in the place of the CRS (zk_vk_verify_batch), on `p`'s context
    pub fn verify_batch(&self, p: &GpuProver, inputs: &[Vec<FrLocal>], proofs: &[Proof<G1Local, G2Local>]) -> Vec<bool> {
        assert!(inputs.len() == proofs.len(), "one input row per proof");
        let k = inputs.first().map_or(0, |r| r.len());
        assert!(inputs.iter().all(|r| r.len() == k), "every proof needs the same number of inputs");
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|q| proof_to_bytes(q).to_vec()).collect();
        let mut ok = vec![0 as c_int; proofs.len()];
        unsafe { check(p.ctx.0, zk_vk_verify_batch(p.ctx.0, self.0, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), ok.as_mut_ptr())); }
        ok.into_iter().map(|v| v == 1).collect()
    }
    /// the compressed and the one-verdict forms, and the input sums on their own
    pub fn verify_batch_compressed(&self, p: &GpuProver, inputs: &[Vec<FrLocal>], proofs: &[[u8; 128]]) -> Vec<bool> {
        let k = inputs.first().map_or(0, |r| r.len());
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|q| q.to_vec()).collect();
        let mut ok = vec![0 as c_int; proofs.len()];
        unsafe { check(p.ctx.0, zk_vk_verify_batch_compressed(p.ctx.0, self.0, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), ok.as_mut_ptr())); }
        ok.into_iter().map(|v| v == 1).collect()
    }
    pub fn verify_batch_all(&self, p: &GpuProver, inputs: &[Vec<FrLocal>], proofs: &[Proof<G1Local, G2Local>], z: &[[u64; 2]]) -> bool {
        assert!(inputs.len() == proofs.len() && z.len() == proofs.len(), "one input row and one multiplier per proof");
        let k = inputs.first().map_or(0, |r| r.len());
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let bytes: Vec<u8> = proofs.iter().flat_map(|q| proof_to_bytes(q).to_vec()).collect();
        let zw: Vec<u64> = z.iter().flat_map(|v| v.to_vec()).collect();
        let mut ok: c_int = 0;
        unsafe { check(p.ctx.0, zk_vk_verify_batch_all(p.ctx.0, self.0, x.as_ptr(), k, bytes.as_ptr(), proofs.len(), zw.as_ptr(), &mut ok)); }
        ok == 1
    }
    pub fn input_sums(&self, p: &GpuProver, inputs: &[Vec<FrLocal>], tables: bool) -> Vec<G1Local> {
        let k = inputs.first().map_or(0, |r| r.len());
        let x: Vec<u64> = inputs.iter().flat_map(|r| frs(r)).collect();
        let mut out = vec![0u64; 8 * inputs.len()];
        unsafe { check(p.ctx.0, zk_vk_input_sums(p.ctx.0, self.0, x.as_ptr(), k, inputs.len(), tables as c_int, out.as_mut_ptr())); }
        out.chunks(8).map(g1_from_words).collect()
    }
}
impl Drop for VerifyingKey { fn drop(&mut self) { unsafe { zk_vk_free(self.0) } } }   // safe before or after the prover's context goes

impl ZkCrsContribution {
    pub fn to_bytes(&self) -> [u8; 224] { self.0 }
    pub fn from_bytes(b: &[u8; 224]) -> Self { ZkCrsContribution(*b) }
    /// zk_crs_contribution_verify (host code, no GPU): does the record prove knowledge of d with delta_after = d delta_before for `tag`?
    pub fn verify(&self, tag: &[u8; 32]) -> bool {
        let mut ok = 0 as c_int;
        assert_eq!(unsafe { zk_crs_contribution_verify(self, tag.as_ptr(), &mut ok) }, 0, "zk_crs_contribution_verify failed");
        ok == 1
    }
}

impl Drop for GpuProver {
    fn drop(&mut self) { unsafe { zk_crs_free(self.crs); zk_qap_free(self.qap); } }   // self.ctx drops afterwards (field order)
}

// ------------------------------------------------------------------------------------------------
// prove() over all GPUs of a node.  One MultiGpuProver per GPU (a thread or a process each); rank 0 draws the 128-byte id
// with MultiGpuProver::unique_id() and hands it to the others by any channel.  A ROUND is `world` proofs, one per rank:
// every rank pushes its own witness, the library exchanges the scalars of the four inner products so that rank g multiplies
// its own 1/world of the CRS points for every proof of the round (RCCL over xGMI, linked into libzkgpu.so), returns the
// 768-byte partial sums to the proofs' owners and assembles.  Every rank must make the same sequence of calls.
// ------------------------------------------------------------------------------------------------
pub struct MultiGpuProver { inner: GpuProver, comm: *mut ZkComm, mgpu: *mut ZkMgpu, world: usize }

impl MultiGpuProver {
    pub fn unique_id() -> [u8; 128] {
        let mut id = [0u8; 128];
        assert_eq!(unsafe { zk_comm_unique_id(id.as_mut_ptr()) }, 0, "zk_comm_unique_id failed");
        id
    }
    /// `prover`: this rank's device copy of (QAP, CRS) in the roots-of-unity form (GpuProver::from_root_rep, made on the device
    /// `ZKGPU_DEVICE` selects); collective over the `world` ranks.
    pub fn new(prover: GpuProver, id: &[u8; 128], rank: usize, world: usize) -> Self {
        let (mut comm, mut mgpu) = (std::ptr::null_mut(), std::ptr::null_mut());
        unsafe {
            check(prover.ctx.0, zk_comm_init(prover.ctx.0, id.as_ptr(), rank as c_int, world as c_int, &mut comm));
            check(prover.ctx.0, zk_mgpu_create(prover.ctx.0, comm, prover.crs, prover.qap, &mut mgpu));
        }
        MultiGpuProver { inner: prover, comm, mgpu, world }
    }
    fn check(&self, rc: c_int) {
        if rc != 0 {
            panic!("{}", unsafe { std::ffi::CStr::from_ptr(zk_mgpu_last_error(self.mgpu)) }.to_string_lossy());
        }
    }
    /// This rank's share of a stream of rounds: job k is the proof this rank owns in round k.  Witnesses are staged in
    /// page-locked memory, two rounds are pushed ahead of every pop (the schedule the throughput numbers are quoted on).
    pub fn prove_stream<'a, I>(&self, jobs: I) -> Vec<Proof<G1Local, G2Local>>
    where I: IntoIterator<Item = (&'a [FrLocal], FrLocal, FrLocal)> {
        let mut out = Vec::new();
        let mut staging: [*mut c_void; 4] = [std::ptr::null_mut(); 4];   // a round's witness is read before its pop; <= 3 in flight
        let mut cap = [0usize; 4];
        let mut in_flight = 0usize;
        let pop = |out: &mut Vec<Proof<G1Local, G2Local>>| {
            let mut bytes = [0u8; 259];
            self.check(unsafe { zk_mgpu_pop(self.mgpu, bytes.as_mut_ptr()) });
            out.push(proof_from_bytes(&bytes));
        };
        for (k, (weights, r, s)) in jobs.into_iter().enumerate() {
            if in_flight == 3 { pop(&mut out); in_flight -= 1; }
            let slot = k % 4;
            let need = weights.len() * 32;
            unsafe {
                if cap[slot] < need {
                    if !staging[slot].is_null() { zk_host_free(staging[slot]); }
                    assert_eq!(zk_host_alloc(need, &mut staging[slot]), 0);
                    cap[slot] = need;
                }
                let dst = std::slice::from_raw_parts_mut(staging[slot] as *mut u64, weights.len() * 4);
                for (i, c) in weights.iter().enumerate() { dst[4 * i..4 * i + 4].copy_from_slice(&fr_to_words(c)); }
                self.check(zk_mgpu_push_host(self.mgpu, staging[slot] as *const u64, weights.len(),
                                             fr_to_words(&r).as_ptr(), fr_to_words(&s).as_ptr()));
            }
            in_flight += 1;
        }
        while in_flight > 0 { pop(&mut out); in_flight -= 1; }
        unsafe { for p in staging.iter() { if !p.is_null() { zk_host_free(*p); } } }
        out
    }
    /// One proof per rank and call: the reference's prove(), `world` of them at a time.
    pub fn prove(&self, weights: &[FrLocal]) -> Proof<G1Local, G2Local> {
        self.prove_stream(std::iter::once((weights, FrLocal::random_elem(), FrLocal::random_elem()))).pop().unwrap()
    }
    pub fn world(&self) -> usize { self.world }
    /// Bound of every wait for a peer (default 120 s): a pop whose round does not complete in time panics with the library's
    /// message instead of blocking for ever, and the communicator is aborted.
    pub fn set_timeout_ms(&self, ms: u64) { unsafe { zk_comm_set_timeout(self.comm, ms as std::os::raw::c_long); } }
    /// Ranks of the RCCL communicator as RCCL counts them (0 when `world` is 1).
    pub fn rccl_ranks(&self) -> usize { unsafe { zk_comm_rccl_ranks(self.comm) as usize } }
    pub fn single(&self) -> &GpuProver { &self.inner }
}
impl Drop for MultiGpuProver {
    fn drop(&mut self) { unsafe { zk_mgpu_destroy(self.mgpu); zk_comm_destroy(self.comm); } }   // self.inner (ctx, crs, qap) drops afterwards
}

// ------------------------------------------------------------------------------------------------
// The reference's three functions
// ------------------------------------------------------------------------------------------------
/// groth16::setup (mod.rs:134): the trapdoor is drawn here (thread_rng, as mod.rs:139-145), every group element is computed
/// on the GPU and handed back in the reference's types.
pub fn setup(qap: &QAP<CoefficientPoly<FrLocal>>) -> (SigmaG1<G1Local>, SigmaG2<G2Local>) {
    let ctx = Ctx::new();
    let q = upload_dense(&ctx, qap);
    let td: Vec<u64> = (0..5).flat_map(|_| fr_to_words(&FrLocal::random_elem()).to_vec()).collect();
    let mut crs = std::ptr::null_mut();
    unsafe { check(ctx.0, zk_setup(ctx.0, q, td.as_ptr(), &mut crs)); }
    let sigma = download_crs(&ctx, crs, qap.degree, qap.u.len(), qap.input);
    unsafe { zk_crs_free(crs); zk_qap_free(q); }
    sigma
}

thread_local! {
    // the prover of the most recent (qap, sigma) pair of this thread: groth16::prove takes both by reference on every call
    // (mod.rs:213-217), and re-uploading 3 m n coefficients + the CRS per proof would dominate.  Keyed by the addresses
    // AND a fingerprint of the contents, so a freed-and-reallocated object at the same address is not mistaken for the old one.
    static CACHED: RefCell<Option<((usize, usize, usize, [u64; 12]), GpuProver)>> = RefCell::new(None);
}
fn fingerprint(qap: &QAP<CoefficientPoly<FrLocal>>, s1: &SigmaG1<G1Local>) -> [u64; 12] {
    let mut f = [0u64; 12];
    f[0] = qap.u.len() as u64; f[1] = qap.degree as u64; f[2] = qap.input as u64; f[3] = s1.xi.len() as u64;
    if let Some(c) = qap.t.iter().nth(qap.degree / 2) { f[4..8].copy_from_slice(&fr_to_words(c)); }
    f[8..12].copy_from_slice(&g1_to_words(&s1.delta)[0..4]);
    f
}

/// Drop-in for groth16::prove: identical signature (mod.rs:213-217).  The device copies of the QAP and the CRS are kept
/// between calls with the same arguments.
pub fn prove(qap: &QAP<CoefficientPoly<FrLocal>>, sigma: (&SigmaG1<G1Local>, &SigmaG2<G2Local>), weights: &[FrLocal])
    -> Proof<G1Local, G2Local> {
    let key = (qap as *const _ as usize, sigma.0 as *const _ as usize, sigma.1 as *const _ as usize, fingerprint(qap, sigma.0));
    CACHED.with(|c| {
        let mut slot = c.borrow_mut();
        let hit = match *slot { Some((ref k, _)) => *k == key, None => false };
        if !hit { *slot = Some((key, GpuProver::new(qap, sigma))); }
        slot.as_ref().unwrap().1.prove(weights)
    })
}

/// groth16::verify (mod.rs:299-303; `P` is the reference's phantom parameter, call sites write verify::<CoefficientPoly<FrLocal>, ..>)
pub fn verify<P>(sigma: (&SigmaG1<G1Local>, &SigmaG2<G2Local>), inputs: &[FrLocal], proof: &Proof<G1Local, G2Local>) -> bool {
    let ctx = Ctx::new();
    let (crs, _, _, _) = upload_crs(&ctx, sigma.0, sigma.1);
    let (x, bytes, mut ok) = (frs(inputs), proof_to_bytes(proof), 0 as c_int);
    unsafe {
        check(ctx.0, zk_verify(ctx.0, crs, x.as_ptr(), inputs.len(), bytes.as_ptr(), &mut ok));
        zk_crs_free(crs);
    }
    ok == 1
}

// ------------------------------------------------------------------------------------------------
// The gate-level builder and bit-sliced witnesses.  Like the rest of this file written without a toolchain: the extern block above
// is held against include/zkgpu.h by tests/test_abi.py, the wrappers below have never been compiled.  The crate's own
// circuit::builder::Circuit<T> keeps its place for CPU evaluation; this one produces what the GPU prover takes.
// ------------------------------------------------------------------------------------------------
pub type WireId = u32;                       // 0 = the constant zero, 1 = the constant one (builder/mod.rs:91-114)
#[derive(Clone, Copy)]
pub enum Gate { BitChecker = 0, Not = 1, And = 2, Or = 3, Xor = 4, Nand = 5, Nor = 6, Xnor = 7, LessThan = 8, GreaterThan = 9 }
#[derive(Clone, Copy)]
pub enum Comparator { IsEqual = 0, IsEqualZero = 1, LessThan = 2, LessThanEq = 3, GreaterThan = 4, GreaterThanEq = 5 }

pub struct GpuCircuitBuilder(*mut ZkBuilder);
/// what zk_builder_finish returns: rows, witness order and both tapes (an ordinary zk_circuit)
pub struct BuiltCircuit(*mut ZkCircuit);
impl Drop for GpuCircuitBuilder { fn drop(&mut self) { unsafe { zk_builder_free(self.0) } } }
impl Drop for BuiltCircuit { fn drop(&mut self) { unsafe { zk_circuit_free(self.0) } } }

impl GpuCircuitBuilder {
    pub fn new() -> Self {
        let mut b: *mut ZkBuilder = std::ptr::null_mut();
        assert_eq!(unsafe { zk_builder_create(&mut b) }, 0);
        GpuCircuitBuilder(b)
    }
    fn ok(&self, rc: c_int) {
        // the reference's builder panics (expect / assert!) where this one refuses
        if rc != 0 { panic!("{}", unsafe { std::ffi::CStr::from_ptr(zk_builder_last_error(self.0)) }.to_string_lossy()) }
    }
    pub fn zero_wire(&self) -> WireId { 0 }
    pub fn unity_wire(&self) -> WireId { 1 }
    fn new_wires(&mut self, kind: c_int, count: usize) -> Vec<WireId> {
        let mut out = vec![0u32; count];
        self.ok(unsafe { zk_builder_new_wires(self.0, kind, count, out.as_mut_ptr()) });
        out
    }
    pub fn new_wire(&mut self) -> WireId { self.new_wires(1, 1)[0] }          // any field element: the circuit is not boolean
    pub fn new_word8(&mut self) -> Vec<WireId> { self.new_wires(0, 8) }       // least significant bit first
    pub fn new_word64(&mut self) -> Vec<WireId> { self.new_wires(0, 64) }
    pub fn const_word8(&self, x: u8) -> Vec<WireId> { (0..8).map(|i| ((x >> i) & 1) as u32).collect() }
    pub fn const_word64(&self, x: u64) -> Vec<WireId> { (0..64).map(|i| ((x >> i) & 1) as u32).collect() }
    pub fn new_sub_circuit(&mut self, lhs: &[(FrLocal, WireId)], rhs: &[(FrLocal, WireId)]) -> WireId {
        let (lw, rw): (Vec<FrLocal>, Vec<FrLocal>) = (lhs.iter().map(|t| t.0).collect(), rhs.iter().map(|t| t.0).collect());
        let (li, ri): (Vec<u32>, Vec<u32>) = (lhs.iter().map(|t| t.1).collect(), rhs.iter().map(|t| t.1).collect());
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_sub_circuit(self.0, frs(&lw).as_ptr(), li.as_ptr(), li.len(), frs(&rw).as_ptr(), ri.as_ptr(), ri.len(), &mut out) });
        out
    }
    pub fn gate(&mut self, g: Gate, x: WireId, y: WireId) -> WireId {
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_gate(self.0, g as c_int, x, y, &mut out) });
        out
    }
    pub fn new_not(&mut self, x: WireId) -> WireId { self.gate(Gate::Not, x, 0) }
    pub fn new_and(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::And, x, y) }
    pub fn new_or(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::Or, x, y) }
    pub fn new_xor(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::Xor, x, y) }
    pub fn new_nand(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::Nand, x, y) }
    pub fn new_nor(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::Nor, x, y) }
    pub fn new_xnor(&mut self, x: WireId, y: WireId) -> WireId { self.gate(Gate::Xnor, x, y) }
    pub fn assert_bit(&mut self, w: WireId) { self.ok(unsafe { zk_builder_assert_bit(self.0, w) }) }
    /// the packed wire sum 2^i bits[i] over 1..253 wires, least significant first: one sub-circuit, a field element (not in the reference)
    pub fn pack(&mut self, bits: &[WireId]) -> WireId {
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_pack(self.0, bits.as_ptr(), bits.len(), &mut out) });
        out
    }
    /// Poseidon of 1, 2 or 4 wires: 217 / 244 / 301 general sub-circuits over linear forms; the output is a field element
    pub fn poseidon(&mut self, inputs: &[WireId]) -> WireId {
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_poseidon(self.0, inputs.as_ptr(), inputs.len(), &mut out) });
        out
    }
    /// the root of the Merkle path leaf, siblings[k], dirs[k] (1: the right child at level k): 246 gates a level
    pub fn merkle_root(&mut self, leaf: WireId, siblings: &[WireId], dirs: &[WireId]) -> WireId {
        assert!(siblings.len() == dirs.len());
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_merkle_root(self.0, leaf, siblings.as_ptr(), dirs.as_ptr(), dirs.len(), &mut out) });
        out
    }
    /// Baby Jubjub: a point is three wires [X, Y, Z], projective; an affine point is [x, y, 1].  The curve equation on (x, y): 4 gates
    pub fn babyjub_assert_on_curve(&mut self, xy: [WireId; 2]) { self.ok(unsafe { zk_builder_babyjub_assert_on_curve(self.0, xy.as_ptr()) }) }
    /// p + q for all pairs of curve points: 11 gates, 10 when q[2] is the unity wire; the operands are not asserted on the curve
    pub fn babyjub_add(&mut self, p: [WireId; 3], q: [WireId; 3]) -> [WireId; 3] {
        let mut out = [0u32; 3];
        self.ok(unsafe { zk_builder_babyjub_add(self.0, p.as_ptr(), q.as_ptr(), out.as_mut_ptr()) });
        out
    }
    /// [sum 2^i bits[i]] Base8 over 1..256 bit wires, each asserted: 1414 gates for 251 bits
    pub fn babyjub_mul_fixed(&mut self, bits: &[WireId]) -> [WireId; 3] {
        let mut out = [0u32; 3];
        self.ok(unsafe { zk_builder_babyjub_mul_fixed(self.0, bits.as_ptr(), bits.len(), out.as_mut_ptr()) });
        out
    }
    /// [sum 2^i bits[i]] P for the affine wires p_xy, asserted on the curve: 4 + n + 2 + 19 (n - 1) gates
    pub fn babyjub_mul(&mut self, p_xy: [WireId; 2], bits: &[WireId]) -> [WireId; 3] {
        let mut out = [0u32; 3];
        self.ok(unsafe { zk_builder_babyjub_mul(self.0, p_xy.as_ptr(), bits.as_ptr(), bits.len(), out.as_mut_ptr()) });
        out
    }
    /// pins the existing wires xy as the affine form of p: 4 gates
    pub fn babyjub_affine(&mut self, p: [WireId; 3], xy: [WireId; 2]) { self.ok(unsafe { zk_builder_babyjub_affine(self.0, p.as_ptr(), xy.as_ptr()) }) }
    /// EdDSA-Poseidon: [S] Base8 = R8 + [8] ([hm] A), hm = H6(R8, A, M), over the affine wires of A and R8, the message wire, the 251 bit
    /// wires of S and the 254 bit wires of hm, which the caller supplies (eddsa_verify_batch writes them): 73384 gates
    pub fn eddsa_verify(&mut self, a_xy: [WireId; 2], r8_xy: [WireId; 2], msg: WireId, s_bits: &[WireId; 251], hm_bits: &[WireId; 254]) {
        self.ok(unsafe { zk_builder_eddsa_verify(self.0, a_xy.as_ptr(), r8_xy.as_ptr(), msg, s_bits.as_ptr(), hm_bits.as_ptr()) })
    }
    pub fn fan_in(&mut self, inputs: &[WireId], g: Gate) -> WireId {
        let mut out = 0u32;
        self.ok(unsafe { zk_builder_fan_in(self.0, g as c_int, inputs.as_ptr(), inputs.len(), &mut out) });
        out
    }
    /// u8_bitwise_op / u64_bitwise_op / bitwise_op: element-wise over two arrays of one length
    pub fn bitwise_op(&mut self, left: &[WireId], right: &[WireId], g: Gate) -> Vec<WireId> {
        assert!(left.len() == right.len());
        let mut out = vec![0u32; left.len()];
        self.ok(unsafe { zk_builder_bitwise(self.0, g as c_int, left.as_ptr(), right.as_ptr(), left.len(), out.as_mut_ptr()) });
        out
    }
    /// is_equal .. greater_than_eq (mod.rs:995-1241); IsEqualZero ignores `right`
    pub fn compare(&mut self, kind: Comparator, left: &[WireId], right: &[WireId]) -> WireId {
        let mut out = 0u32;
        let r = if let Comparator::IsEqualZero = kind { std::ptr::null() } else { assert!(left.len() == right.len()); right.as_ptr() };
        self.ok(unsafe { zk_builder_compare(self.0, kind as c_int, left.as_ptr(), r, left.len(), &mut out) });
        out
    }
    /// the sponge in general form; `input` holds 8 wires per byte
    pub fn keccak(&mut self, input: &[WireId], rate: u32, delim: u8, rounds: u32, out_bytes: usize) -> Vec<WireId> {
        assert!(input.len() % 8 == 0);
        let mut out = vec![0u32; 8 * out_bytes];
        self.ok(unsafe { zk_builder_keccak(self.0, input.as_ptr(), input.len() / 8, rate as c_uint, delim as c_uint, rounds as c_uint, out.as_mut_ptr(), out_bytes) });
        out
    }
    pub fn keccak256(&mut self, input: &[WireId]) -> Vec<WireId> { self.keccak(input, 136, 0x01, 24, 32) }
    pub fn keccak256_stream(&mut self, input: &[WireId]) -> Vec<WireId> { self.keccak256(input) }
    /// ValidateOrder (mod.rs:1459-1476): (is_x_within_range, is_y_greater_than_c, hash_x_y)
    pub fn validate_order(&mut self, x: &[WireId], range: (&[WireId], &[WireId]), y: &[WireId], c: &[WireId]) -> (WireId, WireId, Vec<WireId>) {
        let x_geq = self.compare(Comparator::GreaterThanEq, x, range.0);
        let x_leq = self.compare(Comparator::LessThanEq, x, range.1);
        let in_range = self.new_and(x_geq, x_leq);
        let y_geq = self.compare(Comparator::GreaterThanEq, y, c);
        let stream: Vec<WireId> = x.iter().chain(y.iter()).cloned().collect();
        (in_range, y_geq, self.keccak256_stream(&stream))
    }
    pub fn finish(&mut self, verify: &[WireId]) -> BuiltCircuit {
        let mut c: *mut ZkCircuit = std::ptr::null_mut();
        self.ok(unsafe { zk_builder_finish(self.0, verify.as_ptr(), verify.len(), &mut c) });
        BuiltCircuit(c)
    }
}

impl BuiltCircuit {
    pub fn is_boolean(&self) -> bool { unsafe { zk_circuit_is_boolean(self.0) == 1 } }
    pub fn packed_wires(&self) -> usize {
        let mut n = 0usize;
        unsafe { zk_circuit_packed_wires(self.0, &mut n) };
        n
    }
    pub fn wire_index(&self, wire: WireId) -> Option<usize> {
        let mut i = 0usize;
        if unsafe { zk_circuit_wire_index(self.0, wire, &mut i) } == 0 { Some(i) } else { None }
    }
    /// (m, n, input, n_in)
    pub fn dims(&self) -> (usize, usize, usize, usize) {
        let (mut m, mut n, mut l, mut k) = (0usize, 0usize, 0usize, 0usize);
        unsafe { zk_circuit_dims(self.0, &mut m, &mut n, &mut l, &mut k) };
        (m, n, l, k)
    }
    /// the split into a boolean core and a field tail (zk_circuit_mixed_dims)
    pub fn mixed_dims(&self) -> MixedDims {
        let mut d = MixedDims::default();
        unsafe {
            zk_circuit_mixed_dims(self.0, &mut d.n_bit_inputs, &mut d.n_field_inputs, &mut d.core_ops, &mut d.core_levels, &mut d.tail_ops,
                                  &mut d.tail_levels, &mut d.tail_slots)
        };
        d
    }
    /// one witness through the split on the host (zk_circuit_weights_mixed): packed bit inputs, field inputs of 4 canonical words each
    /// -> m x 4 words, or the status (ZK_ERR_RANGE for a field input >= r)
    pub fn weights_mixed(&self, in_bits: &[u8], in_fields: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, c_int> {
        let m = self.dims().0;
        let mut out = vec![[0u64; 4]; m];
        let rc = unsafe {
            zk_circuit_weights_mixed(self.0, in_bits.as_ptr(), in_bits.len(), in_fields.as_ptr() as *const u64, in_fields.len(),
                                     out.as_mut_ptr() as *mut u64, m)
        };
        if rc == 0 { Ok(out) } else { Err(rc) }
    }
    /// the rows at the roots of unity (zk_circuit_qap_sparse_unity); free with zk_qap_free
    pub fn qap_sparse_unity(&self, ctx: *mut ZkCtx) -> *mut ZkQap {
        let mut q: *mut ZkQap = std::ptr::null_mut();
        unsafe { check(ctx, zk_circuit_qap_sparse_unity(ctx, self.0, &mut q)) };
        q
    }
}

/// zk_boolgen_*: witnesses of a boolean built circuit for `count` packed input rows, left in device memory where the batched prover
/// takes them (d_weights_out + j * m * 32 bytes is witness j)
pub struct Boolgen { ctx: *mut ZkCtx, g: *mut ZkBoolgen, m: usize }
impl Drop for Boolgen { fn drop(&mut self) { unsafe { zk_boolgen_free(self.g) } } }
impl Boolgen {
    pub fn new(ctx: *mut ZkCtx, circuit: &BuiltCircuit) -> Self {
        let mut g: *mut ZkBoolgen = std::ptr::null_mut();
        unsafe { check(ctx, zk_boolgen_create(ctx, circuit.0, &mut g)) };
        Boolgen { ctx, g, m: circuit.dims().0 }
    }
    pub fn run(&self, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, d_weights_out: *mut c_void) {
        unsafe { check(self.ctx, zk_boolgen_run(self.g, d_in_bits, in_stride_bytes, count, d_weights_out, self.m)) }
    }
    pub fn eval(&self, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, wires: &[u32], d_out_bits: *mut c_void, out_stride_bytes: usize) {
        unsafe { check(self.ctx, zk_boolgen_eval(self.g, d_in_bits, in_stride_bytes, count, wires.as_ptr(), wires.len(), d_out_bits, out_stride_bytes)) }
    }
    /// bit and packed wires alike as 4 canonical words each: with wires = 1..l the `inputs` of zk_verify_batch
    pub fn eval_fields(&self, d_in_bits: *const c_void, in_stride_bytes: usize, count: usize, wires: &[u32], d_out_words: *mut c_void) {
        unsafe { check(self.ctx, zk_boolgen_eval_fields(self.g, d_in_bits, in_stride_bytes, count, wires.as_ptr(), wires.len(), d_out_words)) }
    }
}

/// what zk_circuit_mixed_dims reports
#[derive(Default, Debug, Clone, Copy, PartialEq, Eq)]
pub struct MixedDims {
    pub n_bit_inputs: usize, pub n_field_inputs: usize, pub core_ops: usize, pub core_levels: usize,
    pub tail_ops: usize, pub tail_levels: usize, pub tail_slots: usize,
}

/// zk_mixgen_*: witnesses of ANY built circuit -- the boolean core bit-sliced, the field tail one instance per lane -- for `count`
/// input sets (packed bit rows and field inputs of 4 canonical words each), left in device memory in zk_witgen_run's layout
pub struct Mixgen { ctx: *mut ZkCtx, g: *mut ZkMixgen, m: usize }
impl Drop for Mixgen { fn drop(&mut self) { unsafe { zk_mixgen_free(self.g) } } }
impl Mixgen {
    pub fn new(ctx: *mut ZkCtx, circuit: &BuiltCircuit) -> Self {
        let mut g: *mut ZkMixgen = std::ptr::null_mut();
        unsafe { check(ctx, zk_mixgen_create(ctx, circuit.0, &mut g)) };
        Mixgen { ctx, g, m: circuit.dims().0 }
    }
    pub fn run(&self, d_in_bits: *const c_void, in_stride_bytes: usize, d_in_fields: *const c_void, count: usize, d_weights_out: *mut c_void) {
        unsafe { check(self.ctx, zk_mixgen_run(self.g, d_in_bits, in_stride_bytes, d_in_fields, count, d_weights_out, self.m)) }
    }
    /// wires of either class as 4 canonical words each: with wires = 1..l the `inputs` of zk_verify_batch
    pub fn eval_fields(&self, d_in_bits: *const c_void, in_stride_bytes: usize, d_in_fields: *const c_void, count: usize, wires: &[u32],
                       d_out_words: *mut c_void) {
        unsafe {
            check(self.ctx, zk_mixgen_eval_fields(self.g, d_in_bits, in_stride_bytes, d_in_fields, count, wires.as_ptr(), wires.len(), d_out_words))
        }
    }
}

/// zk_poseidon_hash: Poseidon of 1, 2 or 4 elements on the host; None for another arity or an input >= r
pub fn poseidon_hash(inputs: &[[u64; 4]]) -> Option<[u64; 4]> {
    let mut out = [0u64; 4];
    if unsafe { zk_poseidon_hash(inputs.as_ptr() as *const u64, inputs.len(), out.as_mut_ptr()) } == 0 { Some(out) } else { None }
}
/// zk_poseidon_hash_batch: `count` hashes of `arity` elements each, device to device
pub fn poseidon_hash_batch(ctx: *mut ZkCtx, d_inputs: *const c_void, arity: usize, count: usize, d_out: *mut c_void) {
    unsafe { check(ctx, zk_poseidon_hash_batch(ctx, d_inputs, arity, count, d_out)) }
}

/// Baby Jubjub over Fr: a point is [x words | y words], 8 canonical words.  None: a coordinate >= r or a point off the curve
pub fn babyjub_on_curve(p: &[u64; 8]) -> Option<bool> {
    match unsafe { zk_babyjub_on_curve(p.as_ptr()) } { 1 => Some(true), 0 => Some(false), _ => None }
}
pub fn babyjub_add(p: &[u64; 8], q: &[u64; 8]) -> Option<[u64; 8]> {
    let mut out = [0u64; 8];
    if unsafe { zk_babyjub_add(p.as_ptr(), q.as_ptr(), out.as_mut_ptr()) } == 0 { Some(out) } else { None }
}
/// [scalar] p, the scalar an integer of 256 bits that is not reduced; p None: Base8
pub fn babyjub_mul(scalar: &[u64; 4], p: Option<&[u64; 8]>) -> Option<[u64; 8]> {
    let mut out = [0u64; 8];
    let pp = p.map_or(std::ptr::null(), |x| x.as_ptr());
    if unsafe { zk_babyjub_mul(scalar.as_ptr(), pp, out.as_mut_ptr()) } == 0 { Some(out) } else { None }
}
/// (a, d, order of Base8, Base8, Generator)
pub fn babyjub_params() -> ([u64; 4], [u64; 4], [u64; 4], [u64; 8], [u64; 8]) {
    let (mut a, mut d, mut l, mut b, mut g) = ([0u64; 4], [0u64; 4], [0u64; 4], [0u64; 8], [0u64; 8]);
    unsafe { zk_babyjub_params(a.as_mut_ptr(), d.as_mut_ptr(), l.as_mut_ptr(), b.as_mut_ptr(), g.as_mut_ptr()) };
    (a, d, l, b, g)
}
/// zk_babyjub_mul_batch: `count` scalar multiplications, device to device; d_points null: Base8; out_stride_words 0: packed
pub fn babyjub_mul_batch(ctx: *mut ZkCtx, d_scalars: *const c_void, d_points: *const c_void, count: usize, d_out: *mut c_void, out_stride_words: usize) {
    unsafe { check(ctx, zk_babyjub_mul_batch(ctx, d_scalars, d_points, count, d_out, out_stride_words)) }
}

/// EdDSA-Poseidon on Baby Jubjub (include/zkgpu.h states the scheme).  The status of one signature, the lowest that applies
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum EddsaStatus { Valid = 0, Range = 1, KeyOffCurve = 2, ROffCurve = 3, SRange = 4, Mismatch = 5 }
/// H6(R8.x, R8.y, A.x, A.y, M) for any five field elements, no curve check.  None: an element >= r
pub fn eddsa_challenge(r8: &[u64; 8], a: &[u64; 8], msg: &[u64; 4]) -> Option<[u64; 4]> {
    let mut out = [0u64; 4];
    if unsafe { zk_eddsa_challenge(r8.as_ptr(), a.as_ptr(), msg.as_ptr(), out.as_mut_ptr()) } == 0 { Some(out) } else { None }
}
/// [k] Base8.  None: k == 0 or k >= l
pub fn eddsa_public_key(k: &[u64; 4]) -> Option<[u64; 8]> {
    let mut out = [0u64; 8];
    if unsafe { zk_eddsa_public_key(k.as_ptr(), out.as_mut_ptr()) } == 0 { Some(out) } else { None }
}
/// (R8, S), deterministic.  None: k == 0, k >= l, nonce_key >= r or msg >= r
pub fn eddsa_sign(k: &[u64; 4], nonce_key: &[u64; 4], msg: &[u64; 4]) -> Option<([u64; 8], [u64; 4])> {
    let (mut r8, mut s) = ([0u64; 8], [0u64; 4]);
    if unsafe { zk_eddsa_sign(k.as_ptr(), nonce_key.as_ptr(), msg.as_ptr(), r8.as_mut_ptr(), s.as_mut_ptr()) } == 0 { Some((r8, s)) } else { None }
}
/// a malformed signature is a verdict, not an error
pub fn eddsa_verify(a: &[u64; 8], msg: &[u64; 4], r8: &[u64; 8], s: &[u64; 4]) -> EddsaStatus {
    let mut status: c_int = 5;
    unsafe { zk_eddsa_verify(a.as_ptr(), msg.as_ptr(), r8.as_ptr(), s.as_ptr(), &mut status) };
    match status { 0 => EddsaStatus::Valid, 1 => EddsaStatus::Range, 2 => EddsaStatus::KeyOffCurve, 3 => EddsaStatus::ROffCurve, 4 => EddsaStatus::SRange,
                   _ => EddsaStatus::Mismatch }
}
/// zk_eddsa_verify_batch: `count` verdicts, device to device; d_points_msg: count x 20 words (A.x, A.y, R8.x, R8.y, M), d_s: count x 4,
/// d_status: count x u32; d_bits_out null, or rows of bits_stride_bytes (>= 64, a multiple of 8) with the bits of S and of hm
pub fn eddsa_verify_batch(ctx: *mut ZkCtx, d_points_msg: *const c_void, d_s: *const c_void, count: usize, d_status: *mut c_void,
                          d_bits_out: *mut c_void, bits_stride_bytes: usize) {
    unsafe { check(ctx, zk_eddsa_verify_batch(ctx, d_points_msg, d_s, count, d_status, d_bits_out, bits_stride_bytes)) }
}
/// zk_eddsa_sign_batch: `count` signatures, device to device; d_keys, d_nonce_keys, d_msgs: count x 4 words (0 < k < l, n < r, M < r);
/// d_points_msg_out: count x 20 words (A.x, A.y, R8.x, R8.y, M) with A = [k] Base8 computed in the call, d_s_out: count x 4; d_bits_out
/// null, or the rows eddsa_verify_batch writes.  An input out of range refuses the call before anything is written
pub fn eddsa_sign_batch(ctx: *mut ZkCtx, d_keys: *const c_void, d_nonce_keys: *const c_void, d_msgs: *const c_void, count: usize,
                        d_points_msg_out: *mut c_void, d_s_out: *mut c_void, d_bits_out: *mut c_void, bits_stride_bytes: usize) {
    unsafe { check(ctx, zk_eddsa_sign_batch(ctx, d_keys, d_nonce_keys, d_msgs, count, d_points_msg_out, d_s_out, d_bits_out, bits_stride_bytes)) }
}

/// zk_poseidon_tree_*: a binary Merkle tree over Poseidon of arity 2 that stays on the device; paths() writes leaf | siblings and the
/// direction bits in the layout Mixgen::run reads as d_in_fields and d_in_bits
pub struct PoseidonTree { ctx: *mut ZkCtx, t: *mut ZkPoseidonTree }
impl Drop for PoseidonTree { fn drop(&mut self) { unsafe { zk_poseidon_tree_free(self.t) } } }
impl PoseidonTree {
    pub fn build(ctx: *mut ZkCtx, d_leaves: *const c_void, n_leaves: usize, depth: u32) -> Self {
        let mut t: *mut ZkPoseidonTree = std::ptr::null_mut();
        unsafe { check(ctx, zk_poseidon_tree_build(ctx, d_leaves, n_leaves, depth as c_uint, &mut t)) };
        PoseidonTree { ctx, t }
    }
    pub fn root(&self) -> [u64; 4] {
        let mut out = [0u64; 4];
        unsafe { check(self.ctx, zk_poseidon_tree_root(self.t, out.as_mut_ptr())) };
        out
    }
    /// (n_leaves, depth)
    pub fn dims(&self) -> (usize, u32) {
        let (mut n, mut d) = (0usize, 0 as c_uint);
        unsafe { check(self.ctx, zk_poseidon_tree_dims(self.t, &mut n, &mut d)) };
        (n, d as u32)
    }
    pub fn nodes(&self, level: u32) -> Vec<[u64; 4]> {
        let (n, _) = self.dims();
        let size = if level == 0 { n } else { std::cmp::max(1, (n + (1usize << level) - 1) >> level) };
        let mut out = vec![[0u64; 4]; size];
        unsafe { check(self.ctx, zk_poseidon_tree_nodes(self.t, level as c_uint, out.as_mut_ptr() as *mut u64)) };
        out
    }
    pub fn paths(&self, d_indices: *const c_void, count: usize, d_fields_out: *mut c_void, field_stride_words: usize, d_bits_out: *mut c_void,
                 bits_stride_bytes: usize) {
        unsafe { check(self.ctx, zk_poseidon_tree_paths(self.t, d_indices, count, d_fields_out, field_stride_words, d_bits_out, bits_stride_bytes)) }
    }
    /// leaf d_indices[j] = d_values[j] (count u64 indices, count x 4 canonical words, on the device) and every node above, up to the
    /// root; an index >= n_leaves, a value >= r or an index that occurs twice is refused and leaves the tree as it was
    pub fn update(&mut self, d_indices: *const c_void, d_values: *const c_void, count: usize) {
        unsafe { check(self.ctx, zk_poseidon_tree_update(self.t, d_indices, d_values, count)) }
    }
    /// `count` more leaves (count x 4 canonical words on the device) behind the last one; dims() reports the new size
    pub fn append(&mut self, d_leaves: *const c_void, count: usize) {
        unsafe { check(self.ctx, zk_poseidon_tree_append(self.t, d_leaves, count)) }
    }
}

// ------------------------------------------------------------------------------------------------
// One `cargo test` on a machine with the crate settles every [recollection] above
// ------------------------------------------------------------------------------------------------
#[cfg(test)]
mod tests {
    use super::*;
    use super::super::fr::*;
    use super::super::EllipticEncryptable;

    #[test]
    fn bn_byte_layout_is_what_the_shim_assumes() {
        // Fr: 32 bytes big-endian
        let seven = FrLocal::from(7usize);
        assert_eq!(fr_to_words(&seven), [7, 0, 0, 0]);
        assert!(fr_from_words(&[7, 0, 0, 0]) == seven);
        // G1: 69 * (1, 2) (fr.rs:106-109) round-trips, and 2 * (1, 2) is the public EIP-196 value (tests/golden/alt_bn128.json, cdetrio11)
        let g = FrLocal::from(1usize).encrypt_g1();
        assert!(g1_from_words(&g1_to_words(&g)) == g);
        let two_g = g1_from_words(&[1, 0, 0, 0, 2, 0, 0, 0]) + g1_from_words(&[1, 0, 0, 0, 2, 0, 0, 0]);
        assert_eq!(g1_to_words(&two_g)[0], 0xd3c208c16d87cfd3);
        // G2: packing c1 * q + c0 round-trips through bn's decoder (which checks the curve equation)
        let h = FrLocal::from(1usize).encrypt_g2();
        assert!(g2_from_words(&g2_to_words(&h)) == h);
        // identity
        assert!(g1_to_words(&(g - g)).iter().all(|&x| x == 0));
    }

    #[test]
    fn simple_circuit_on_the_gpu() {
        // lib.rs:156-190 with gpu::{setup, prove, verify} in place of the generic functions
        use super::super::circuit::{ASTParser, TryParse};
        let code = include_str!("../../test_programs/simple.zk");
        let qap: QAP<CoefficientPoly<FrLocal>> = ASTParser::try_parse(code).unwrap().into();
        let weights = super::super::circuit::weights(code, &[FrLocal::from(3usize), FrLocal::from(2usize), FrLocal::from(4usize)]).unwrap();
        let (s1, s2) = setup(&qap);
        let proof = prove(&qap, (&s1, &s2), &weights);
        assert!(verify::<CoefficientPoly<FrLocal>>((&s1, &s2), &[FrLocal::from(2usize), FrLocal::from(34usize)], &proof));
        assert!(!verify::<CoefficientPoly<FrLocal>>((&s1, &s2), &[FrLocal::from(2usize), FrLocal::from(25usize)], &proof));
        // and interchangeably with the CPU functions: a GPU proof verifies on the CPU path, a CPU proof on the GPU path
        assert!(super::super::verify::<CoefficientPoly<FrLocal>, _, _, _, _>((s1_ref(&s1), &s2), &[FrLocal::from(2usize), FrLocal::from(34usize)], proof_ref(&proof)));
    }
    fn s1_ref(s: &SigmaG1<G1Local>) -> &SigmaG1<G1Local> { s }
    fn proof_ref(p: &Proof<G1Local, G2Local>) -> &Proof<G1Local, G2Local> { p }
}
