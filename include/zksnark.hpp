// zksnark.hpp -- C++17 host side above the C ABI (zkgpu.h), mirroring the reference crate's API for the
// accelerated path: same names, argument order and meaning, and error behaviour, so that code and tests
// written against republicprotocol/zksnark-rs read the same here.  Header-only; link with -lzkgpu.
//
//   reference (Rust)                                              here
//   ------------------------------------------------------------  -------------------------------------------
//   FrLocal, From<usize>, FromStr, + - * / neg   (fr.rs:18-99)     zksnark::FrLocal (canonical 4 x u64; arithmetic
//                                                                  through zk_fr_batch on the GPU)
//   ASTParser::try_parse(code) -> RootRepresentation              zksnark::ASTParser::try_parse(code) -> Circuit
//                                 (circuit/mod.rs:224-527)
//   groth16::weights(code, assignments)  (circuit/mod.rs:529-637)  zksnark::groth16::weights(code, assignments)
//   QAP<CoefficientPoly<FrLocal>>: From<root_rep> (fr.rs:140-173)  zksnark::QAP::from(ctx, circuit)
//   QAP { u, v, w, t, input, degree }    (groth16/mod.rs:60-67)    zksnark::QAP::from_dense(ctx, u, v, w, t, input)
//   groth16::setup(&qap) -> (SigmaG1, SigmaG2)  (mod.rs:134-197)   zksnark::groth16::setup(ctx, qap) -> Sigma
//   groth16::prove(&qap, (&s1, &s2), &weights)  (mod.rs:213-296)   zksnark::groth16::prove(ctx, qap, sigma, weights)
//   groth16::verify((s1, s2), &inputs, proof)   (mod.rs:299-320)   zksnark::groth16::verify(ctx, sigma, inputs, proof)
//   (none: prove drops the remainder, mod.rs:277)                  zksnark::groth16::is_satisfied / which_is_unsatisfied(ctx, qap, weights)
//   (none: a CRS is taken on trust)                                zksnark::groth16::check_setup(ctx, qap, sigma)
//   Circuit<T>, WireId, Word8, Word64, new_and .. keccak256,       zksnark::builder::Circuit (WireId, Word8, Word64), whose finish()
//   validate_order                 (circuit/builder/mod.rs)        is a zksnark::Circuit; zksnark::Boolgen: bit-sliced witnesses
//
// Where the reference panics (division by zero fr.rs:54,69; "Dividend must be non-zero" field/mod.rs:440;
// unwrap() of a ParseErr) this API throws zksnark::Error carrying the ABI status and message.  The
// randomness the reference draws inside setup / prove (thread_rng, mod.rs:139-145,231) is drawn here from
// std::random_device; the *_with variants take it as arguments (tests, reproducible runs).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "zkgpu.h"

namespace zksnark {

class Error : public std::runtime_error {
   public:
    int status;
    Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

// One device context; not shareable between threads without external locking (as the ABI).
class Context {
   public:
    explicit Context(int device = 0) {
        int rc = zk_ctx_create(device, &ctx_);
        if (rc != ZK_OK) throw Error(rc, std::string("zk_ctx_create: ") + zk_strerror(rc));   // no GPU: no CPU fallback
    }
    ~Context() { zk_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    zk_ctx* get() const { return ctx_; }
    void check(int rc, const char* where) const {
        if (rc != ZK_OK) throw Error(rc, std::string(where) + ": " + zk_strerror(rc) + " (" + zk_last_error(ctx_) + ")");
    }

   private:
    zk_ctx* ctx_ = nullptr;
};

// ---- FrLocal (fr.rs:9-99): an element of the BN254 scalar field, canonical integer --------------
struct FrLocal {
    std::array<uint64_t, 4> w{};   // little-endian words
    FrLocal() = default;
    FrLocal(uint64_t v) { w[0] = v; }                                   // From<usize> (fr.rs:73-77)
    bool operator==(const FrLocal& o) const { return w == o.w; }
    bool operator!=(const FrLocal& o) const { return !(*this == o); }
    static constexpr std::array<uint64_t, 4> MODULUS = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    bool in_range() const {
        for (int i = 3; i >= 0; --i)
            if (w[i] != MODULUS[i]) return w[i] < MODULUS[i];
        return false;
    }
    // Random::random_elem (fr.rs:89-99): uniform, rejection sampled
    static FrLocal random_elem() {
        static thread_local std::random_device rd;
        FrLocal x;
        do {
            for (auto& l : x.w) l = ((uint64_t)rd() << 32) | rd();
            x.w[3] &= (1ull << 62) - 1;
        } while (!x.in_range());
        return x;
    }
};

// field arithmetic needs a device; bind one Context to get operators with the reference's spelling
class Field {
   public:
    explicit Field(const Context& c) : c_(c) {}
    FrLocal add(const FrLocal& a, const FrLocal& b) const { return op(0, a, b); }
    FrLocal sub(const FrLocal& a, const FrLocal& b) const { return op(1, a, b); }
    FrLocal mul(const FrLocal& a, const FrLocal& b) const { return op(2, a, b); }
    FrLocal inv(const FrLocal& a) const { return op(3, a, a); }           // panics on zero in the reference (fr.rs:54,69)
    FrLocal div(const FrLocal& a, const FrLocal& b) const { return mul(a, inv(b)); }
    FrLocal neg(const FrLocal& a) const { return sub(FrLocal(0), a); }

   private:
    FrLocal op(int code, const FrLocal& a, const FrLocal& b) const {
        FrLocal r;
        c_.check(zk_fr_batch(c_.get(), code, a.w.data(), b.w.data(), r.w.data(), 1), "FrLocal arithmetic");
        return r;
    }
    const Context& c_;
};

// ---- front end -----------------------------------------------------------------------------------
// RootRepresentation produced by ASTParser::try_parse (circuit/mod.rs:224-527)
class Circuit {
   public:
    Circuit(Circuit&& o) noexcept : c_(std::exchange(o.c_, nullptr)) {}
    Circuit(const Circuit&) = delete;
    ~Circuit() { if (c_) zk_circuit_free(c_); }
    const zk_circuit* get() const { return c_; }
    static Circuit adopt(zk_circuit* c) { return Circuit(c); }   // takes ownership (builder::Circuit::finish)
    bool is_boolean() const { return zk_circuit_is_boolean(c_) != 0; }
    size_t packed_wires() const { size_t n = 0; zk_circuit_packed_wires(c_, &n); return n; }   // builder::Circuit::pack calls
    // witness index of a builder wire (built circuits; the constant-zero wire has none)
    size_t wire_index(uint32_t wire) const {
        size_t i = 0;
        if (zk_circuit_wire_index(c_, wire, &i) != ZK_OK) throw Error(ZK_ERR_ARG, "wire_index: the wire has no witness index in this circuit");
        return i;
    }
    // the split of a built circuit into a boolean core and a field tail (zk_circuit_mixed_dims)
    struct MixedDims { size_t n_bit_inputs, n_field_inputs, core_ops, core_levels, tail_ops, tail_levels, tail_slots; };
    MixedDims mixed_dims() const {
        MixedDims d{};
        int rc = zk_circuit_mixed_dims(c_, &d.n_bit_inputs, &d.n_field_inputs, &d.core_ops, &d.core_levels, &d.tail_ops, &d.tail_levels, &d.tail_slots);
        if (rc != ZK_OK) throw Error(rc, std::string("mixed_dims: ") + zk_circuit_last_error(c_));
        return d;
    }
    // weights() through the split, the host model of Mixgen::run: the bit inputs packed (bit k % 8 of byte k / 8 = the k-th bit input),
    // the field inputs in input order
    std::vector<FrLocal> weights_mixed(const std::vector<uint8_t>& in_bits, const std::vector<FrLocal>& in_fields) const {
        std::vector<FrLocal> out(wires());
        int rc = zk_circuit_weights_mixed(c_, in_bits.empty() ? nullptr : in_bits.data(), in_bits.size(),
                                          in_fields.empty() ? nullptr : in_fields[0].w.data(), in_fields.size(), out[0].w.data(), out.size());
        if (rc != ZK_OK) throw Error(rc, std::string("weights_mixed: ") + zk_circuit_last_error(c_));
        return out;
    }
    size_t wires() const { return dims()[0]; }
    size_t gates() const { return dims()[1]; }
    size_t input() const { return dims()[2]; }
    size_t assignments() const { return dims()[3]; }
    // circuit::weights: [1] ++ every wire value, inputs in `in` order
    std::vector<FrLocal> weights(const std::vector<FrLocal>& assignments_in) const {
        std::vector<FrLocal> out(wires());
        int rc = zk_circuit_weights(c_, assignments_in.empty() ? nullptr : assignments_in[0].w.data(), assignments_in.size(), out[0].w.data(), out.size());
        if (rc != ZK_OK) throw Error(rc, std::string("weights: ") + zk_circuit_last_error(c_));
        return out;
    }
    // the same through the compiled tape (zk_circuit_weights_tape)
    std::vector<FrLocal> weights_tape(const std::vector<FrLocal>& assignments_in) const {
        std::vector<FrLocal> out(wires());
        int rc = zk_circuit_weights_tape(c_, assignments_in.empty() ? nullptr : assignments_in[0].w.data(), assignments_in.size(), out[0].w.data(), out.size());
        if (rc != ZK_OK) throw Error(rc, std::string("weights: ") + zk_circuit_last_error(c_));
        return out;
    }

   private:
    friend struct ASTParser;
    explicit Circuit(zk_circuit* c) : c_(c) {}
    std::array<size_t, 4> dims() const {
        std::array<size_t, 4> d{};
        zk_circuit_dims(c_, &d[0], &d[1], &d[2], &d[3]);
        return d;
    }
    zk_circuit* c_;
};

struct ASTParser {
    // Result<_, ParseErr>: the Err arm is thrown, its text is the ParseErr's Debug form
    static Circuit try_parse(const std::string& code) {
        zk_circuit* c = nullptr;
        char err[512] = {0};
        int rc = zk_circuit_parse(code.c_str(), &c, err, sizeof(err));
        if (rc != ZK_OK) throw Error(rc, std::string("ParseErr: ") + err);
        return Circuit(c);
    }
};

// ---- QAP<CoefficientPoly<FrLocal>> (groth16/mod.rs:60-67), device resident ------------------------
class QAP {
   public:
    QAP(QAP&& o) noexcept : q_(std::exchange(o.q_, nullptr)) {}
    QAP(const QAP&) = delete;
    ~QAP() { if (q_) zk_qap_free(q_); }
    // From<RootRepresentation> (fr.rs:140-173): Lagrange interpolation over the circuit's roots 1..n
    static QAP from(const Context& c, const Circuit& circuit) {
        zk_qap* q = nullptr;
        c.check(zk_circuit_qap(c.get(), circuit.get(), &q), "QAP::from");
        return QAP(q);
    }
    // the same QAP kept as rows over the roots 1..n (zk_circuit_qap_sparse): no interpolation, any size, identical proofs; the form
    // groth16::is_satisfied / which_is_unsatisfied take
    static QAP from_sparse(const Context& c, const Circuit& circuit) {
        zk_qap* q = nullptr;
        c.check(zk_circuit_qap_sparse(c.get(), circuit.get(), &q), "QAP::from_sparse");
        return QAP(q);
    }
    // the same rows at the roots of unity (zk_circuit_qap_sparse_unity): gate k at w^k, n padded to a power of two; the faster prover
    static QAP from_sparse_unity(const Context& c, const Circuit& circuit) {
        zk_qap* q = nullptr;
        c.check(zk_circuit_qap_sparse_unity(c.get(), circuit.get(), &q), "QAP::from_sparse_unity");
        return QAP(q);
    }
    // the struct literal QAP { u, v, w, t, input, degree }: u, v, w = m polynomials of `degree` coefficients
    // (shorter ones are zero padded), t = degree + 1 coefficients
    static QAP from_dense(const Context& c, const std::vector<std::vector<FrLocal>>& u, const std::vector<std::vector<FrLocal>>& v,
                          const std::vector<std::vector<FrLocal>>& w, const std::vector<FrLocal>& t, size_t input) {
        const size_t m = u.size(), n = t.size() - 1;
        auto flat = [&](const std::vector<std::vector<FrLocal>>& p) {
            std::vector<uint64_t> out(m * n * 4, 0);
            for (size_t i = 0; i < m; ++i)
                for (size_t k = 0; k < p[i].size() && k < n; ++k)
                    for (int l = 0; l < 4; ++l) out[(i * n + k) * 4 + l] = p[i][k].w[l];
            return out;
        };
        if (v.size() != m || w.size() != m) throw Error(ZK_ERR_ARG, "QAP: u, v, w must have one polynomial per wire");
        auto fu = flat(u), fv = flat(v), fw = flat(w);
        zk_qap* q = nullptr;
        c.check(zk_qap_upload_dense(c.get(), fu.data(), fv.data(), fw.data(), t[0].w.data(), m, n, input, &q), "QAP");
        return QAP(q);
    }
    // From<RootRepresentation> for ANY root representation (circuit/mod.rs:201-214; fr.rs:140-173): u, v, w = one row per wire of
    // (root, value) pairs, roots = the representation's distinct roots in gate order, `input` as RootRepresentation::input().  The
    // wire polynomials are never interpolated (zk_qap_upload_sparse_roots): any size up to 2^22 gates, the reference's proof bytes.
    typedef std::vector<std::vector<std::pair<FrLocal, FrLocal>>> Rows;
    static QAP from_root_rep(const Context& c, const std::vector<FrLocal>& roots, const Rows& u, const Rows& v, const Rows& w, size_t input) {
        const size_t n = roots.size(), m = u.size();
        if (v.size() != m || w.size() != m) throw Error(ZK_ERR_ARG, "QAP: u, v, w must have one row per wire");
        auto index_of = [&](const FrLocal& r) {
            for (size_t j = 0; j < n; ++j) if (roots[j].w == r.w) return (uint32_t)j;
            throw Error(ZK_ERR_ARG, "QAP: a row names a root that roots() does not list");
        };
        struct Csr { std::vector<uint64_t> ptr, val; std::vector<uint32_t> gate; };
        auto pack = [&](const Rows& rows) {
            Csr x;
            x.ptr.push_back(0);
            for (const auto& row : rows) {
                for (const auto& e : row) {
                    x.gate.push_back(index_of(e.first));
                    x.val.insert(x.val.end(), e.second.w.begin(), e.second.w.end());
                }
                x.ptr.push_back(x.gate.size());
            }
            if (x.gate.empty()) { x.gate.push_back(0); x.val.resize(4); }   // non-null pointers for empty rows
            return x;
        };
        Csr cu = pack(u), cv = pack(v), cw = pack(w);
        std::vector<uint64_t> rw(4 * n);
        for (size_t j = 0; j < n; ++j) std::copy(roots[j].w.begin(), roots[j].w.end(), rw.begin() + 4 * j);
        zk_qap_sparse_desc d{};
        d.log_n = 0; d.m = m; d.input = input;
        d.u = zk_sparse_rows{cu.ptr.data(), cu.gate.data(), cu.val.data()};
        d.v = zk_sparse_rows{cv.ptr.data(), cv.gate.data(), cv.val.data()};
        d.w = zk_sparse_rows{cw.ptr.data(), cw.gate.data(), cw.val.data()};
        zk_qap* q = nullptr;
        c.check(zk_qap_upload_sparse_roots(c.get(), &d, rw.data(), n, &q), "QAP::from_root_rep");
        return QAP(q);
    }
    const zk_qap* get() const { return q_; }
    size_t degree() const { size_t n, m, l; int d; zk_qap_dims(q_, &n, &m, &l, &d); return n; }
    size_t wires() const { size_t n, m, l; int d; zk_qap_dims(q_, &n, &m, &l, &d); return m; }
    size_t input() const { size_t n, m, l; int d; zk_qap_dims(q_, &n, &m, &l, &d); return l; }

   private:
    explicit QAP(zk_qap* q) : q_(q) {}
    zk_qap* q_;
};

// ---- the gate-level circuit builder (circuit/builder/mod.rs, types.rs) -------------------------------
namespace builder {

typedef uint32_t WireId;                       // WireId(0) = the constant 0, WireId(1) = the constant 1 (mod.rs:91-114)
typedef std::array<WireId, 8> Word8;           // least significant bit first (types.rs)
typedef std::array<WireId, 64> Word64;         // 8 Word8s, little endian: bit i of the number is wire i
enum class Gate { BitChecker = ZK_GATE_BIT_CHECK, Not = ZK_GATE_NOT, And = ZK_GATE_AND, Or = ZK_GATE_OR, Xor = ZK_GATE_XOR, Nand = ZK_GATE_NAND,
                  Nor = ZK_GATE_NOR, Xnor = ZK_GATE_XNOR, LessThan = ZK_GATE_LESS, GreaterThan = ZK_GATE_GREATER };
struct ValidateOrder {                         // mod.rs:30-36
    WireId is_x_within_range, is_y_greater_than_c;
    std::array<Word8, 32> hash_x_y;
};

// Circuit<FrLocal> (mod.rs:56-64): the reference's method names over zk_builder_*.  Where the reference takes a gate constructor
// (Circuit::new_xor) this takes the Gate.  What differs from the reference is listed in zkgpu.h at zk_builder_create.
class Circuit {
   public:
    Circuit() { if (zk_builder_create(&b_) != ZK_OK) throw Error(ZK_ERR_ARG, "zk_builder_create"); }
    Circuit(Circuit&& o) noexcept : b_(std::exchange(o.b_, nullptr)) {}
    Circuit(const Circuit&) = delete;
    ~Circuit() { zk_builder_free(b_); }
    zk_builder* get() const { return b_; }
    WireId zero_wire() const { return ZK_WIRE_ZERO; }
    WireId unity_wire() const { return ZK_WIRE_ONE; }
    size_t wires() const { size_t w = 0, g = 0; check(zk_builder_dims(b_, &w, &g)); return w; }
    size_t gates() const { size_t w = 0, g = 0; check(zk_builder_dims(b_, &w, &g)); return g; }

    WireId new_wire() { WireId w; check(zk_builder_new_wires(b_, ZK_WIRE_FIELD, 1, &w)); return w; }   // any field element: not boolean
    WireId new_bit() { WireId w; check(zk_builder_new_wires(b_, ZK_WIRE_BIT, 1, &w)); return w; }
    Word8 new_word8() { Word8 w; check(zk_builder_new_wires(b_, ZK_WIRE_BIT, 8, w.data())); return w; }
    Word64 new_word64() { Word64 w; check(zk_builder_new_wires(b_, ZK_WIRE_BIT, 64, w.data())); return w; }
    std::vector<Word8> new_word8_vec(size_t size) { std::vector<Word8> v(size); for (auto& w : v) w = new_word8(); return v; }
    Word8 const_word8(uint8_t x) const { Word8 w; for (int i = 0; i < 8; ++i) w[i] = (x >> i) & 1; return w; }
    Word64 const_word64(uint64_t x) const { Word64 w; for (int i = 0; i < 64; ++i) w[i] = (WireId)((x >> i) & 1); return w; }

    typedef std::vector<std::pair<FrLocal, WireId>> Side;
    WireId new_sub_circuit(const Side& lhs, const Side& rhs) {
        std::vector<uint64_t> lw, rw;
        std::vector<WireId> li, ri;
        for (const auto& t : lhs) { lw.insert(lw.end(), t.first.w.begin(), t.first.w.end()); li.push_back(t.second); }
        for (const auto& t : rhs) { rw.insert(rw.end(), t.first.w.begin(), t.first.w.end()); ri.push_back(t.second); }
        WireId out;
        check(zk_builder_sub_circuit(b_, lw.data(), li.data(), li.size(), rw.data(), ri.data(), ri.size(), &out));
        return out;
    }
    WireId gate(Gate g, WireId x, WireId y = ZK_WIRE_ZERO) { WireId o; check(zk_builder_gate(b_, (int)g, x, y, &o)); return o; }
    WireId new_bit_checker(WireId x) { return gate(Gate::BitChecker, x); }
    WireId new_not(WireId x) { return gate(Gate::Not, x); }
    WireId new_and(WireId x, WireId y) { return gate(Gate::And, x, y); }
    WireId new_or(WireId x, WireId y) { return gate(Gate::Or, x, y); }
    WireId new_xor(WireId x, WireId y) { return gate(Gate::Xor, x, y); }
    WireId new_nand(WireId x, WireId y) { return gate(Gate::Nand, x, y); }
    WireId new_nor(WireId x, WireId y) { return gate(Gate::Nor, x, y); }
    WireId new_xnor(WireId x, WireId y) { return gate(Gate::Xnor, x, y); }
    // w (w - 1) = 0 without output wire: what forces an input to be 0 or 1 (not in the reference)
    void assert_bit(WireId w) { check(zk_builder_assert_bit(b_, w)); }
    // the packed wire sum 2^i bits[i] over 1..ZK_PACK_MAX_BITS wires, least significant first: one sub-circuit whose output is a field
    // element (not in the reference); a 32-byte digest is two of them as verify wires instead of 256 bits
    template <class Wires>
    WireId pack(const Wires& bits) { WireId o; check(zk_builder_pack(b_, bits.data(), bits.size(), &o)); return o; }

    // Poseidon of 1, 2 or 4 wires (poseidon::hash on their values): 217 / 244 / 301 general sub-circuits; the output is a field element
    template <class Wires>
    WireId poseidon(const Wires& inputs) { WireId o; check(zk_builder_poseidon(b_, inputs.data(), inputs.size(), &o)); return o; }
    // the root of the Merkle path leaf, siblings[k], dirs[k] (1: the right child at level k) over Poseidon of arity 2: 246 gates a level
    template <class Wires>
    WireId merkle_root(WireId leaf, const Wires& siblings, const Wires& dirs) {
        if (siblings.size() != dirs.size()) throw Error(ZK_ERR_ARG, "merkle_root: one direction per sibling");
        WireId o;
        check(zk_builder_merkle_root(b_, leaf, siblings.data(), dirs.data(), dirs.size(), &o));
        return o;
    }

    // Baby Jubjub (babyjub::): a point is three wires (X, Y, Z), projective; an affine point is (x, y, ZK_WIRE_ONE)
    typedef std::array<WireId, 3> Point;
    // a x^2 + y^2 = 1 + d x^2 y^2 on the wires (x, y): 4 gates, the last one an assertion without output
    void babyjub_assert_on_curve(WireId x, WireId y) { const WireId xy[2] = {x, y}; check(zk_builder_babyjub_assert_on_curve(b_, xy)); }
    // p + q, right for all pairs of curve points: 11 gates, 10 when q's Z is ZK_WIRE_ONE; the operands are not asserted on the curve
    Point babyjub_add(const Point& p, const Point& q) { Point o; check(zk_builder_babyjub_add(b_, p.data(), q.data(), o.data())); return o; }
    // [sum 2^i bits[i]] Base8 over 1..256 bit wires, each asserted: 1414 gates for 251 bits
    template <class Wires>
    Point babyjub_mul_fixed(const Wires& bits) { Point o; check(zk_builder_babyjub_mul_fixed(b_, bits.data(), bits.size(), o.data())); return o; }
    // [sum 2^i bits[i]] P for the affine wires (px, py), asserted on the curve: 4 + n + 2 + 19 (n - 1) gates
    template <class Wires>
    Point babyjub_mul(WireId px, WireId py, const Wires& bits) {
        const WireId xy[2] = {px, py};
        Point o;
        check(zk_builder_babyjub_mul(b_, xy, bits.data(), bits.size(), o.data()));
        return o;
    }
    // pins the existing wires (x, y) as the affine form of p: 4 gates
    void babyjub_affine(const Point& p, WireId x, WireId y) { const WireId xy[2] = {x, y}; check(zk_builder_babyjub_affine(b_, p.data(), xy)); }

    // EdDSA-Poseidon (eddsa::): [S] Base8 = R8 + [8] ([hm] A), hm = H6(R8, A, M), over the affine wires of A and R8, the message wire, the
    // 251 bit wires of S and the 254 bit wires of hm (supplied by the caller; eddsa::verify_batch writes them): 73384 gates
    template <class Wires>
    void eddsa_verify(WireId ax, WireId ay, WireId r8x, WireId r8y, WireId msg, const Wires& s_bits, const Wires& hm_bits) {
        if (s_bits.size() != 251 || hm_bits.size() != 254) throw Error(ZK_ERR_ARG, "eddsa_verify: 251 bit wires of S and 254 of hm are expected");
        const WireId a[2] = {ax, ay}, r8[2] = {r8x, r8y};
        check(zk_builder_eddsa_verify(b_, a, r8, msg, s_bits.data(), hm_bits.data()));
    }

    template <class Wires>
    WireId fan_in(const Wires& inputs, Gate g) { WireId o; check(zk_builder_fan_in(b_, (int)g, inputs.data(), inputs.size(), &o)); return o; }
    template <class Wires>
    Wires bitwise_op(const Wires& l, const Wires& r, Gate g) {
        if (l.size() != r.size()) throw Error(ZK_ERR_ARG, "bitwise_op: arrays of different lengths");
        Wires o = l;
        check(zk_builder_bitwise(b_, (int)g, l.data(), r.data(), l.size(), o.data()));
        return o;
    }
    Word8 u8_bitwise_op(const Word8& l, const Word8& r, Gate g) { return bitwise_op(l, r, g); }
    Word64 u64_bitwise_op(const Word64& l, const Word64& r, Gate g) { return bitwise_op(l, r, g); }
    template <class Wires>
    Wires unary_op(const Wires& x, Gate g) { Wires o = x; check(zk_builder_bitwise(b_, (int)g, x.data(), nullptr, x.size(), o.data())); return o; }
    Word8 u8_unary_op(const Word8& x, Gate g) { return unary_op(x, g); }
    Word64 u64_unary_op(const Word64& x, Gate g) { return unary_op(x, g); }

    template <class Wires> WireId is_equal(const Wires& l, const Wires& r) { return compare(ZK_CMP_EQUAL, l, &r); }
    template <class Wires> WireId is_equal_zero(const Wires& x) { return compare(ZK_CMP_EQUAL_ZERO, x, (const Wires*)nullptr); }
    template <class Wires> WireId less_than(const Wires& l, const Wires& r) { return compare(ZK_CMP_LESS, l, &r); }
    template <class Wires> WireId less_than_eq(const Wires& l, const Wires& r) { return compare(ZK_CMP_LESS_EQ, l, &r); }
    template <class Wires> WireId greater_than(const Wires& l, const Wires& r) { return compare(ZK_CMP_GREATER, l, &r); }
    template <class Wires> WireId greater_than_eq(const Wires& l, const Wires& r) { return compare(ZK_CMP_GREATER_EQ, l, &r); }

    // the sponge in general form: rate in bytes, the delimiter byte, rounds of Keccak-f[1600] (24 = the real permutation)
    std::vector<Word8> keccak(const std::vector<Word8>& input, unsigned rate, unsigned delim, unsigned rounds, size_t out_bytes) {
        std::vector<Word8> out(out_bytes);
        check(zk_builder_keccak(b_, input.empty() ? nullptr : input[0].data(), input.size(), rate, delim, rounds, out.empty() ? nullptr : out[0].data(),
                                out_bytes));
        return out;
    }
    std::array<Word8, 32> keccak256(const std::vector<Word8>& input) {
        std::array<Word8, 32> out;
        check(zk_builder_keccak(b_, input.empty() ? nullptr : input[0].data(), input.size(), 136, 0x01, 24, out[0].data(), 32));
        return out;
    }
    // the reference absorbs a stream byte by byte; the sub-circuits and their order are keccak256's
    std::array<Word8, 32> keccak256_stream(const std::vector<Word8>& input) { return keccak256(input); }
    ValidateOrder validate_order(const Word64& input_x, const std::pair<Word64, Word64>& pub_range, const Word64& input_y, const Word64& pub_c) {
        const WireId x_geq = greater_than_eq(input_x, pub_range.first);
        const WireId x_leq = less_than_eq(input_x, pub_range.second);
        ValidateOrder v;
        v.is_x_within_range = new_and(x_geq, x_leq);
        v.is_y_greater_than_c = greater_than_eq(input_y, pub_c);
        std::vector<Word8> stream(16);
        for (int k = 0; k < 8; ++k)
            for (int i = 0; i < 8; ++i) { stream[k][i] = input_x[8 * k + i]; stream[8 + k][i] = input_y[8 * k + i]; }
        v.hash_x_y = keccak256_stream(stream);
        return v;
    }
    // -> the circuit as a RootRepresentation: witness = [1], `verify` as given, the other inputs in creation order, the other wires by id
    zksnark::Circuit finish(const std::vector<WireId>& verify) {
        zk_circuit* c = nullptr;
        check(zk_builder_finish(b_, verify.data(), verify.size(), &c));
        return zksnark::Circuit::adopt(c);
    }

   private:
    void check(int rc) const {
        if (rc != ZK_OK) throw Error(rc, std::string("builder: ") + zk_builder_last_error(b_));
    }
    template <class Wires>
    WireId compare(int kind, const Wires& l, const Wires* r) {
        if (r && r->size() != l.size()) throw Error(ZK_ERR_ARG, "comparator: arrays of different lengths");
        WireId o;
        check(zk_builder_compare(b_, kind, l.data(), r ? r->data() : nullptr, l.size(), &o));
        return o;
    }
    zk_builder* b_ = nullptr;
};

}  // namespace builder

// zk_boolgen_*: the witnesses of a boolean built circuit for many input sets at once, bit-sliced (device pointers in and out)
class Boolgen {
   public:
    Boolgen(const Context& c, const Circuit& circuit) : c_(c) { c.check(zk_boolgen_create(c.get(), circuit.get(), &g_), "Boolgen"); }
    Boolgen(const Boolgen&) = delete;
    ~Boolgen() { zk_boolgen_free(g_); }
    void run(const void* d_in_bits, size_t in_stride_bytes, size_t count, void* d_weights_out, size_t m) const {
        c_.check(zk_boolgen_run(g_, d_in_bits, in_stride_bytes, count, d_weights_out, m), "Boolgen::run");
    }
    void eval(const void* d_in_bits, size_t in_stride_bytes, size_t count, const std::vector<uint32_t>& wires, void* d_out_bits,
              size_t out_stride_bytes) const {
        c_.check(zk_boolgen_eval(g_, d_in_bits, in_stride_bytes, count, wires.data(), wires.size(), d_out_bits, out_stride_bytes), "Boolgen::eval");
    }
    // bit and packed wires alike as 4 canonical words each: with wires = 1..l the `inputs` of zk_verify_batch
    void eval_fields(const void* d_in_bits, size_t in_stride_bytes, size_t count, const std::vector<uint32_t>& wires, void* d_out_words) const {
        c_.check(zk_boolgen_eval_fields(g_, d_in_bits, in_stride_bytes, count, wires.data(), wires.size(), d_out_words), "Boolgen::eval_fields");
    }

   private:
    const Context& c_;
    zk_boolgen* g_ = nullptr;
};

// zk_mixgen_*: the witnesses of ANY built circuit for many input sets at once: the boolean core bit-sliced, the field tail one instance
// per lane (device pointers in and out; d_in_fields: 4 canonical words per field input, instance-major)
class Mixgen {
   public:
    Mixgen(const Context& c, const Circuit& circuit) : c_(c) { c.check(zk_mixgen_create(c.get(), circuit.get(), &g_), "Mixgen"); }
    Mixgen(const Mixgen&) = delete;
    ~Mixgen() { zk_mixgen_free(g_); }
    void run(const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count, void* d_weights_out, size_t m) const {
        c_.check(zk_mixgen_run(g_, d_in_bits, in_stride_bytes, d_in_fields, count, d_weights_out, m), "Mixgen::run");
    }
    // wires of either class as 4 canonical words each: with wires = 1..l the `inputs` of zk_verify_batch
    void eval_fields(const void* d_in_bits, size_t in_stride_bytes, const void* d_in_fields, size_t count, const std::vector<uint32_t>& wires,
                     void* d_out_words) const {
        c_.check(zk_mixgen_eval_fields(g_, d_in_bits, in_stride_bytes, d_in_fields, count, wires.data(), wires.size(), d_out_words),
                 "Mixgen::eval_fields");
    }

   private:
    const Context& c_;
    zk_mixgen* g_ = nullptr;
};

// Poseidon over Fr, circomlib's parameter sets (zk_poseidon_*): hash of 1, 2 or 4 elements on the host, `count` hashes on the device
namespace poseidon {
inline FrLocal hash(const std::vector<FrLocal>& inputs) {
    FrLocal out;
    const int rc = zk_poseidon_hash(inputs.empty() ? nullptr : inputs[0].w.data(), inputs.size(), out.w.data());
    if (rc != ZK_OK) throw Error(rc, rc == ZK_ERR_RANGE ? "poseidon: an input is not below r" : "poseidon: the arity must be 1, 2 or 4");
    return out;
}
// z_0 = 0, z_{k+1} = hash(z_k, z_k): depth + 1 elements
inline std::vector<FrLocal> zero_hashes(unsigned depth) {
    std::vector<FrLocal> z{FrLocal(0)};
    for (unsigned k = 0; k < depth; ++k) z.push_back(hash({z.back(), z.back()}));
    return z;
}
// d_inputs: count x arity elements, d_out: count elements (device pointers, canonical words)
inline void hash_batch(const Context& c, const void* d_inputs, size_t arity, size_t count, void* d_out) {
    c.check(zk_poseidon_hash_batch(c.get(), d_inputs, arity, count, d_out), "poseidon::hash_batch");
}
}  // namespace poseidon

// Baby Jubjub over Fr (zk_babyjub_*): a x^2 + y^2 = 1 + d x^2 y^2, a = 168700, d = 168696; the identity is (0, 1).  A coordinate >= r
// and a point off the curve both throw Error(ZK_ERR_RANGE).
namespace babyjub {
struct Point {
    FrLocal x, y;
    bool operator==(const Point& o) const { return x.w == o.x.w && y.w == o.y.w; }
};
struct Params { FrLocal a, d, order; Point base8, generator; };
namespace detail {
inline void words(const Point& p, uint64_t w[8]) { std::copy(p.x.w.begin(), p.x.w.end(), w); std::copy(p.y.w.begin(), p.y.w.end(), w + 4); }
inline Point point(const uint64_t w[8]) { Point p; std::copy(w, w + 4, p.x.w.begin()); std::copy(w + 4, w + 8, p.y.w.begin()); return p; }
inline void check(int rc) {
    if (rc < 0) throw Error(rc, rc == ZK_ERR_RANGE ? "babyjub: a coordinate is not below r, or the point is not on the curve" : "babyjub: bad argument");
}
}  // namespace detail
inline Params params() {
    Params p;
    uint64_t b[8], g[8];
    detail::check(zk_babyjub_params(p.a.w.data(), p.d.w.data(), p.order.w.data(), b, g));
    p.base8 = detail::point(b);
    p.generator = detail::point(g);
    return p;
}
inline bool on_curve(const Point& p) {
    uint64_t w[8];
    detail::words(p, w);
    const int rc = zk_babyjub_on_curve(w);
    detail::check(rc);
    return rc == 1;
}
inline Point add(const Point& p, const Point& q) {
    uint64_t a[8], b[8], o[8];
    detail::words(p, a);
    detail::words(q, b);
    detail::check(zk_babyjub_add(a, b, o));
    return detail::point(o);
}
// [scalar] p; the scalar is four words of 64 bits, least significant first, taken as an integer; p == nullptr: Base8
inline Point mul(const std::array<uint64_t, 4>& scalar, const Point* p = nullptr) {
    uint64_t a[8], o[8];
    if (p) detail::words(*p, a);
    detail::check(zk_babyjub_mul(scalar.data(), p ? a : nullptr, o));
    return detail::point(o);
}
// d_scalars: count x 4 words, d_points: count x 8 canonical words or nullptr for Base8, d_out: 8 words per result, out_stride_words
// apart (0: packed, the input of poseidon::hash_batch of arity 2); device pointers
inline void mul_batch(const Context& c, const void* d_scalars, const void* d_points, size_t count, void* d_out, size_t out_stride_words = 0) {
    c.check(zk_babyjub_mul_batch(c.get(), d_scalars, d_points, count, d_out, out_stride_words), "babyjub::mul_batch");
}
}  // namespace babyjub

// EdDSA-Poseidon on Baby Jubjub (zk_eddsa_*; include/zkgpu.h states the scheme): a secret key is 0 < k < l, a public key [k] Base8, a
// signature (R8, S).  A malformed signature is a verdict (Status), not an error.
namespace eddsa {
enum class Status : int { Valid = ZK_EDDSA_VALID, Range = ZK_EDDSA_RANGE, KeyOffCurve = ZK_EDDSA_KEY_OFF_CURVE, ROffCurve = ZK_EDDSA_R_OFF_CURVE,
                          SRange = ZK_EDDSA_S_RANGE, Mismatch = ZK_EDDSA_MISMATCH };
struct Signature { babyjub::Point r8; FrLocal s; };
namespace detail {
inline void check(int rc, const char* range) {
    if (rc < 0) throw Error(rc, rc == ZK_ERR_RANGE ? range : "eddsa: bad argument");
}
}  // namespace detail
// H6(R8.x, R8.y, A.x, A.y, M): any five field elements, no curve check
inline FrLocal challenge(const babyjub::Point& r8, const babyjub::Point& a, const FrLocal& msg) {
    uint64_t r[8], p[8];
    babyjub::detail::words(r8, r);
    babyjub::detail::words(a, p);
    FrLocal out;
    detail::check(zk_eddsa_challenge(r, p, msg.w.data(), out.w.data()), "eddsa: an element is not below r");
    return out;
}
inline babyjub::Point public_key(const FrLocal& k) {
    uint64_t o[8];
    detail::check(zk_eddsa_public_key(k.w.data(), o), "eddsa: the key is 0 or not below l");
    return babyjub::detail::point(o);
}
inline Signature sign(const FrLocal& k, const FrLocal& nonce_key, const FrLocal& msg) {
    uint64_t o[8];
    Signature sig;
    detail::check(zk_eddsa_sign(k.w.data(), nonce_key.w.data(), msg.w.data(), o, sig.s.w.data()),
                  "eddsa: the key is 0 or not below l, or the nonce key or the message is not below r");
    sig.r8 = babyjub::detail::point(o);
    return sig;
}
inline Status verify(const babyjub::Point& a, const FrLocal& msg, const Signature& sig) {
    uint64_t p[8], r[8];
    babyjub::detail::words(a, p);
    babyjub::detail::words(sig.r8, r);
    int status = 0;
    detail::check(zk_eddsa_verify(p, msg.w.data(), r, sig.s.w.data(), &status), "eddsa: bad argument");
    return (Status)status;
}
// d_points_msg: count x 20 words (A.x, A.y, R8.x, R8.y, M), d_s: count x 4 words, d_status: count x uint32 (Status); d_bits_out:
// nullptr, or rows of bits_stride_bytes with the 251 bits of S and the 254 bits of hm (Mixgen::run's d_in_bits); device pointers
inline void verify_batch(const Context& c, const void* d_points_msg, const void* d_s, size_t count, void* d_status, void* d_bits_out = nullptr,
                         size_t bits_stride_bytes = 64) {
    c.check(zk_eddsa_verify_batch(c.get(), d_points_msg, d_s, count, d_status, d_bits_out, bits_stride_bytes), "eddsa::verify_batch");
}
// d_keys, d_nonce_keys, d_msgs: count x 4 words each (0 < k < l, n < r, M < r); instance j is signed as sign(k_j, n_j, M_j).
// d_points_msg_out: count x 20 words (A.x, A.y, R8.x, R8.y, M), A = [k] Base8 computed in the call; d_s_out: count x 4 words -- the
// inputs of verify_batch; d_bits_out: nullptr, or the rows verify_batch writes; device pointers.  An input out of range throws
// (ZK_ERR_RANGE, the text naming the lowest instance and the input) before anything is written
inline void sign_batch(const Context& c, const void* d_keys, const void* d_nonce_keys, const void* d_msgs, size_t count, void* d_points_msg_out,
                       void* d_s_out, void* d_bits_out = nullptr, size_t bits_stride_bytes = 64) {
    c.check(zk_eddsa_sign_batch(c.get(), d_keys, d_nonce_keys, d_msgs, count, d_points_msg_out, d_s_out, d_bits_out, bits_stride_bytes),
            "eddsa::sign_batch");
}
}  // namespace eddsa

// zk_poseidon_tree_*: a binary Merkle tree over Poseidon of arity 2 that stays on the device; paths() writes leaf | siblings and the
// direction bits in the layout Mixgen::run reads as d_in_fields and d_in_bits
class PoseidonTree {
   public:
    PoseidonTree(const Context& c, const void* d_leaves, size_t n_leaves, unsigned depth) : c_(c) {
        c.check(zk_poseidon_tree_build(c.get(), d_leaves, n_leaves, depth, &t_), "PoseidonTree");
    }
    PoseidonTree(const PoseidonTree&) = delete;
    ~PoseidonTree() { zk_poseidon_tree_free(t_); }
    FrLocal root() const { FrLocal r; c_.check(zk_poseidon_tree_root(t_, r.w.data()), "PoseidonTree::root"); return r; }
    size_t n_leaves() const { size_t n = 0; c_.check(zk_poseidon_tree_dims(t_, &n, nullptr), "PoseidonTree::dims"); return n; }
    unsigned depth() const { unsigned d = 0; c_.check(zk_poseidon_tree_dims(t_, nullptr, &d), "PoseidonTree::dims"); return d; }
    std::vector<FrLocal> nodes(unsigned level) const {
        const size_t n = n_leaves();
        const size_t above = level > 63 ? 0 : (n + (((size_t)1 << level) - 1)) >> level;
        std::vector<FrLocal> out(level == 0 ? n : above ? above : 1);
        c_.check(zk_poseidon_tree_nodes(t_, level, out.empty() ? nullptr : out[0].w.data()), "PoseidonTree::nodes");
        return out;
    }
    void paths(const void* d_indices, size_t count, void* d_fields_out, size_t field_stride_words, void* d_bits_out, size_t bits_stride_bytes) const {
        c_.check(zk_poseidon_tree_paths(t_, d_indices, count, d_fields_out, field_stride_words, d_bits_out, bits_stride_bytes), "PoseidonTree::paths");
    }
    // leaf d_indices[j] = d_values[j] (count uint64 indices, count x 4 canonical words, on the device) and every node above, up to the
    // root; an index >= n_leaves, a value >= r or an index that occurs twice is refused and leaves the tree as it was
    void update(const void* d_indices, const void* d_values, size_t count) {
        c_.check(zk_poseidon_tree_update(t_, d_indices, d_values, count), "PoseidonTree::update");
    }
    // `count` more leaves (count x 4 canonical words on the device) behind the last one; n_leaves() follows
    void append(const void* d_leaves, size_t count) { c_.check(zk_poseidon_tree_append(t_, d_leaves, count), "PoseidonTree::append"); }

   private:
    const Context& c_;
    zk_poseidon_tree* t_ = nullptr;
};

namespace groth16 {

// (SigmaG1, SigmaG2) (groth16/mod.rs:105-121), device resident
using Tag = std::array<uint8_t, 32>;   // what a contribution record is bound to (contribute, below)
struct Contribution;
// A powers-of-tau transcript (setup_from_powers, below): canonical affine words, 8 per G1 point and 16 per G2 point.  tau_g1 holds at
// least 2n - 1 points for a QAP of n gates; tau_g2, alpha_tau_g1 and beta_tau_g1 one common count of at least n.
struct PowersOfTau {
    std::vector<uint64_t> tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1;
    std::array<uint64_t, ZK_G2_WORDS> beta_g2{};
};
class Sigma {
   public:
    Sigma(Sigma&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Sigma(const Sigma&) = delete;
    ~Sigma() { if (s_) zk_crs_free(s_); }
    const zk_crs* get() const { return s_; }
    void save(const Context& c, const std::string& path) const { c.check(zk_crs_save(c.get(), s_, path.c_str()), "Sigma::save"); }
    static Sigma load(const Context& c, const std::string& path) {
        zk_crs* s = nullptr;
        c.check(zk_crs_load(c.get(), path.c_str(), &s), "Sigma::load");
        return Sigma(s);
    }

   private:
    friend Sigma setup_with(const Context&, const QAP&, const std::array<FrLocal, 5>&);
    friend Sigma setup_from_powers(const Context&, const QAP&, const PowersOfTau&);
    friend std::pair<Sigma, Contribution> contribute_with(const Context&, const Sigma&, const FrLocal&, const Tag&);
    friend std::pair<Sigma, Contribution> contribute(const Context&, const Sigma&, const Tag&);
    explicit Sigma(zk_crs* s) : s_(s) {}
    zk_crs* s_;
};

// Proof { a, b, c } (groth16/mod.rs:124-128) in the canonical 259-byte encoding
struct Proof {
    std::array<uint8_t, ZK_PROOF_BYTES> bytes{};
    bool operator==(const Proof& o) const { return bytes == o.bytes; }
};

// the same proof in the compressed 128-byte form (zkgpu.h "Compressed proof bytes": x coordinates, the sign of y in a flag)
struct CompressedProof {
    std::array<uint8_t, ZK_PROOF_COMPRESSED_BYTES> bytes{};
    bool operator==(const CompressedProof& o) const { return bytes == o.bytes; }
};
// zk_proof_compress / zk_proof_decompress: host code, no context.  Error(ZK_ERR_RANGE) for a proof that is no canonical encoding
// of points on their curves / for bytes that are no valid compressed proof.
inline CompressedProof compress(const Proof& p) {
    CompressedProof c;
    const int st = zk_proof_compress(p.bytes.data(), c.bytes.data());
    if (st != ZK_OK) throw Error(st, "groth16::compress: not a canonical proof encoding");
    return c;
}
inline Proof decompress(const CompressedProof& c) {
    Proof p;
    const int st = zk_proof_decompress(c.bytes.data(), p.bytes.data());
    if (st != ZK_OK) throw Error(st, "groth16::decompress: not a valid compressed proof");
    return p;
}

// weights(code, assignments) (circuit/mod.rs:529-637)
inline std::vector<FrLocal> weights(const std::string& code, const std::vector<FrLocal>& assignments) {
    return ASTParser::try_parse(code).weights(assignments);
}

// setup with the trapdoor (alpha, beta, gamma, delta, x) given
inline Sigma setup_with(const Context& c, const QAP& qap, const std::array<FrLocal, 5>& trapdoor) {
    uint64_t td[20];
    for (int k = 0; k < 5; ++k)
        for (int l = 0; l < 4; ++l) td[4 * k + l] = trapdoor[k].w[l];
    zk_crs* s = nullptr;
    c.check(zk_setup(c.get(), qap.get(), td, &s), "groth16::setup");
    return Sigma(s);
}
// groth16::setup(&qap) (mod.rs:134-197): five non-zero random draws (mod.rs:139-145)
inline Sigma setup(const Context& c, const QAP& qap) {
    std::array<FrLocal, 5> td;
    for (auto& t : td) do { t = FrLocal::random_elem(); } while (t == FrLocal(0));
    return setup_with(c, qap, td);
}

// What a ceremony starts from instead of setup (zk_crs_from_powers): the QAP's CRS derived from a powers-of-tau transcript by group
// operations only, with gamma = delta = 1 -- the CRS setup_with(c, qap, {alpha, beta, 1, 1, x}) makes, for an (alpha, beta, x) nobody
// has to know.  QAP::from_sparse (rows over the roots 1..n); QAP::from, from_dense and from_root_rep throw ZK_ERR_UNSUPPORTED.  The transcript is NOT checked to
// be a sequence of powers: check_setup(c, qap, sigma) on the result, then one contribute per party, each checked by check_contribution.
inline Sigma setup_from_powers(const Context& c, const QAP& qap, const PowersOfTau& p) {
    if (p.tau_g1.size() % ZK_G1_WORDS || p.tau_g2.size() % ZK_G2_WORDS || p.alpha_tau_g1.size() * 2 != p.tau_g2.size() ||
        p.beta_tau_g1.size() * 2 != p.tau_g2.size())
        throw Error(ZK_ERR_ARG, "groth16::setup_from_powers: tau_g2, alpha_tau_g1 and beta_tau_g1 must hold the same number of whole points");
    zk_powers_desc d{p.tau_g1.size() / ZK_G1_WORDS, p.tau_g2.size() / ZK_G2_WORDS, p.tau_g1.data(), p.tau_g2.data(), p.alpha_tau_g1.data(),
                     p.beta_tau_g1.data(), p.beta_g2.data()};
    zk_crs* s = nullptr;
    c.check(zk_crs_from_powers(c.get(), qap.get(), &d, &s), "groth16::setup_from_powers");
    return Sigma(s);
}

// prove with the blinding scalars given
inline Proof prove_with(const Context& c, const QAP& qap, const Sigma& sigma, const std::vector<FrLocal>& weights_, const FrLocal& r, const FrLocal& s) {
    Proof p;
    c.check(zk_prove(c.get(), sigma.get(), qap.get(), weights_.empty() ? nullptr : weights_[0].w.data(), weights_.size(), r.w.data(), s.w.data(), p.bytes.data()),
            "groth16::prove");
    return p;
}
// groth16::prove(&qap, (&sigma_g1, &sigma_g2), &weights) (mod.rs:213-296): r, s drawn inside (mod.rs:231)
inline Proof prove(const Context& c, const QAP& qap, const Sigma& sigma, const std::vector<FrLocal>& weights_) {
    return prove_with(c, qap, sigma, weights_, FrLocal::random_elem(), FrLocal::random_elem());
}

// What the reference lacks (prove drops the remainder of (U V - W) / t, mod.rs:277): the witness against the QAP on the GPU, before a
// proof is spent on it (zk_qap_check).  Sparse QAP forms (QAP::from_sparse, QAP::from_root_rep); the dense form throws ZK_ERR_UNSUPPORTED.
inline zk_qap_check_result check(const Context& c, const QAP& qap, const std::vector<FrLocal>& weights_) {
    zk_qap_check_result r{};
    c.check(zk_qap_check(c.get(), qap.get(), weights_.empty() ? nullptr : weights_[0].w.data(), weights_.size(), &r), "groth16::is_satisfied");
    return r;
}
// true iff prove(c, qap, sigma, weights) yields a proof that verify accepts: every gate holds and weights[0] == 1
inline bool is_satisfied(const Context& c, const QAP& qap, const std::vector<FrLocal>& weights_) {
    const zk_qap_check_result r = check(c, qap, weights_);
    return r.bad_gates == 0 && r.flags == 0;
}
// the lowest gate (0-based row of the root representation) with U_j V_j != W_j; nullopt when every gate holds
inline std::optional<size_t> which_is_unsatisfied(const Context& c, const QAP& qap, const std::vector<FrLocal>& weights_) {
    const zk_qap_check_result r = check(c, qap, weights_);
    return r.first_bad == ZK_QAP_CHECK_NONE ? std::nullopt : std::optional<size_t>(r.first_bad);
}

// What the reference lacks as well: is `sigma` a CRS of SOME trapdoor for this QAP (zk_crs_check)?  What a prover that did not run
// setup itself asks once about the CRS it was handed (a ceremony, a file, another machine).  The challenge is drawn from the OS
// inside the library; check_setup_with fixes it and is for tests -- whoever made the CRS must not be able to predict it.
struct SetupCheck {
    uint32_t failed = 0;   // ZK_CRS_CHECK_GENERATORS .. ZK_CRS_CHECK_DEGENERATE: the relations that do not hold
    uint32_t flags = 0;    // ZK_CRS_CHECK_T_ZERO | ZK_CRS_CHECK_LAGRANGE_PRESENT
    bool ok() const { return failed == 0 && !(flags & ZK_CRS_CHECK_T_ZERO); }
    bool has(uint32_t bit) const { return (failed & bit) != 0; }
};
inline SetupCheck check_setup_with(const Context& c, const QAP& qap, const Sigma& sigma, const FrLocal& challenge) {
    zk_crs_check_result r{};
    c.check(zk_crs_check(c.get(), sigma.get(), qap.get(), challenge.w.data(), &r), "groth16::check_setup");
    return SetupCheck{r.failed, r.flags};
}
inline SetupCheck check_setup(const Context& c, const QAP& qap, const Sigma& sigma) {
    zk_crs_check_result r{};
    c.check(zk_crs_check(c.get(), sigma.get(), qap.get(), nullptr, &r), "groth16::check_setup");
    return SetupCheck{r.failed, r.flags};
}

// Re-keying delta (zk_crs_contribute): what a party does to a CRS it was handed so that whoever ran setup no longer knows its
// trapdoor.  contribute draws the factor d from the OS inside the library (it is wiped and never returned); contribute_with fixes
// it and is for tests.  The Contribution proves knowledge of d for a 32-byte tag of the caller's (the hash of the transcript so
// far); its 224 bytes are its byte form.  check_contribution: is `after` the CRS `before` with only delta re-keyed by whoever made
// the record (zk_crs_contribution_check)?  `after` is then as good a CRS as `before` is (check_setup, once, for a chain's head).
struct Contribution {
    zk_crs_contribution raw{};
    // zk_crs_contribution_verify: host code, no context
    bool verify(const Tag& tag) const {
        int ok = 0;
        const int st = zk_crs_contribution_verify(&raw, tag.data(), &ok);
        if (st != ZK_OK) throw Error(st, "Contribution::verify");
        return ok != 0;
    }
    std::array<uint8_t, sizeof(zk_crs_contribution)> to_bytes() const {
        std::array<uint8_t, sizeof(zk_crs_contribution)> b;
        std::memcpy(b.data(), &raw, b.size());
        return b;
    }
    static Contribution from_bytes(const std::array<uint8_t, sizeof(zk_crs_contribution)>& b) {
        Contribution c;
        std::memcpy(&c.raw, b.data(), b.size());
        return c;
    }
};
struct ContributionCheck {
    uint32_t failed = 0;   // ZK_CONTRIB_UNCHANGED .. ZK_CONTRIB_DEGENERATE: the relations that do not hold
    bool ok() const { return failed == 0; }
    bool has(uint32_t bit) const { return (failed & bit) != 0; }
};
inline std::pair<Sigma, Contribution> contribute_with(const Context& c, const Sigma& sigma, const FrLocal& d, const Tag& tag) {
    zk_crs* s = nullptr;
    Contribution rec;
    c.check(zk_crs_contribute(c.get(), sigma.get(), d.w.data(), tag.data(), &s, &rec.raw), "groth16::contribute");
    return {Sigma(s), rec};
}
inline std::pair<Sigma, Contribution> contribute(const Context& c, const Sigma& sigma, const Tag& tag) {
    zk_crs* s = nullptr;
    Contribution rec;
    c.check(zk_crs_contribute(c.get(), sigma.get(), nullptr, tag.data(), &s, &rec.raw), "groth16::contribute");
    return {Sigma(s), rec};
}
inline ContributionCheck check_contribution_with(const Context& c, const Sigma& before, const Sigma& after, const Contribution& rec, const Tag& tag,
                                                 const FrLocal& challenge) {
    zk_crs_contribution_result r{};
    c.check(zk_crs_contribution_check(c.get(), before.get(), after.get(), &rec.raw, tag.data(), challenge.w.data(), &r), "groth16::check_contribution");
    return ContributionCheck{r.failed};
}
inline ContributionCheck check_contribution(const Context& c, const Sigma& before, const Sigma& after, const Contribution& rec, const Tag& tag) {
    zk_crs_contribution_result r{};
    c.check(zk_crs_contribution_check(c.get(), before.get(), after.get(), &rec.raw, tag.data(), nullptr, &r), "groth16::check_contribution");
    return ContributionCheck{r.failed};
}

// Phase 1 (zk_powers_*): the transcript itself, resident on the device.  check_powers: is it a powers-of-tau sequence over the
// library's generators (once per transcript, whatever the circuit)?  contribute_powers: the transcript of (alpha a, beta b, x s) for
// secrets drawn from the OS inside the library (wiped, never returned; contribute_powers_with fixes them, for tests) and the record
// that proves knowledge of them for a tag.  check_powers_contribution: is `after` a transcript, and `before` re-keyed by whoever made
// the record?  `before` is not checked again: a chain starts at ResidentPowers::initial or one check_powers.  download() gives the
// PowersOfTau that setup_from_powers takes.
struct PowersCheck {
    uint32_t failed = 0;   // ZK_POWERS_CHECK_GENERATORS .. ZK_POWERS_CHECK_KNOWLEDGE: the relations that do not hold
    bool ok() const { return failed == 0; }
    bool has(uint32_t bit) const { return (failed & bit) != 0; }
};
using PowersContributionCheck = PowersCheck;
struct PowersContribution {
    zk_powers_contribution raw{};
    bool verify(const Tag& tag) const {   // zk_powers_contribution_verify: host code, no context
        int ok = 0;
        const int st = zk_powers_contribution_verify(&raw, tag.data(), &ok);
        if (st != ZK_OK) throw Error(st, "PowersContribution::verify");
        return ok != 0;
    }
};
class ResidentPowers {
   public:
    ResidentPowers(ResidentPowers&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    ResidentPowers(const ResidentPowers&) = delete;
    ~ResidentPowers() { if (p_) zk_powers_free(p_); }
    const zk_powers* get() const { return p_; }
    static ResidentPowers upload(const Context& c, const PowersOfTau& p) {
        if (p.tau_g1.size() % ZK_G1_WORDS || p.tau_g2.size() % ZK_G2_WORDS || p.alpha_tau_g1.size() * 2 != p.tau_g2.size() ||
            p.beta_tau_g1.size() * 2 != p.tau_g2.size())
            throw Error(ZK_ERR_ARG, "ResidentPowers::upload: tau_g2, alpha_tau_g1 and beta_tau_g1 must hold the same number of whole points");
        zk_powers_desc d{p.tau_g1.size() / ZK_G1_WORDS, p.tau_g2.size() / ZK_G2_WORDS, p.tau_g1.data(), p.tau_g2.data(), p.alpha_tau_g1.data(),
                         p.beta_tau_g1.data(), p.beta_g2.data()};
        zk_powers* h = nullptr;
        c.check(zk_powers_upload(c.get(), &d, &h), "ResidentPowers::upload");
        return ResidentPowers(h);
    }
    static ResidentPowers initial(const Context& c, size_t n_tau_g1, size_t n_rest) {
        zk_powers* h = nullptr;
        c.check(zk_powers_initial(c.get(), n_tau_g1, n_rest, &h), "ResidentPowers::initial");
        return ResidentPowers(h);
    }
    std::pair<size_t, size_t> dims() const {
        size_t n1 = 0, n2 = 0;
        zk_powers_dims(p_, &n1, &n2);
        return {n1, n2};
    }
    PowersOfTau download(const Context& c) const {
        const auto d = dims();
        PowersOfTau p;
        p.tau_g1.resize(d.first * ZK_G1_WORDS); p.tau_g2.resize(d.second * ZK_G2_WORDS);
        p.alpha_tau_g1.resize(d.second * ZK_G1_WORDS); p.beta_tau_g1.resize(d.second * ZK_G1_WORDS);
        const zk_powers_out o{p.tau_g1.data(), p.tau_g2.data(), p.alpha_tau_g1.data(), p.beta_tau_g1.data(), p.beta_g2.data()};
        c.check(zk_powers_download(c.get(), p_, &o), "ResidentPowers::download");
        return p;
    }

   private:
    friend std::pair<ResidentPowers, PowersContribution> contribute_powers_with(const Context&, const ResidentPowers&, const std::array<FrLocal, 3>&, const Tag&);
    friend std::pair<ResidentPowers, PowersContribution> contribute_powers(const Context&, const ResidentPowers&, const Tag&);
    explicit ResidentPowers(zk_powers* p) : p_(p) {}
    zk_powers* p_;
};
inline PowersCheck check_powers_with(const Context& c, const ResidentPowers& p, const FrLocal& challenge) {
    zk_powers_check_result r{};
    c.check(zk_powers_check(c.get(), p.get(), challenge.w.data(), &r), "groth16::check_powers");
    return PowersCheck{r.failed};
}
inline PowersCheck check_powers(const Context& c, const ResidentPowers& p) {
    zk_powers_check_result r{};
    c.check(zk_powers_check(c.get(), p.get(), nullptr, &r), "groth16::check_powers");
    return PowersCheck{r.failed};
}
inline std::pair<ResidentPowers, PowersContribution> contribute_powers_with(const Context& c, const ResidentPowers& p, const std::array<FrLocal, 3>& sab,
                                                                            const Tag& tag) {
    uint64_t sec[12];
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < 4; ++l) sec[4 * k + l] = sab[k].w[l];
    zk_powers* h = nullptr;
    PowersContribution rec;
    c.check(zk_powers_contribute(c.get(), p.get(), sec, tag.data(), &h, &rec.raw), "groth16::contribute_powers");
    return {ResidentPowers(h), rec};
}
inline std::pair<ResidentPowers, PowersContribution> contribute_powers(const Context& c, const ResidentPowers& p, const Tag& tag) {
    zk_powers* h = nullptr;
    PowersContribution rec;
    c.check(zk_powers_contribute(c.get(), p.get(), nullptr, tag.data(), &h, &rec.raw), "groth16::contribute_powers");
    return {ResidentPowers(h), rec};
}
inline PowersContributionCheck check_powers_contribution_with(const Context& c, const ResidentPowers& before, const ResidentPowers& after,
                                                              const PowersContribution& rec, const Tag& tag, const FrLocal& challenge) {
    zk_powers_check_result r{};
    c.check(zk_powers_contribution_check(c.get(), before.get(), after.get(), &rec.raw, tag.data(), challenge.w.data(), &r), "groth16::check_powers_contribution");
    return PowersCheck{r.failed};
}
inline PowersContributionCheck check_powers_contribution(const Context& c, const ResidentPowers& before, const ResidentPowers& after,
                                                         const PowersContribution& rec, const Tag& tag) {
    zk_powers_check_result r{};
    c.check(zk_powers_contribution_check(c.get(), before.get(), after.get(), &rec.raw, tag.data(), nullptr, &r), "groth16::check_powers_contribution");
    return PowersCheck{r.failed};
}

// groth16::verify((sigma_g1, sigma_g2), &inputs, proof) (mod.rs:299-320)
inline bool verify(const Context& c, const Sigma& sigma, const std::vector<FrLocal>& inputs, const Proof& proof) {
    int ok = 0;
    c.check(zk_verify(c.get(), sigma.get(), inputs.empty() ? nullptr : inputs[0].w.data(), inputs.size(), proof.bytes.data(), &ok), "groth16::verify");
    return ok != 0;
}

// verify for many proofs over one CRS on the GPU (zk_verify_batch): entry j == verify(c, sigma, inputs[j], proofs[j]); every
// inputs[j] has the same length
inline std::vector<bool> verify_batch(const Context& c, const Sigma& sigma, const std::vector<std::vector<FrLocal>>& inputs,
                                      const std::vector<Proof>& proofs) {
    if (inputs.size() != proofs.size()) throw Error(ZK_ERR_ARG, "groth16::verify_batch: one input row per proof");
    const size_t n = proofs.size(), k = n ? inputs[0].size() : 0;
    std::vector<uint64_t> x(n * k * 4);
    std::vector<uint8_t> bytes(n * ZK_PROOF_BYTES);
    for (size_t j = 0; j < n; ++j) {
        if (inputs[j].size() != k) throw Error(ZK_ERR_ARG, "groth16::verify_batch: every proof needs the same number of inputs");
        for (size_t i = 0; i < k; ++i) std::copy(inputs[j][i].w.begin(), inputs[j][i].w.end(), x.begin() + (j * k + i) * 4);
        std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_BYTES);
    }
    std::vector<int> ok(n, 0);
    c.check(zk_verify_batch(c.get(), sigma.get(), k ? x.data() : nullptr, k, bytes.data(), n, ok.data()), "groth16::verify_batch");
    return std::vector<bool>(ok.begin(), ok.end());
}

// verify_batch over compressed proofs, decompressed on the GPU (zk_verify_batch_compressed): entry j is true iff proofs[j]
// decompresses and verify accepts the result
inline std::vector<bool> verify_batch_compressed(const Context& c, const Sigma& sigma, const std::vector<std::vector<FrLocal>>& inputs,
                                                 const std::vector<CompressedProof>& proofs) {
    if (inputs.size() != proofs.size()) throw Error(ZK_ERR_ARG, "groth16::verify_batch_compressed: one input row per proof");
    const size_t n = proofs.size(), k = n ? inputs[0].size() : 0;
    std::vector<uint64_t> x(n * k * 4);
    std::vector<uint8_t> bytes(n * ZK_PROOF_COMPRESSED_BYTES);
    for (size_t j = 0; j < n; ++j) {
        if (inputs[j].size() != k) throw Error(ZK_ERR_ARG, "groth16::verify_batch_compressed: every proof needs the same number of inputs");
        for (size_t i = 0; i < k; ++i) std::copy(inputs[j][i].w.begin(), inputs[j][i].w.end(), x.begin() + (j * k + i) * 4);
        std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_COMPRESSED_BYTES);
    }
    std::vector<int> ok(n, 0);
    c.check(zk_verify_batch_compressed(c.get(), sigma.get(), k ? x.data() : nullptr, k, bytes.data(), n, ok.data()),
            "groth16::verify_batch_compressed");
    return std::vector<bool>(ok.begin(), ok.end());
}

// one verdict for many proofs over one CRS on the GPU (zk_verify_batch_all): true iff every proof decodes and the random linear
// combination of their pairing equations with the multipliers z (z[j] = {low, high} words of a non-zero 128-bit integer) holds
inline bool verify_batch_all_with(const Context& c, const Sigma& sigma, const std::vector<std::vector<FrLocal>>& inputs,
                                  const std::vector<Proof>& proofs, const std::vector<std::array<uint64_t, 2>>& z) {
    if (inputs.size() != proofs.size() || z.size() != proofs.size())
        throw Error(ZK_ERR_ARG, "groth16::verify_batch_all: one input row and one multiplier per proof");
    const size_t n = proofs.size(), k = n ? inputs[0].size() : 0;
    // one spare element each: proofs and z must not be null even for an empty batch
    std::vector<uint64_t> x(n * k * 4), zw(2 * n + 2);
    std::vector<uint8_t> bytes(n * ZK_PROOF_BYTES + 1);
    for (size_t j = 0; j < n; ++j) {
        if (inputs[j].size() != k) throw Error(ZK_ERR_ARG, "groth16::verify_batch_all: every proof needs the same number of inputs");
        for (size_t i = 0; i < k; ++i) std::copy(inputs[j][i].w.begin(), inputs[j][i].w.end(), x.begin() + (j * k + i) * 4);
        std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_BYTES);
        zw[2 * j] = z[j][0];
        zw[2 * j + 1] = z[j][1];
    }
    int ok = 0;
    c.check(zk_verify_batch_all(c.get(), sigma.get(), k ? x.data() : nullptr, k, bytes.data(), n, zw.data(), &ok),
            "groth16::verify_batch_all");
    return ok != 0;
}
// the same with z drawn from std::random_device (secret to whoever made the proofs); a batch with a bad proof passes with
// probability at most 1 / (2^128 - 1)
inline bool verify_batch_all(const Context& c, const Sigma& sigma, const std::vector<std::vector<FrLocal>>& inputs,
                             const std::vector<Proof>& proofs) {
    static thread_local std::random_device rd;
    std::vector<std::array<uint64_t, 2>> z(proofs.size());
    for (auto& zj : z)
        do {
            for (auto& w : zj) w = ((uint64_t)rd() << 32) | rd();
        } while (!(zj[0] | zj[1]));
    return verify_batch_all_with(c, sigma, inputs, proofs, z);
}

// The verifying key (zk_vk): alpha, beta, gamma, delta and sum_gamma[0..l], all groth16::verify reads of (SigmaG1, SigmaG2).
// Host data: from_points / from_bytes / load / to_bytes / save / verify need no Context and no GPU.  The batch calls take a
// Context; the first one binds the key to it (a later call with another Context throws ZK_ERR_ARG).  Key and Context may be
// destroyed in either order.
class VerifyingKey {
   public:
    VerifyingKey(VerifyingKey&& o) noexcept : k_(std::exchange(o.k_, nullptr)) {}
    VerifyingKey(const VerifyingKey&) = delete;
    ~VerifyingKey() { zk_vk_free(k_); }
    zk_vk* get() const { return k_; }
    // points as canonical little-endian words: 8, 16, 16, 16 and (l + 1) x 8
    static VerifyingKey from_points(const std::vector<uint64_t>& alpha_g1, const std::vector<uint64_t>& beta_g2, const std::vector<uint64_t>& gamma_g2,
                                    const std::vector<uint64_t>& delta_g2, const std::vector<uint64_t>& sum_gamma_g1) {
        if (alpha_g1.size() != 8 || beta_g2.size() != 16 || gamma_g2.size() != 16 || delta_g2.size() != 16 || sum_gamma_g1.size() < 8 ||
            sum_gamma_g1.size() % 8)
            throw Error(ZK_ERR_ARG, "VerifyingKey::from_points: 8, 16, 16, 16 and (l + 1) x 8 words");
        const zk_vk_desc d{sum_gamma_g1.size() / 8 - 1, alpha_g1.data(), beta_g2.data(), gamma_g2.data(), delta_g2.data(), sum_gamma_g1.data()};
        zk_vk* k = nullptr;
        host(zk_vk_create(&d, &k), "VerifyingKey::from_points");
        return VerifyingKey(k);
    }
    static VerifyingKey from_sigma(const Context& c, const Sigma& sigma) {
        zk_vk* k = nullptr;
        c.check(zk_vk_from_crs(c.get(), sigma.get(), &k), "VerifyingKey::from_sigma");
        return VerifyingKey(k);
    }
    static VerifyingKey from_bytes(const std::vector<uint8_t>& b) {
        zk_vk* k = nullptr;
        const uint8_t none = 0;
        host(zk_vk_from_bytes(b.empty() ? &none : b.data(), b.size(), &k), "VerifyingKey::from_bytes");
        return VerifyingKey(k);
    }
    static VerifyingKey load(const std::string& path) {
        zk_vk* k = nullptr;
        host(zk_vk_load(path.c_str(), &k), "VerifyingKey::load");
        return VerifyingKey(k);
    }
    size_t input() const {
        size_t l = 0;
        host(zk_vk_dims(k_, &l), "VerifyingKey::input");
        return l;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> b(zk_vk_bytes(input()));
        host(zk_vk_to_bytes(k_, b.data(), b.size()), "VerifyingKey::to_bytes");
        return b;
    }
    void save(const std::string& path) const { host(zk_vk_save(k_, path.c_str()), "VerifyingKey::save"); }
    // groth16::verify on the host: the verdict of verify(c, sigma, inputs, proof)
    bool verify(const std::vector<FrLocal>& inputs, const Proof& proof) const {
        int ok = 0;
        host(zk_vk_verify(k_, inputs.empty() ? nullptr : inputs[0].w.data(), inputs.size(), proof.bytes.data(), &ok), "VerifyingKey::verify");
        return ok != 0;
    }
    // the batch calls of groth16:: with the key in the place of sigma
    std::vector<bool> verify_batch(const Context& c, const std::vector<std::vector<FrLocal>>& inputs, const std::vector<Proof>& proofs) const {
        std::vector<uint64_t> x;
        const size_t k = pack(inputs, proofs.size(), x, "VerifyingKey::verify_batch");
        std::vector<uint8_t> bytes(proofs.size() * ZK_PROOF_BYTES + 1);
        for (size_t j = 0; j < proofs.size(); ++j) std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_BYTES);
        std::vector<int> ok(proofs.size(), 0);
        c.check(zk_vk_verify_batch(c.get(), k_, k ? x.data() : nullptr, k, bytes.data(), proofs.size(), ok.data()), "VerifyingKey::verify_batch");
        return std::vector<bool>(ok.begin(), ok.end());
    }
    std::vector<bool> verify_batch_compressed(const Context& c, const std::vector<std::vector<FrLocal>>& inputs,
                                              const std::vector<CompressedProof>& proofs) const {
        std::vector<uint64_t> x;
        const size_t k = pack(inputs, proofs.size(), x, "VerifyingKey::verify_batch_compressed");
        std::vector<uint8_t> bytes(proofs.size() * ZK_PROOF_COMPRESSED_BYTES + 1);
        for (size_t j = 0; j < proofs.size(); ++j)
            std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_COMPRESSED_BYTES);
        std::vector<int> ok(proofs.size(), 0);
        c.check(zk_vk_verify_batch_compressed(c.get(), k_, k ? x.data() : nullptr, k, bytes.data(), proofs.size(), ok.data()),
                "VerifyingKey::verify_batch_compressed");
        return std::vector<bool>(ok.begin(), ok.end());
    }
    bool verify_batch_all_with(const Context& c, const std::vector<std::vector<FrLocal>>& inputs, const std::vector<Proof>& proofs,
                               const std::vector<std::array<uint64_t, 2>>& z) const {
        if (z.size() != proofs.size()) throw Error(ZK_ERR_ARG, "VerifyingKey::verify_batch_all: one multiplier per proof");
        std::vector<uint64_t> x, zw(2 * proofs.size() + 2);
        const size_t k = pack(inputs, proofs.size(), x, "VerifyingKey::verify_batch_all");
        std::vector<uint8_t> bytes(proofs.size() * ZK_PROOF_BYTES + 1);
        for (size_t j = 0; j < proofs.size(); ++j) {
            std::copy(proofs[j].bytes.begin(), proofs[j].bytes.end(), bytes.begin() + j * ZK_PROOF_BYTES);
            zw[2 * j] = z[j][0];
            zw[2 * j + 1] = z[j][1];
        }
        int ok = 0;
        c.check(zk_vk_verify_batch_all(c.get(), k_, k ? x.data() : nullptr, k, bytes.data(), proofs.size(), zw.data(), &ok),
                "VerifyingKey::verify_batch_all");
        return ok != 0;
    }
    bool verify_batch_all(const Context& c, const std::vector<std::vector<FrLocal>>& inputs, const std::vector<Proof>& proofs) const {
        static thread_local std::random_device rd;
        std::vector<std::array<uint64_t, 2>> z(proofs.size());
        for (auto& zj : z)
            do {
                for (auto& w : zj) w = ((uint64_t)rd() << 32) | rd();
            } while (!(zj[0] | zj[1]));
        return verify_batch_all_with(c, inputs, proofs, z);
    }
    // S_j = sum_gamma_0 + sum_i inputs[j][i] sum_gamma_i as 8 canonical words per row (zk_vk_input_sums); tables = false runs
    // verify_batch's bit-serial kernel, true the key's window tables: the same words
    std::vector<uint64_t> input_sums(const Context& c, const std::vector<std::vector<FrLocal>>& inputs, bool tables = true) const {
        std::vector<uint64_t> x, out(inputs.size() * 8);
        const size_t k = pack(inputs, inputs.size(), x, "VerifyingKey::input_sums");
        c.check(zk_vk_input_sums(c.get(), k_, k ? x.data() : nullptr, k, inputs.size(), tables ? 1 : 0, out.data()), "VerifyingKey::input_sums");
        return out;
    }

   private:
    explicit VerifyingKey(zk_vk* k) : k_(k) {}
    static void host(int st, const char* where) {
        if (st != ZK_OK) throw Error(st, where);
    }
    static size_t pack(const std::vector<std::vector<FrLocal>>& inputs, size_t n, std::vector<uint64_t>& x, const char* where) {
        if (inputs.size() != n) throw Error(ZK_ERR_ARG, std::string(where) + ": one input row per proof");
        const size_t k = n ? inputs[0].size() : 0;
        x.assign(n * k * 4, 0);
        for (size_t j = 0; j < n; ++j) {
            if (inputs[j].size() != k) throw Error(ZK_ERR_ARG, std::string(where) + ": every proof needs the same number of inputs");
            for (size_t i = 0; i < k; ++i) std::copy(inputs[j][i].w.begin(), inputs[j][i].w.end(), x.begin() + (j * k + i) * 4);
        }
        return k;
    }
    zk_vk* k_;
};

}  // namespace groth16
}  // namespace zksnark
