// builder.hip -- zk_builder_*: the C ABI over builder.hpp, zk_poseidon_hash / zk_poseidon_params over poseidon.hpp and zk_babyjub_params /
// _on_curve / _add / _mul over babyjub.hpp and zk_eddsa_challenge / _public_key / _sign / _verify over eddsa.hpp (host code only; no
// context, no device).
#include "builder.hpp"

namespace zk {

template <class Fn>
static int builder_guard(zk_builder* b, Fn&& fn) {
    if (!b) return ZK_ERR_ARG;
    try {
        BuilderOps ops{*b};
        ops.live();
        fn(ops);
        return ZK_OK;
    } catch (const ParseError& e) { b->last_error = e.msg; return e.status; }
    catch (const std::exception& e) { b->last_error = e.what(); return ZK_ERR_ARG; }
    catch (...) { b->last_error = "unknown error"; return ZK_ERR_ARG; }
}

}  // namespace zk

using namespace zk;

extern "C" {

int zk_builder_create(zk_builder** out) {
    if (!out) return ZK_ERR_ARG;
    *out = nullptr;
    try { *out = new zk_builder(); } catch (...) { return ZK_ERR_ARG; }
    return ZK_OK;
}
void zk_builder_free(zk_builder* b) { delete b; }
const char* zk_builder_last_error(const zk_builder* b) { return b ? b->last_error.c_str() : "null builder"; }
int zk_builder_dims(const zk_builder* b, size_t* wires, size_t* gates) {
    if (!b) return ZK_ERR_ARG;
    return builder_guard(const_cast<zk_builder*>(b), [&](BuilderOps& o) {
        if (wires) *wires = o.b.kind.size();
        if (gates) *gates = o.b.subs.size();
    });
}
int zk_builder_new_wires(zk_builder* b, int kind, size_t count, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (kind != ZK_WIRE_BIT && kind != ZK_WIRE_FIELD) BuilderOps::fail("unknown wire kind " + std::to_string(kind));
        if (count && !out) BuilderOps::fail("null output array");
        for (size_t i = 0; i < count; ++i) out[i] = o.new_wire(kind == ZK_WIRE_BIT ? 1 : 2);
    });
}
int zk_builder_sub_circuit(zk_builder* b, const uint64_t* left_weights, const uint32_t* left_wires, size_t nl, const uint64_t* right_weights,
                           const uint32_t* right_wires, size_t nr, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out || (nl && (!left_weights || !left_wires)) || (nr && (!right_weights || !right_wires))) BuilderOps::fail("null array");
        *out = o.general(left_weights, left_wires, nl, right_weights, right_wires, nr);
    });
}
int zk_builder_gate(zk_builder* b, int kind, uint32_t x, uint32_t y, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out) BuilderOps::fail("null output");
        o.known(x);
        if (!BuilderOps::unary(kind)) o.known(y);
        *out = o.gate(kind, x, y);
    });
}
int zk_builder_bitwise(zk_builder* b, int kind, const uint32_t* x, const uint32_t* y, size_t n, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        const bool un = BuilderOps::unary(kind);
        if (kind < ZK_GATE_BIT_CHECK || kind > ZK_GATE_GREATER) BuilderOps::fail("unknown gate kind " + std::to_string(kind));
        if (n && (!x || !out || (!un && !y))) BuilderOps::fail("null array");
        for (size_t i = 0; i < n; ++i) { o.known(x[i]); if (!un) o.known(y[i]); }
        for (size_t i = 0; i < n; ++i) {
            const uint32_t r = o.gate(kind, x[i], un ? 0 : y[i]);   // out may alias x or y
            out[i] = r;
        }
    });
}
int zk_builder_fan_in(zk_builder* b, int kind, const uint32_t* x, size_t n, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (kind < ZK_GATE_BIT_CHECK || kind > ZK_GATE_GREATER || BuilderOps::unary(kind)) BuilderOps::fail("fan_in takes a two-input gate kind");
        if (!n || !x || !out) BuilderOps::fail("fan_in: the input must have at least one element");
        for (size_t i = 0; i < n; ++i) o.known(x[i]);
        uint32_t acc = x[0];
        for (size_t i = 1; i < n; ++i) acc = o.gate(kind, acc, x[i]);
        *out = acc;
    });
}
int zk_builder_compare(zk_builder* b, int kind, const uint32_t* left, const uint32_t* right, size_t n_bits, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (kind < ZK_CMP_EQUAL || kind > ZK_CMP_GREATER_EQ) BuilderOps::fail("unknown comparator " + std::to_string(kind));
        const bool one_sided = kind == ZK_CMP_EQUAL_ZERO;
        if (!n_bits || !left || !out || (!one_sided && !right)) BuilderOps::fail("comparator: the inputs must have at least one wire");
        for (size_t i = 0; i < n_bits; ++i) { o.known(left[i]); if (!one_sided) o.known(right[i]); }
        *out = o.compare(kind, left, right, n_bits);
    });
}
int zk_builder_keccak(zk_builder* b, const uint32_t* in_wires, size_t n_bytes, unsigned rate_bytes, unsigned delim, unsigned rounds,
                      uint32_t* out_wires, size_t out_bytes) {
    return builder_guard(b, [&](BuilderOps& o) {
        if ((n_bytes && !in_wires) || (out_bytes && !out_wires)) BuilderOps::fail("null array");
        o.keccak(in_wires, n_bytes, rate_bytes, delim, rounds, out_wires, out_bytes);
    });
}
int zk_builder_assert_bit(zk_builder* b, uint32_t wire) {
    return builder_guard(b, [&](BuilderOps& o) {
        o.known(wire);
        o.assert_bit(wire);
    });
}
int zk_builder_pack(zk_builder* b, const uint32_t* bits, size_t n_bits, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out || (n_bits && !bits)) BuilderOps::fail("null array");
        *out = o.pack(bits, n_bits);
    });
}
int zk_builder_poseidon(zk_builder* b, const uint32_t* in_wires, size_t arity, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out || (arity && !in_wires)) BuilderOps::fail("null array");
        *out = o.poseidon(in_wires, arity);
    });
}
int zk_builder_merkle_root(zk_builder* b, uint32_t leaf, const uint32_t* siblings, const uint32_t* dirs, size_t depth, uint32_t* out) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out || (depth && (!siblings || !dirs))) BuilderOps::fail("null array");
        *out = o.merkle_root(leaf, siblings, dirs, depth);
    });
}
int zk_builder_babyjub_assert_on_curve(zk_builder* b, const uint32_t xy[2]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!xy) BuilderOps::fail("null array");
        o.known(xy[0]); o.known(xy[1]);
        o.babyjub_assert_on_curve(xy[0], xy[1]);
    });
}
int zk_builder_babyjub_add(zk_builder* b, const uint32_t p[3], const uint32_t q[3], uint32_t out[3]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!p || !q || !out) BuilderOps::fail("null array");
        o.babyjub_add(p, q, out);
    });
}
int zk_builder_babyjub_mul_fixed(zk_builder* b, const uint32_t* bits, size_t n_bits, uint32_t out[3]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!out || (n_bits && !bits)) BuilderOps::fail("null array");
        o.babyjub_mul_fixed(bits, n_bits, out);
    });
}
int zk_builder_babyjub_mul(zk_builder* b, const uint32_t p_xy[2], const uint32_t* bits, size_t n_bits, uint32_t out[3]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!p_xy || !out || (n_bits && !bits)) BuilderOps::fail("null array");
        o.babyjub_mul(p_xy, bits, n_bits, out);
    });
}
int zk_builder_babyjub_affine(zk_builder* b, const uint32_t p[3], const uint32_t xy[2]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!p || !xy) BuilderOps::fail("null array");
        o.babyjub_affine(p, xy);
    });
}
int zk_builder_eddsa_verify(zk_builder* b, const uint32_t a_xy[2], const uint32_t r8_xy[2], uint32_t msg, const uint32_t s_bits[251],
                            const uint32_t hm_bits[254]) {
    return builder_guard(b, [&](BuilderOps& o) {
        if (!a_xy || !r8_xy || !s_bits || !hm_bits) BuilderOps::fail("null array");
        o.eddsa_verify(a_xy, r8_xy, msg, s_bits, hm_bits);
    });
}
int zk_builder_finish(zk_builder* b, const uint32_t* verify_wires, size_t n_verify, zk_circuit** out) {
    if (!out) return ZK_ERR_ARG;
    *out = nullptr;
    return builder_guard(b, [&](BuilderOps& o) {
        if (n_verify && !verify_wires) BuilderOps::fail("null array");
        *out = builder_finish(o.b, verify_wires, n_verify);
    });
}

int zk_poseidon_hash(const uint64_t* inputs, size_t arity, uint64_t out[4]) {
    try { return poseidon_hash_words(inputs, arity, out); } catch (...) { return ZK_ERR_ARG; }
}
int zk_poseidon_params(size_t arity, unsigned* rf, unsigned* rp, uint64_t* round_constants, uint64_t* mds) {
    try { return poseidon_params_words(arity, rf, rp, round_constants, mds); } catch (...) { return ZK_ERR_ARG; }
}

int zk_babyjub_params(uint64_t a[4], uint64_t d[4], uint64_t order[4], uint64_t base8[8], uint64_t generator[8]) {
    return babyjub_params_words(a, d, order, base8, generator);
}
int zk_babyjub_on_curve(const uint64_t p[8]) { return babyjub_on_curve_words(p); }
int zk_babyjub_add(const uint64_t p[8], const uint64_t q[8], uint64_t out[8]) { return babyjub_add_words(p, q, out); }
int zk_babyjub_mul(const uint64_t scalar[4], const uint64_t* p, uint64_t out[8]) { return babyjub_mul_words(scalar, p, out); }

int zk_eddsa_challenge(const uint64_t r8[8], const uint64_t a[8], const uint64_t msg[4], uint64_t out[4]) {
    try { return eddsa_challenge_words(r8, a, msg, out); } catch (...) { return ZK_ERR_ARG; }
}
int zk_eddsa_public_key(const uint64_t k[4], uint64_t out[8]) { return eddsa_public_key_words(k, out); }
int zk_eddsa_sign(const uint64_t k[4], const uint64_t nonce_key[4], const uint64_t msg[4], uint64_t r8_out[8], uint64_t s_out[4]) {
    try { return eddsa_sign_words(k, nonce_key, msg, r8_out, s_out); } catch (...) { return ZK_ERR_ARG; }
}
int zk_eddsa_verify(const uint64_t a[8], const uint64_t msg[4], const uint64_t r8[8], const uint64_t s[4], int* status) {
    try { return eddsa_verify_words(a, msg, r8, s, status); } catch (...) { return ZK_ERR_ARG; }
}

}  // extern "C"
