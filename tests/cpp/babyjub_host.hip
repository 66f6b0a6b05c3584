// babyjub_host.hip -- Baby Jubjub's host code (csrc/babyjub.hpp: the constants, the projective formulas, the scalar multiple, the window
// table; the gadgets of csrc/builder.hpp; zk_builder_finish and the three host evaluators on what they emit) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_babyjub_host.py (hipcc --cuda-host-only -Xarch_host
// -fsanitize=address,undefined).  No device, no context.
// stdin: one line: a scalar k of 64 hex digits, then n_bits.  With s = k mod 2^n_bits, prints
//   "params A D L"                    a, d in decimal, l in hex
//   "mul X Y"                         [k] Base8
//   "mulgen X Y"                      [k] Generator
//   "add X Y"                         [k] Base8 + Generator
//   "fixed N X Y"                     zk_builder_babyjub_mul_fixed over n_bits bits: gates (with the 4 of _affine), the pinned affine wires
//   "var N X Y"                       zk_builder_babyjub_mul over Generator: gates (with _affine), the pinned affine wires
//   "refused R"                       refusals that came back with the right status out of those tried
#include "builder.hip"
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace zk;

static std::string hex(const uint64_t* w) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (int k = 3; k >= 0; --k)
        for (int i = 60; i >= 0; i -= 4) s += d[(w[k] >> i) & 15];
    return s;
}
static void parse(const std::string& s, uint64_t* w) {
    for (int k = 0; k < 4; ++k) w[3 - k] = std::stoull(s.substr(16 * k, 16), nullptr, 16);
}

struct Handles {
    zk_builder* b = nullptr;
    zk_circuit* c = nullptr;
    Handles() { if (zk_builder_create(&b) != ZK_OK) std::abort(); }
    ~Handles() { zk_builder_free(b); delete c; }
};

// the three evaluators on exact-size heap buffers; false where they differ
static bool evaluate(const zk_circuit& c, const std::vector<uint64_t>& inputs, const std::vector<uint8_t>& bits, const std::vector<uint64_t>& fields,
                     std::vector<uint64_t>& words) {
    const size_t m = c.u.size(), n_in = inputs.size() / 4;
    std::unique_ptr<uint64_t[]> in(new uint64_t[std::max<size_t>(inputs.size(), 1)]);
    std::copy(inputs.begin(), inputs.end(), in.get());
    std::unique_ptr<uint64_t[]> a(new uint64_t[4 * m]), b(new uint64_t[4 * m]), x(new uint64_t[4 * m]);
    built_weights(c, in.get(), n_in, a.get(), m);
    built_check_inputs(c.tape, in.get(), n_in);
    if (c.tape.status) return false;
    std::unique_ptr<Fr[]> vals(new Fr[c.tape.slots]);
    tape_run_host(c.tape, in.get(), vals.get(), b.get());
    std::unique_ptr<uint8_t[]> pb(new uint8_t[std::max<size_t>(bits.size(), 1)]);
    std::copy(bits.begin(), bits.end(), pb.get());
    std::unique_ptr<uint64_t[]> pf(new uint64_t[std::max<size_t>(fields.size(), 1)]);
    std::copy(fields.begin(), fields.end(), pf.get());
    mixed_run_host(c, pb.get(), bits.size(), pf.get(), fields.size() / 4, x.get(), m);
    words.assign(a.get(), a.get() + 4 * m);
    for (size_t i = 0; i < 4 * m; ++i)
        if (a[i] != b[i] || a[i] != x[i]) return false;
    return true;
}

int main() {
    std::string line, ks;
    std::getline(std::cin, line);
    std::istringstream is(line);
    size_t n_bits = 0;
    is >> ks >> n_bits;
    if (n_bits < 1 || n_bits > 256) return 1;
    std::unique_ptr<uint64_t[]> k(new uint64_t[4]), p(new uint64_t[8]), q(new uint64_t[8]), g(new uint64_t[8]), l(new uint64_t[4]);
    parse(ks, k.get());
    {
        uint64_t a[4], d[4];
        if (zk_babyjub_params(a, d, l.get(), nullptr, g.get()) != ZK_OK) return 1;
        std::cout << "params " << a[0] << " " << d[0] << " " << hex(l.get()) << "\n";
    }
    if (zk_babyjub_mul(k.get(), nullptr, p.get()) != ZK_OK || zk_babyjub_on_curve(p.get()) != 1) return 2;
    std::cout << "mul " << hex(p.get()) << " " << hex(p.get() + 4) << "\n";
    if (zk_babyjub_mul(k.get(), g.get(), q.get()) != ZK_OK) return 2;
    std::cout << "mulgen " << hex(q.get()) << " " << hex(q.get() + 4) << "\n";
    if (zk_babyjub_add(p.get(), g.get(), q.get()) != ZK_OK) return 2;
    std::cout << "add " << hex(q.get()) << " " << hex(q.get() + 4) << "\n";

    // s = k mod 2^n_bits, its bits as inputs and packed
    std::vector<uint64_t> s(k.get(), k.get() + 4), bit_inputs;
    for (size_t i = n_bits; i < 256; ++i) s[i / 64] &= ~(1ull << (i % 64));
    std::vector<uint8_t> packed((n_bits + 7) / 8, 0);
    for (size_t i = 0; i < n_bits; ++i) {
        const uint64_t b = (s[i / 64] >> (i % 64)) & 1;
        bit_inputs.push_back(b);
        bit_inputs.insert(bit_inputs.end(), 3, 0);
        packed[i / 8] |= (uint8_t)(b << (i % 8));
    }
    for (int variable = 0; variable < 2; ++variable) {
        Handles h;
        std::unique_ptr<uint32_t[]> bits(new uint32_t[n_bits]);
        uint32_t xy[2], pxy[2], out[3];
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 2, xy) || (variable && zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 2, pxy)) ||
            zk_builder_new_wires(h.b, ZK_WIRE_BIT, n_bits, bits.get()))
            return 3;
        if (variable ? zk_builder_babyjub_mul(h.b, pxy, bits.get(), n_bits, out) : zk_builder_babyjub_mul_fixed(h.b, bits.get(), n_bits, out)) return 3;
        if (zk_builder_babyjub_affine(h.b, out, xy)) return 3;
        size_t gates = 0;
        if (zk_builder_dims(h.b, nullptr, &gates) || zk_builder_finish(h.b, xy, 2, &h.c)) return 3;
        std::unique_ptr<uint64_t[]> want(new uint64_t[8]);
        if (zk_babyjub_mul(s.data(), variable ? g.get() : nullptr, want.get()) != ZK_OK) return 4;
        std::vector<uint64_t> fields(want.get(), want.get() + 8), w;
        if (variable) fields.insert(fields.end(), g.get(), g.get() + 8);
        std::vector<uint64_t> inputs(fields);
        inputs.insert(inputs.end(), bit_inputs.begin(), bit_inputs.end());
        if (!evaluate(*h.c, inputs, packed, fields, w)) return 4;
        // every gate holds: U_j V_j = W_j over the rows
        const size_t m = h.c->u.size();
        std::vector<Fr> val(m), u(h.c->n_gates, Fr::zero()), v(h.c->n_gates, Fr::zero()), o(h.c->n_gates, Fr::zero());
        for (size_t i = 0; i < m; ++i) val[i] = Fr::from_canonical(fr_from_words(w.data() + 4 * i));
        for (size_t i = 0; i < m; ++i) {
            for (const auto& e : h.c->u[i]) u[e.first] = u[e.first] + e.second * val[i];
            for (const auto& e : h.c->v[i]) v[e.first] = v[e.first] + e.second * val[i];
            for (const auto& e : h.c->w[i]) o[e.first] = o[e.first] + e.second * val[i];
        }
        for (size_t j = 0; j < h.c->n_gates; ++j)
            if (u[j] * v[j] != o[j]) return 5;
        std::cout << (variable ? "var " : "fixed ") << gates << " " << hex(w.data() + 4) << " " << hex(w.data() + 8) << "\n";
    }
    {
        Handles h;
        uint32_t x[3], out[3];
        int refused = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 3, x)) return 7;
        const uint32_t unknown[3] = {x[0], x[1], 99};
        refused += zk_builder_babyjub_mul_fixed(h.b, x, 0, out) == ZK_ERR_ARG;
        refused += zk_builder_babyjub_mul_fixed(h.b, unknown, 3, out) == ZK_ERR_ARG;
        refused += zk_builder_babyjub_mul(h.b, x, unknown, 3, out) == ZK_ERR_ARG;
        refused += zk_builder_babyjub_add(h.b, x, unknown, out) == ZK_ERR_ARG;
        refused += zk_builder_babyjub_affine(h.b, unknown, x) == ZK_ERR_ARG;
        refused += zk_builder_babyjub_assert_on_curve(h.b, nullptr) == ZK_ERR_ARG;
        size_t gates = 1;
        refused += zk_builder_dims(h.b, nullptr, &gates) == ZK_OK && gates == 0;      // a refusal emits nothing
        const uint64_t r[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
        std::unique_ptr<uint64_t[]> bad(new uint64_t[8]), off(new uint64_t[8]);
        std::copy(g.get(), g.get() + 8, bad.get());
        std::copy(r, r + 4, bad.get() + 4);
        std::copy(g.get(), g.get() + 8, off.get());
        off[4] ^= 1;
        refused += zk_babyjub_on_curve(bad.get()) == ZK_ERR_RANGE && zk_babyjub_on_curve(off.get()) == 0;
        refused += zk_babyjub_add(g.get(), bad.get(), q.get()) == ZK_ERR_RANGE && zk_babyjub_add(off.get(), g.get(), q.get()) == ZK_ERR_RANGE;
        refused += zk_babyjub_mul(k.get(), bad.get(), q.get()) == ZK_ERR_RANGE && zk_babyjub_mul(k.get(), off.get(), q.get()) == ZK_ERR_RANGE;
        std::cout << "refused " << refused << " of 10\n";
    }
    return 0;
}
