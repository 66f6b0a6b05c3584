// mixgen_host.hip -- the split of a built circuit into a boolean core and a field tail and its host runner (csrc/builder.hpp:
// built_split, mixed_run_host, over csrc/builder.hip) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program,
// built and run by tests/test_mixgen_host.py (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined).  No device, no context.
// stdin: one line, the hex of 32 bytes of input bits.  Every buffer handed to the code under test is a heap block of its exact size.
// Prints
//   "pack W V T"      per width W: the pack over the first W input bits, read by a tail sub-circuit (p + 7 f) p: V the packed value, T
//                     the tail wire, 64 hex digits each, equal from built_weights and from mixed_run_host
//   "dims ..."        n_bit n_field core_ops core_levels tail_ops tail_levels tail_slots | pack_core ... of a circuit with a pack over
//                     bit-class wires, a pack with one field-class operand and every gate kind on a field operand
//   "gates N"         witnesses of that circuit that agreed between the two evaluators
//   "field-only ..."  dims of a circuit without any boolean operation
//   "refused R of 4"  wrong byte count, wrong field count, wrong m, a field input >= r
#include "builder.hip"
#include <iostream>
#include <memory>
#include <string>

using namespace zk;

struct Handles {
    zk_builder* b = nullptr;
    zk_circuit* c = nullptr;
    Handles() { if (zk_builder_create(&b) != ZK_OK) std::abort(); }
    ~Handles() { zk_builder_free(b); delete c; }
};

static std::string hex_words(const uint64_t* w) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (int k = 3; k >= 0; --k)
        for (int i = 60; i >= 0; i -= 4) s += d[(w[k] >> i) & 15];
    return s;
}

// inputs in creation order (bits first, then fields: how every circuit here is made) through built_weights and through mixed_run_host
static bool evaluate(const zk_circuit& c, const std::vector<uint64_t>& bits, const std::vector<std::array<uint64_t, 4>>& fields, std::vector<uint64_t>& words) {
    const size_t m = c.u.size(), n_in = bits.size() + fields.size(), n_bytes = (bits.size() + 7) / 8;
    std::unique_ptr<uint64_t[]> in(new uint64_t[std::max<size_t>(4 * n_in, 1)]);
    for (size_t i = 0; i < bits.size(); ++i) { in[4 * i] = bits[i]; in[4 * i + 1] = in[4 * i + 2] = in[4 * i + 3] = 0; }
    for (size_t i = 0; i < fields.size(); ++i)
        for (int k = 0; k < 4; ++k) in[4 * (bits.size() + i) + k] = fields[i][k];
    std::unique_ptr<uint8_t[]> packed(new uint8_t[std::max<size_t>(n_bytes, 1)]);
    for (size_t i = 0; i < n_bytes; ++i) packed[i] = 0;
    for (size_t i = 0; i < bits.size(); ++i) packed[i / 8] |= (uint8_t)(bits[i] << (i % 8));
    std::unique_ptr<uint64_t[]> f(new uint64_t[std::max<size_t>(4 * fields.size(), 1)]);
    for (size_t i = 0; i < fields.size(); ++i)
        for (int k = 0; k < 4; ++k) f[4 * i + k] = fields[i][k];
    std::unique_ptr<uint64_t[]> a(new uint64_t[4 * m]), b(new uint64_t[4 * m]);
    built_weights(c, in.get(), n_in, a.get(), m);
    mixed_run_host(c, packed.get(), n_bytes, f.get(), fields.size(), b.get(), m);
    words.assign(b.get(), b.get() + 4 * m);
    for (size_t i = 0; i < 4 * m; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

static const uint64_t R_WORDS[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

int main() {
    std::string hexmsg;
    std::getline(std::cin, hexmsg);
    std::vector<uint64_t> bits;
    for (size_t i = 0; i + 1 < hexmsg.size(); i += 2) {
        const unsigned byte = (unsigned)std::stoul(hexmsg.substr(i, 2), nullptr, 16);
        for (int k = 0; k < 8; ++k) bits.push_back((byte >> k) & 1);
    }
    if (bits.size() < ZK_PACK_MAX_BITS) return 1;
    const std::array<uint64_t, 4> r_minus_1 = {R_WORDS[0] - 1, R_WORDS[1], R_WORDS[2], R_WORDS[3]}, one = {1, 0, 0, 0}, seven = {7, 0, 0, 0};

    for (size_t width : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)128, (size_t)ZK_PACK_MAX_BITS}) {
        Handles h;
        std::unique_ptr<uint32_t[]> in(new uint32_t[width]);
        uint32_t f, p, t;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, width, in.get()) || zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 1, &f)) return 2;
        if (zk_builder_pack(h.b, in.get(), width, &p)) return 2;
        const uint32_t lw[2] = {p, f};
        const uint64_t lweights[8] = {1, 0, 0, 0, 7, 0, 0, 0}, rweights[4] = {1, 0, 0, 0};
        if (zk_builder_sub_circuit(h.b, lweights, lw, 2, rweights, &p, 1, &t)) return 2;
        const uint32_t verify[2] = {p, t};
        if (zk_builder_finish(h.b, verify, 2, &h.c)) return 2;
        const Mixed& x = h.c->built->mix;
        if (x.pack_core.size() != 1 || !x.pack_core[0] || x.cpack_out.size() != 1 || x.tail.n_in != 1 || x.core_ops.size() != 0) return 3;
        std::vector<uint64_t> w;
        if (!evaluate(*h.c, std::vector<uint64_t>(bits.begin(), bits.begin() + width), {r_minus_1}, w)) return 4;
        std::cout << "pack " << width << " " << hex_words(&w[4]) << " " << hex_words(&w[8]) << "\n";
    }

    {
        Handles h;
        uint32_t x[6], f[2], g, fg, p[2], last = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 6, x) || zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 2, f)) return 5;
        if (zk_builder_gate(h.b, ZK_GATE_NOR, x[0], x[1], &g) || zk_builder_gate(h.b, ZK_GATE_AND, x[2], f[0], &fg)) return 5;
        const uint32_t core[5] = {x[3], g, ZK_WIRE_ONE, ZK_WIRE_ZERO, x[3]}, tail[3] = {x[4], fg, ZK_WIRE_ONE};
        if (zk_builder_pack(h.b, core, 5, &p[0]) || zk_builder_pack(h.b, tail, 3, &p[1])) return 5;
        for (int kind = ZK_GATE_BIT_CHECK; kind <= ZK_GATE_GREATER; ++kind) {
            if (zk_builder_gate(h.b, kind, f[1], x[5], &last) || zk_builder_gate(h.b, kind, g, f[1], &last)) return 5;
            if (zk_builder_gate(h.b, kind, p[0], last, &last) || zk_builder_gate(h.b, kind, x[5], g, &last)) return 5;
        }
        if (zk_builder_assert_bit(h.b, f[0]) || zk_builder_assert_bit(h.b, last)) return 5;
        const uint32_t verify[2] = {p[1], last};
        if (zk_builder_finish(h.b, verify, 2, &h.c)) return 5;
        const Mixed& m = h.c->built->mix;
        std::cout << "dims " << m.bit_in_wit.size() << " " << m.tail.n_in << " " << m.core_ops.size() << " " << m.core_level_ptr.size() - 1 << " "
                  << m.tail.ops.size() << " " << m.tail.levels() << " " << m.tail.slots << " |";
        for (uint8_t v : m.pack_core) std::cout << " " << (int)v;
        std::cout << "\n";
        int agreed = 0;
        for (unsigned k = 0; k < 64; ++k) {
            std::vector<uint64_t> in, w;
            for (int i = 0; i < 6; ++i) in.push_back((k >> i) & 1);
            agreed += evaluate(*h.c, in, {k % 3 == 0 ? r_minus_1 : (k % 3 == 1 ? one : seven), k % 2 ? r_minus_1 : std::array<uint64_t, 4>{k, 1, 0, 0}}, w);
        }
        std::cout << "gates " << agreed << "\n";
    }

    {
        Handles h;
        uint32_t f[2], t, u;
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 2, f)) return 6;
        const uint64_t w2[8] = {3, 0, 0, 0, R_WORDS[0] - 1, R_WORDS[1], R_WORDS[2], R_WORDS[3]}, w1[4] = {1, 0, 0, 0};
        const uint32_t one_wire[1] = {ZK_WIRE_ONE};
        if (zk_builder_sub_circuit(h.b, w2, f, 2, w1, &f[1], 1, &t) || zk_builder_sub_circuit(h.b, w1, &t, 1, w1, one_wire, 1, &u)) return 6;
        if (zk_builder_finish(h.b, &u, 1, &h.c)) return 6;
        const Mixed& m = h.c->built->mix;
        std::vector<uint64_t> w;
        if (!evaluate(*h.c, {}, {seven, r_minus_1}, w)) return 6;
        std::cout << "field-only " << m.bit_in_wit.size() << " " << m.tail.n_in << " " << m.core_ops.size() << " " << m.core_level_ptr.size() - 1 << " "
                  << m.tail.ops.size() << " " << m.tail.levels() << " " << m.tail.slots << "\n";

        int refused = 0;
        std::unique_ptr<uint64_t[]> in(new uint64_t[8]), out(new uint64_t[4 * h.c->u.size()]);
        for (int k = 0; k < 8; ++k) in[k] = k % 4 == 0;
        auto status = [&](size_t n_bytes, size_t n_field, size_t m_out) {
            uint8_t byte = 0;
            try { mixed_run_host(*h.c, &byte, n_bytes, in.get(), n_field, out.get(), m_out); }
            catch (const ParseError& e) { return e.status; }
            return (int)ZK_OK;
        };
        const size_t m_circuit = h.c->u.size();
        if (status(0, 2, m_circuit) != ZK_OK) return 7;
        refused += status(1, 2, m_circuit) == ZK_ERR_ARG;
        refused += status(0, 1, m_circuit) == ZK_ERR_ARG;
        refused += status(0, 2, m_circuit - 1) == ZK_ERR_ARG;
        for (int k = 0; k < 4; ++k) in[4 + k] = R_WORDS[k];
        refused += status(0, 2, m_circuit) == ZK_ERR_RANGE;
        std::cout << "refused " << refused << " of 4\n";
    }
    return 0;
}
