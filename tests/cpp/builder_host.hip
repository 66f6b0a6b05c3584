// builder_host.hip -- the circuit builder's host code (csrc/builder.hip over csrc/builder.hpp: the constructors, zk_builder_finish, the
// field tape's compiler and both host evaluators) under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, built
// and run by tests/test_builder_host.py (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined).  No device, no context.
// stdin: one line, the hex of a message.  Prints
//   "gate K T"        per gate kind K: the outputs on (x, y) = (0,0) (1,0) (0,1) (1,1) as four digits, from both evaluators
//   "cmp C"           the six 64-bit comparators on fixed operand pairs: how many (kind, pair) results were right (and agreed)
//   "keccak N D"      SHA3-256 at 2 rounds of the message: gates, digest hex
//   "refused R"       refusals that came back as ZK_ERR_ARG out of those tried
#include "builder.hip"
#include <iostream>
#include <memory>
#include <string>

using namespace zk;

// both evaluators on exact-size heap buffers; returns false where they differ
static bool evaluate(const zk_circuit& c, const std::vector<uint64_t>& bits, std::vector<uint64_t>& first_words) {
    const size_t m = c.u.size(), n_in = bits.size();
    std::unique_ptr<uint64_t[]> in(new uint64_t[std::max<size_t>(4 * n_in, 1)]);
    for (size_t i = 0; i < n_in; ++i) { in[4 * i] = bits[i]; in[4 * i + 1] = in[4 * i + 2] = in[4 * i + 3] = 0; }
    std::unique_ptr<uint64_t[]> a(new uint64_t[4 * m]), b(new uint64_t[4 * m]);
    built_weights(c, in.get(), n_in, a.get(), m);
    built_check_inputs(c.tape, in.get(), n_in);
    if (c.tape.status) return false;
    std::unique_ptr<Fr[]> vals(new Fr[c.tape.slots]);
    tape_run_host(c.tape, in.get(), vals.get(), b.get());
    first_words.resize(m);
    bool same = true;
    for (size_t i = 0; i < m; ++i) {
        first_words[i] = a[4 * i];
        for (int k = 0; k < 4; ++k) same = same && a[4 * i + k] == b[4 * i + k] && (k == 0 || a[4 * i + k] == 0);
    }
    return same;
}

struct Handles {
    zk_builder* b = nullptr;
    zk_circuit* c = nullptr;
    Handles() { if (zk_builder_create(&b) != ZK_OK) std::abort(); }
    ~Handles() { zk_builder_free(b); delete c; }
};

int main() {
    std::string hexmsg;
    std::getline(std::cin, hexmsg);
    std::vector<uint8_t> msg(hexmsg.size() / 2);
    for (size_t i = 0; i < msg.size(); ++i) msg[i] = (uint8_t)std::stoul(hexmsg.substr(2 * i, 2), nullptr, 16);

    for (int kind = ZK_GATE_BIT_CHECK; kind <= ZK_GATE_GREATER; ++kind) {
        Handles h;
        uint32_t in[2], out;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 2, in) || zk_builder_gate(h.b, kind, in[0], in[1], &out) || zk_builder_finish(h.b, &out, 1, &h.c)) return 1;
        std::string t;
        for (uint64_t v = 0; v < 4; ++v) {
            std::vector<uint64_t> w;
            if (!evaluate(*h.c, {v & 1, v >> 1}, w)) return 2;
            t += (char)('0' + w[1]);
        }
        std::cout << "gate " << kind << " " << t << "\n";
    }

    const uint64_t top = 1ull << 63, full = ~0ull;
    const uint64_t pairs[][2] = {{0, 0}, {0, 1}, {1, 0}, {top, top}, {top, full}, {full, top}, {full, full}, {top | 5, 5}, {6, 7}, {full - 1, full}};
    int right = 0;
    for (int kind = ZK_CMP_EQUAL; kind <= ZK_CMP_GREATER_EQ; ++kind) {
        Handles h;
        uint32_t l[64], r[64], out;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 64, l) || (kind != ZK_CMP_EQUAL_ZERO && zk_builder_new_wires(h.b, ZK_WIRE_BIT, 64, r))) return 3;
        if (zk_builder_compare(h.b, kind, l, kind == ZK_CMP_EQUAL_ZERO ? nullptr : r, 64, &out) || zk_builder_finish(h.b, &out, 1, &h.c)) return 3;
        for (const auto& p : pairs) {
            std::vector<uint64_t> bits, w;
            for (int i = 0; i < 64; ++i) bits.push_back((p[0] >> i) & 1);
            if (kind != ZK_CMP_EQUAL_ZERO) for (int i = 0; i < 64; ++i) bits.push_back((p[1] >> i) & 1);
            if (!evaluate(*h.c, bits, w)) return 4;
            const bool want = kind == ZK_CMP_EQUAL ? p[0] == p[1] : kind == ZK_CMP_EQUAL_ZERO ? p[0] == 0 : kind == ZK_CMP_LESS ? p[0] < p[1]
                            : kind == ZK_CMP_LESS_EQ ? p[0] <= p[1] : kind == ZK_CMP_GREATER ? p[0] > p[1] : p[0] >= p[1];
            right += w[1] == (want ? 1u : 0u);
        }
    }
    std::cout << "cmp " << right << "\n";

    {
        Handles h;
        std::unique_ptr<uint32_t[]> in(new uint32_t[std::max<size_t>(8 * msg.size(), 1)]), out(new uint32_t[256]);
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 8 * msg.size(), in.get())) return 5;
        if (zk_builder_keccak(h.b, in.get(), msg.size(), 136, 0x06, 2, out.get(), 32)) return 5;
        if (zk_builder_assert_bit(h.b, in[0]) || zk_builder_finish(h.b, out.get(), 256, &h.c)) return 5;
        std::vector<uint64_t> bits, w;
        for (uint8_t byte : msg) for (int i = 0; i < 8; ++i) bits.push_back((byte >> i) & 1);
        if (!evaluate(*h.c, bits, w)) return 6;
        static const char* d = "0123456789abcdef";
        std::string digest;
        for (int k = 0; k < 32; ++k) {
            unsigned v = 0;
            for (int i = 0; i < 8; ++i) v |= (unsigned)w[1 + 8 * k + i] << i;
            digest += d[v >> 4];
            digest += d[v & 15];
        }
        std::cout << "keccak " << h.c->n_gates << " " << digest << "\n";
    }

    {
        Handles h;
        uint32_t x[2], out = 0;
        int refused = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 2, x)) return 7;
        refused += zk_builder_gate(h.b, ZK_GATE_AND, x[0], 99, &out) == ZK_ERR_ARG;
        refused += zk_builder_gate(h.b, 77, x[0], x[1], &out) == ZK_ERR_ARG;
        refused += zk_builder_keccak(h.b, x, 0, 0, 1, 24, &out, 0) == ZK_ERR_ARG;
        const uint32_t twice[2] = {x[0], x[0]}, constant[1] = {ZK_WIRE_ONE};
        refused += zk_builder_finish(h.b, twice, 2, &h.c) == ZK_ERR_ARG;
        refused += zk_builder_finish(h.b, constant, 1, &h.c) == ZK_ERR_ARG;
        if (zk_builder_finish(h.b, x, 1, &h.c)) return 7;
        refused += zk_builder_gate(h.b, ZK_GATE_AND, x[0], x[1], &out) == ZK_ERR_ARG;
        zk_circuit* again = nullptr;
        refused += zk_builder_finish(h.b, x, 1, &again) == ZK_ERR_ARG && again == nullptr;
        std::cout << "refused " << refused << " of 7\n";
    }
    return 0;
}
