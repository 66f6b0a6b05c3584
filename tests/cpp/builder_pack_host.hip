// builder_pack_host.hip -- zk_builder_pack's host code (csrc/builder.hip over csrc/builder.hpp: the constructor, the pack lists that
// zk_builder_finish leaves in Built, the tape compiler and both host evaluators on weights 2^i) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_builder_pack_host.py (hipcc --cuda-host-only
// -Xarch_host -fsanitize=address,undefined).  No device, no context.  stdin: one line, the hex of the input bits' bytes.  Prints
//   "pack W V"        per width W: the packed value on the first W input bits as 64 hex digits, from both evaluators
//   "lists ..."       Built's CSR lists of a circuit with constants and a repeated wire: pack_out | pack_ptr | pack_bits
//   "boolean A B C"   is-boolean of: packs over gates; a packed wire into AND; a packed wire into a pack
//   "refused R of N"  refusals that came back as ZK_ERR_ARG
#include "builder.hip"
#include <iostream>
#include <memory>
#include <string>

using namespace zk;

// both evaluators on exact-size heap buffers; returns false where they differ
static bool evaluate(const zk_circuit& c, const std::vector<uint64_t>& bits, std::vector<uint64_t>& words) {
    const size_t m = c.u.size(), n_in = bits.size();
    std::unique_ptr<uint64_t[]> in(new uint64_t[std::max<size_t>(4 * n_in, 1)]);
    for (size_t i = 0; i < n_in; ++i) { in[4 * i] = bits[i]; in[4 * i + 1] = in[4 * i + 2] = in[4 * i + 3] = 0; }
    std::unique_ptr<uint64_t[]> a(new uint64_t[4 * m]), b(new uint64_t[4 * m]);
    built_weights(c, in.get(), n_in, a.get(), m);
    built_check_inputs(c.tape, in.get(), n_in);
    if (c.tape.status) return false;
    std::unique_ptr<Fr[]> vals(new Fr[c.tape.slots]);
    tape_run_host(c.tape, in.get(), vals.get(), b.get());
    words.assign(a.get(), a.get() + 4 * m);
    for (size_t i = 0; i < 4 * m; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

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

int main() {
    std::string hexmsg;
    std::getline(std::cin, hexmsg);
    std::vector<uint64_t> bits;
    for (size_t i = 0; i + 1 < hexmsg.size(); i += 2) {
        const unsigned byte = (unsigned)std::stoul(hexmsg.substr(i, 2), nullptr, 16);
        for (int k = 0; k < 8; ++k) bits.push_back((byte >> k) & 1);
    }
    if (bits.size() < ZK_PACK_MAX_BITS) return 1;

    for (size_t width : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)128, (size_t)ZK_PACK_MAX_BITS}) {
        Handles h;
        std::unique_ptr<uint32_t[]> in(new uint32_t[width]);          // exact size: a read past the operands is caught
        uint32_t out;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, width, in.get()) || zk_builder_pack(h.b, in.get(), width, &out)) return 2;
        if (zk_builder_finish(h.b, &out, 1, &h.c)) return 2;
        if (h.c->built->pack_out.size() != 1 || !h.c->built->boolean) return 3;
        std::vector<uint64_t> w;
        if (!evaluate(*h.c, std::vector<uint64_t>(bits.begin(), bits.begin() + width), w)) return 4;
        std::cout << "pack " << width << " " << hex_words(&w[4]) << "\n";
    }

    {
        Handles h;
        uint32_t x[3], g, p[2];
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 3, x) || zk_builder_gate(h.b, ZK_GATE_XOR, x[0], x[1], &g)) return 5;
        const uint32_t first[6] = {x[2], ZK_WIRE_ZERO, g, ZK_WIRE_ONE, x[2], ZK_WIRE_ZERO}, second[1] = {ZK_WIRE_ZERO};
        if (zk_builder_pack(h.b, first, 6, &p[0]) || zk_builder_pack(h.b, second, 1, &p[1])) return 5;
        if (zk_builder_finish(h.b, &p[1], 1, &h.c)) return 5;
        const Built& built = *h.c->built;
        std::cout << "lists";
        for (uint32_t v : built.pack_out) std::cout << " " << v;
        std::cout << " |";
        for (uint32_t v : built.pack_ptr) std::cout << " " << v;
        std::cout << " |";
        for (uint32_t v : built.pack_bits) std::cout << " " << v;
        std::cout << "\n";
        std::vector<uint64_t> w;
        if (!evaluate(*h.c, {1, 0, 1}, w)) return 6;
        if (w[4 * 1] != 0 || w[4 * built.pack_out[0]] != (1 | 4 | 8 | 16)) return 6;      // x2 + 4 (x0 ^ x1) + 8 + 16 x2
    }

    {
        int flags[3];
        for (int k = 0; k < 3; ++k) {
            Handles h;
            uint32_t x[4], g, p, q;
            if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, 4, x) || zk_builder_gate(h.b, ZK_GATE_AND, x[0], x[1], &g)) return 7;
            const uint32_t ops[3] = {g, x[2], ZK_WIRE_ONE};
            if (zk_builder_pack(h.b, ops, 3, &p)) return 7;
            const uint32_t nested[2] = {x[3], p};
            if (k == 1 && zk_builder_gate(h.b, ZK_GATE_AND, p, x[3], &g)) return 7;
            if (k == 2 && zk_builder_pack(h.b, nested, 2, &q)) return 7;
            if (zk_builder_finish(h.b, &p, 1, &h.c)) return 7;
            flags[k] = h.c->built->boolean;
            std::vector<uint64_t> w;
            if (!evaluate(*h.c, {1, 1, 0, 1}, w) || w[4] != 5) return 8;
        }
        std::cout << "boolean " << flags[0] << " " << flags[1] << " " << flags[2] << "\n";
    }

    {
        Handles h;
        std::unique_ptr<uint32_t[]> x(new uint32_t[ZK_PACK_MAX_BITS + 1]);
        uint32_t out = 0;
        int refused = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_BIT, ZK_PACK_MAX_BITS + 1, x.get())) return 9;
        refused += zk_builder_pack(h.b, x.get(), 0, &out) == ZK_ERR_ARG;
        refused += zk_builder_pack(h.b, x.get(), ZK_PACK_MAX_BITS + 1, &out) == ZK_ERR_ARG;
        const uint32_t unknown[2] = {x[0], 100000};
        refused += zk_builder_pack(h.b, unknown, 2, &out) == ZK_ERR_ARG;
        refused += zk_builder_pack(h.b, x.get(), 2, nullptr) == ZK_ERR_ARG;
        if (zk_builder_finish(h.b, x.get(), 1, &h.c)) return 9;
        refused += zk_builder_pack(h.b, x.get(), 2, &out) == ZK_ERR_ARG;
        if (!h.c->built->pack_out.empty() || h.c->built->pack_ptr.size() != 1) return 9;
        std::cout << "refused " << refused << " of 5\n";
    }
    return 0;
}
