// poseidon_host.hip -- Poseidon's host code (csrc/poseidon.hpp: the Grain generator, the parameters, the permutation; the gadgets of
// csrc/builder.hpp over linear forms; zk_builder_finish and the three host evaluators on what they emit) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_poseidon_host.py (hipcc --cuda-host-only -Xarch_host
// -fsanitize=address,undefined).  No device, no context.
// stdin: one line, hex words separated by spaces: four field elements a b c d (64 digits each), then a leaf index.  Prints
//   "params A RP C0 CLAST M00 MLAST"   per arity: R_P, the first and last round constant, the first and last entry of M
//   "hash A D"                         per arity: the digest of the first A of a b c d
//   "zero D"                           z_3
//   "gadget A N D"                     per arity: gates, and the gadget's output wire from all three evaluators (they agree)
//   "merkle N ROOT"                    a depth-3 membership circuit for leaf `index` of the five leaves a b c d a: gates, the root wire
//   "refused R"                        refusals that came back with the right status out of those tried
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

// the three evaluators on exact-size heap buffers; false where they differ.  bits: the packed bit inputs, fields: the field inputs, in
// input order; `inputs`: all inputs in creation order
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
    std::string line;
    std::getline(std::cin, line);
    std::istringstream is(line);
    std::vector<uint64_t> abcd(16);
    for (int i = 0; i < 4; ++i) { std::string s; is >> s; parse(s, abcd.data() + 4 * i); }
    uint64_t index = 0;
    is >> index;

    for (size_t arity : {1, 2, 4}) {
        const size_t t = arity + 1;
        unsigned rf = 0, rp = 0;
        if (zk_poseidon_params(arity, &rf, &rp, nullptr, nullptr) != ZK_OK || rf != 8) return 1;
        const size_t nc = (rf + rp) * t;
        std::unique_ptr<uint64_t[]> c(new uint64_t[4 * nc]), m(new uint64_t[4 * t * t]);
        if (zk_poseidon_params(arity, nullptr, nullptr, c.get(), m.get()) != ZK_OK) return 1;
        std::cout << "params " << arity << " " << rp << " " << hex(c.get()) << " " << hex(c.get() + 4 * (nc - 1)) << " " << hex(m.get()) << " "
                  << hex(m.get() + 4 * (t * t - 1)) << "\n";
    }
    for (size_t arity : {1, 2, 4}) {
        std::unique_ptr<uint64_t[]> in(new uint64_t[4 * arity]), out(new uint64_t[4]);
        std::copy(abcd.begin(), abcd.begin() + 4 * arity, in.get());
        if (zk_poseidon_hash(in.get(), arity, out.get()) != ZK_OK) return 2;
        std::cout << "hash " << arity << " " << hex(out.get()) << "\n";
    }
    {
        const std::vector<Fr> z = poseidon_zero_hashes(3);
        uint64_t w[4];
        fr_to_words(z[3].to_canonical(), w);
        std::cout << "zero " << hex(w) << "\n";
    }
    for (size_t arity : {1, 2, 4}) {
        Handles h;
        std::unique_ptr<uint32_t[]> in(new uint32_t[arity]);
        uint32_t out = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, arity, in.get()) || zk_builder_poseidon(h.b, in.get(), arity, &out)) return 3;
        size_t gates = 0;
        if (zk_builder_dims(h.b, nullptr, &gates) || zk_builder_finish(h.b, &out, 1, &h.c)) return 3;
        const std::vector<uint64_t> inputs(abcd.begin(), abcd.begin() + 4 * arity);
        std::vector<uint64_t> w;
        if (!evaluate(*h.c, inputs, {}, inputs, w)) return 4;
        std::cout << "gadget " << arity << " " << gates << " " << hex(w.data() + 4) << "\n";
    }
    {
        // five leaves: a, b, c, d, a; the path of leaf `index` from a host-side tree over zk_poseidon_hash
        const unsigned depth = 3;
        std::vector<std::vector<uint64_t>> level(1);
        for (int i = 0; i < 5; ++i) level[0].insert(level[0].end(), abcd.begin() + 4 * (i % 4), abcd.begin() + 4 * (i % 4) + 4);
        const std::vector<Fr> z = poseidon_zero_hashes(depth);
        std::vector<uint64_t> fields(level[0].begin() + 4 * index, level[0].begin() + 4 * index + 4);
        for (unsigned k = 0; k < depth; ++k) {
            const std::vector<uint64_t>& below = level[k];
            uint64_t zero[4];
            fr_to_words(z[k].to_canonical(), zero);
            auto node = [&](size_t i, uint64_t* o) {          // a child that does not exist is z_k
                const uint64_t* src = 4 * i + 4 <= below.size() ? below.data() + 4 * i : zero;
                std::copy(src, src + 4, o);
            };
            uint64_t sib[4];
            node((index >> k) ^ 1, sib);
            fields.insert(fields.end(), sib, sib + 4);
            std::vector<uint64_t> next;
            for (size_t i = 0; i < std::max<size_t>(1, (below.size() / 4 + 1) / 2); ++i) {
                uint64_t pair[8], o[4];
                node(2 * i, pair);
                node(2 * i + 1, pair + 4);
                if (zk_poseidon_hash(pair, 2, o) != ZK_OK) return 5;
                next.insert(next.end(), o, o + 4);
            }
            level.push_back(next);
        }
        Handles h;
        uint32_t leaf = 0, sibs[3], dirs[3], root = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 1, &leaf) || zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 3, sibs) ||
            zk_builder_new_wires(h.b, ZK_WIRE_BIT, 3, dirs) || zk_builder_merkle_root(h.b, leaf, sibs, dirs, depth, &root))
            return 5;
        size_t gates = 0;
        if (zk_builder_dims(h.b, nullptr, &gates) || zk_builder_finish(h.b, &root, 1, &h.c)) return 5;
        std::vector<uint64_t> inputs(fields), w;
        for (unsigned k = 0; k < depth; ++k) { inputs.push_back((index >> k) & 1); inputs.insert(inputs.end(), 3, 0); }
        if (!evaluate(*h.c, inputs, {(uint8_t)index}, fields, w)) return 6;
        if (!std::equal(w.begin() + 4, w.begin() + 8, level[depth].begin())) return 6;
        std::cout << "merkle " << gates << " " << hex(w.data() + 4) << "\n";
    }
    {
        Handles h;
        uint32_t x[2], out = 0;
        int refused = 0;
        if (zk_builder_new_wires(h.b, ZK_WIRE_FIELD, 2, x)) return 7;
        const uint32_t three[3] = {x[0], x[1], x[0]}, unknown[2] = {x[0], 99};
        refused += zk_builder_poseidon(h.b, three, 3, &out) == ZK_ERR_ARG;
        refused += zk_builder_poseidon(h.b, x, 0, &out) == ZK_ERR_ARG;
        refused += zk_builder_poseidon(h.b, unknown, 2, &out) == ZK_ERR_ARG;
        refused += zk_builder_merkle_root(h.b, x[0], unknown, x, 2, &out) == ZK_ERR_ARG;
        refused += zk_builder_merkle_root(h.b, x[0], nullptr, nullptr, 1, &out) == ZK_ERR_ARG;
        size_t gates = 1;
        refused += zk_builder_dims(h.b, nullptr, &gates) == ZK_OK && gates == 0;      // a refusal emits nothing
        refused += zk_builder_merkle_root(h.b, x[1], nullptr, nullptr, 0, &out) == ZK_OK && out == x[1];
        const uint64_t r[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
        uint64_t o[4];
        refused += zk_poseidon_hash(r, 1, o) == ZK_ERR_RANGE;
        refused += zk_poseidon_hash(r, 3, o) == ZK_ERR_ARG && zk_poseidon_params(3, nullptr, nullptr, nullptr, nullptr) == ZK_ERR_ARG;
        std::cout << "refused " << refused << " of 9\n";
    }
    return 0;
}
