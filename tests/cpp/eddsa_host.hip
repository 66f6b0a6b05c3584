// eddsa_host.hip -- EdDSA-Poseidon's host code (csrc/eddsa.hpp: arithmetic mod l, H6 and its parameters, sign, verify; the gadget of
// csrc/builder.hpp; zk_builder_finish and the three host evaluators on what it emits) under AddressSanitizer and
// UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_eddsa_host.py (hipcc --cuda-host-only -Xarch_host
// -fsanitize=address,undefined).  No device, no context.
// stdin: one line: a key k, a nonce key and a message, 64 hex digits each.  Prints
//   "challenge H"                     H6(1, 2, 3, 4, 5) through zk_eddsa_challenge
//   "c I V" x 408, "m I V" x 36       the round constants and the matrix of width 6
//   "public X Y"                      [k] Base8
//   "sign RX RY S"                    the signature
//   "status a b c d e f"              zk_eddsa_verify on: the signature; the message + 1; S + l; A.x = r; A.y + 1; R8.y + 1
//   "gadget N F"                      zk_builder_eddsa_verify: gates, and the gates that do not hold on the signature's witness
//   "refused R of 9"                  refusals that came back with the right status
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
static void add_small(const uint64_t* a, const uint64_t* b, uint64_t* out) {   // 256-bit a + b, no reduction
    unsigned __int128 carry = 0;
    for (int i = 0; i < 4; ++i) {
        carry += (unsigned __int128)a[i] + b[i];
        out[i] = (uint64_t)carry;
        carry >>= 64;
    }
}

struct Handles {
    zk_builder* b = nullptr;
    zk_circuit* c = nullptr;
    Handles() { if (zk_builder_create(&b) != ZK_OK) std::abort(); }
    ~Handles() { zk_builder_free(b); delete c; }
};

int main() {
    std::string line, ks, ns, ms;
    std::getline(std::cin, line);
    std::istringstream is(line);
    is >> ks >> ns >> ms;
    if (ks.size() != 64 || ns.size() != 64 || ms.size() != 64) return 1;
    // every buffer the library writes is an exact-size heap block
    std::unique_ptr<uint64_t[]> k(new uint64_t[4]), nonce(new uint64_t[4]), msg(new uint64_t[4]), a(new uint64_t[8]), r8(new uint64_t[8]),
        s(new uint64_t[4]), h(new uint64_t[4]);
    parse(ks, k.get()); parse(ns, nonce.get()); parse(ms, msg.get());
    {
        const uint64_t p[8] = {1, 0, 0, 0, 2, 0, 0, 0}, q[8] = {3, 0, 0, 0, 4, 0, 0, 0}, m[4] = {5, 0, 0, 0};
        if (zk_eddsa_challenge(p, q, m, h.get()) != ZK_OK) return 2;
        std::cout << "challenge " << hex(h.get()) << "\n";
        std::unique_ptr<uint64_t[]> c(new uint64_t[4 * 408]), mds(new uint64_t[4 * 36]);
        eddsa_h6_params_words(c.get(), mds.get());
        for (int i = 0; i < 408; ++i) std::cout << "c " << i << " " << hex(c.get() + 4 * i) << "\n";
        for (int i = 0; i < 36; ++i) std::cout << "m " << i << " " << hex(mds.get() + 4 * i) << "\n";
    }
    if (zk_eddsa_public_key(k.get(), a.get()) != ZK_OK) return 3;
    std::cout << "public " << hex(a.get()) << " " << hex(a.get() + 4) << "\n";
    if (zk_eddsa_sign(k.get(), nonce.get(), msg.get(), r8.get(), s.get()) != ZK_OK) return 3;
    std::cout << "sign " << hex(r8.get()) << " " << hex(r8.get() + 4) << " " << hex(s.get()) << "\n";
    const uint64_t r[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
    const uint64_t one[4] = {1, 0, 0, 0};
    {
        int st[6];
        std::unique_ptr<uint64_t[]> t(new uint64_t[8]), u(new uint64_t[4]);
        if (zk_eddsa_verify(a.get(), msg.get(), r8.get(), s.get(), &st[0])) return 4;
        add_small(msg.get(), one, u.get());
        if (zk_eddsa_verify(a.get(), u.get(), r8.get(), s.get(), &st[1])) return 4;
        add_small(s.get(), BABYJUB_ORDER, u.get());
        if (zk_eddsa_verify(a.get(), msg.get(), r8.get(), u.get(), &st[2])) return 4;
        std::copy(a.get(), a.get() + 8, t.get());
        std::copy(r, r + 4, t.get());
        if (zk_eddsa_verify(t.get(), msg.get(), r8.get(), s.get(), &st[3])) return 4;
        std::copy(a.get(), a.get() + 8, t.get());
        add_small(a.get() + 4, one, t.get() + 4);
        if (zk_eddsa_verify(t.get(), msg.get(), r8.get(), s.get(), &st[4])) return 4;
        std::copy(r8.get(), r8.get() + 8, t.get());
        add_small(r8.get() + 4, one, t.get() + 4);
        if (zk_eddsa_verify(a.get(), msg.get(), t.get(), s.get(), &st[5])) return 4;
        std::cout << "status";
        for (int v : st) std::cout << " " << v;
        std::cout << "\n";
    }
    {
        Handles hd;
        std::unique_ptr<uint32_t[]> f(new uint32_t[5]), sb(new uint32_t[251]), hb(new uint32_t[254]);
        if (zk_builder_new_wires(hd.b, ZK_WIRE_FIELD, 5, f.get()) || zk_builder_new_wires(hd.b, ZK_WIRE_BIT, 251, sb.get()) ||
            zk_builder_new_wires(hd.b, ZK_WIRE_BIT, 254, hb.get()))
            return 5;
        if (zk_builder_eddsa_verify(hd.b, f.get(), f.get() + 2, f[4], sb.get(), hb.get())) return 5;
        size_t gates = 0;
        if (zk_builder_dims(hd.b, nullptr, &gates) || zk_builder_finish(hd.b, nullptr, 0, &hd.c)) return 5;
        if (zk_eddsa_challenge(r8.get(), a.get(), msg.get(), h.get()) != ZK_OK) return 5;
        std::vector<uint64_t> fields(a.get(), a.get() + 8), inputs;
        fields.insert(fields.end(), r8.get(), r8.get() + 8);
        fields.insert(fields.end(), msg.get(), msg.get() + 4);
        inputs = fields;
        std::vector<uint8_t> packed((251 + 254 + 7) / 8, 0);
        for (size_t i = 0; i < 251 + 254; ++i) {
            const uint64_t* src = i < 251 ? s.get() : h.get();
            const size_t at = i < 251 ? i : i - 251;
            const uint64_t bit = (src[at / 64] >> (at % 64)) & 1;
            inputs.push_back(bit);
            inputs.insert(inputs.end(), 3, 0);
            packed[i / 8] |= (uint8_t)(bit << (i % 8));
        }
        const zk_circuit& c = *hd.c;
        const size_t m = c.u.size(), n_in = inputs.size() / 4;
        std::unique_ptr<uint64_t[]> in(new uint64_t[inputs.size()]), w0(new uint64_t[4 * m]), w1(new uint64_t[4 * m]), w2(new uint64_t[4 * m]);
        std::copy(inputs.begin(), inputs.end(), in.get());
        built_weights(c, in.get(), n_in, w0.get(), m);
        built_check_inputs(c.tape, in.get(), n_in);
        if (c.tape.status) return 6;
        std::unique_ptr<Fr[]> vals(new Fr[c.tape.slots]);
        tape_run_host(c.tape, in.get(), vals.get(), w1.get());
        std::unique_ptr<uint8_t[]> pb(new uint8_t[packed.size()]);
        std::copy(packed.begin(), packed.end(), pb.get());
        std::unique_ptr<uint64_t[]> pf(new uint64_t[fields.size()]);
        std::copy(fields.begin(), fields.end(), pf.get());
        mixed_run_host(c, pb.get(), packed.size(), pf.get(), fields.size() / 4, w2.get(), m);
        for (size_t i = 0; i < 4 * m; ++i)
            if (w0[i] != w1[i] || w0[i] != w2[i]) return 6;
        std::vector<Fr> val(m), u(c.n_gates, Fr::zero()), v(c.n_gates, Fr::zero()), o(c.n_gates, Fr::zero());
        for (size_t i = 0; i < m; ++i) val[i] = Fr::from_canonical(fr_from_words(w0.get() + 4 * i));
        for (size_t i = 0; i < m; ++i) {
            for (const auto& e : c.u[i]) u[e.first] = u[e.first] + e.second * val[i];
            for (const auto& e : c.v[i]) v[e.first] = v[e.first] + e.second * val[i];
            for (const auto& e : c.w[i]) o[e.first] = o[e.first] + e.second * val[i];
        }
        size_t failing = 0;
        for (size_t j = 0; j < c.n_gates; ++j) failing += u[j] * v[j] != o[j];
        std::cout << "gadget " << gates << " " << failing << "\n";
    }
    {
        Handles hd;
        int refused = 0;
        std::unique_ptr<uint32_t[]> f(new uint32_t[5]), sb(new uint32_t[251]), hb(new uint32_t[254]);
        if (zk_builder_new_wires(hd.b, ZK_WIRE_FIELD, 5, f.get()) || zk_builder_new_wires(hd.b, ZK_WIRE_BIT, 251, sb.get()) ||
            zk_builder_new_wires(hd.b, ZK_WIRE_BIT, 254, hb.get()))
            return 7;
        hb[253] = 100000;
        refused += zk_builder_eddsa_verify(hd.b, f.get(), f.get() + 2, f[4], sb.get(), hb.get()) == ZK_ERR_ARG;
        refused += zk_builder_eddsa_verify(hd.b, f.get(), nullptr, f[4], sb.get(), hb.get()) == ZK_ERR_ARG;
        size_t gates = 1;
        refused += zk_builder_dims(hd.b, nullptr, &gates) == ZK_OK && gates == 0;      // a refusal emits nothing
        const uint64_t zero[4] = {0, 0, 0, 0};
        std::unique_ptr<uint64_t[]> o8(new uint64_t[8]), o4(new uint64_t[4]);
        refused += zk_eddsa_sign(zero, nonce.get(), msg.get(), o8.get(), o4.get()) == ZK_ERR_RANGE;
        refused += zk_eddsa_sign(BABYJUB_ORDER, nonce.get(), msg.get(), o8.get(), o4.get()) == ZK_ERR_RANGE;
        refused += zk_eddsa_sign(k.get(), r, msg.get(), o8.get(), o4.get()) == ZK_ERR_RANGE;
        refused += zk_eddsa_sign(k.get(), nonce.get(), r, o8.get(), o4.get()) == ZK_ERR_RANGE;
        refused += zk_eddsa_public_key(BABYJUB_ORDER, o8.get()) == ZK_ERR_RANGE;
        refused += zk_eddsa_challenge(r8.get(), a.get(), r, o4.get()) == ZK_ERR_RANGE;
        std::cout << "refused " << refused << " of 9\n";
    }
    return 0;
}
