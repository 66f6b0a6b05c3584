// powers_host.hip -- the host code of a powers-of-tau contribution (csrc/powers_record.hip over csrc/crs_contribution.hip: the three
// role-tagged records; csrc/mul_each_recode.hpp: the split and the regular recoding k_mul_each's lanes do, compiled for the host)
// under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_powers_recode_host.py
// (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined).
// stdin: the three before-points (24 words, hex of their little-endian bytes) | secrets (12 words) | nonces (12 words) | tag (32 bytes).
// Prints "record <hex of the 672 bytes>", "verify V wrongtag W swapped S" (the record; under another tag; with tau and alpha
// exchanged) and "recoded N" (scalars, in heap buffers of their exact size, whose regular digits recompose to both halves for both
// window widths, compared modulo 2^64, every digit odd and in range).
#include "crs_contribution.hip"
#include "powers_record.hip"
#include "mul_each_recode.hpp"
#include <iostream>
#include <memory>
#include <string>

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
// exact-size heap copy, so that a byte read past the end is reported
template <class T>
static std::unique_ptr<T[]> heap(const std::vector<uint8_t>& v, size_t count) {
    std::unique_ptr<T[]> p(new T[count]);
    std::memcpy(p.get(), v.data(), count * sizeof(T));
    return p;
}

// the digits of one half recompose (mod 2^64) to its magnitude, plus one where it is even; all odd, |d| < 2^W
template <int W>
static bool half_ok(const uint32_t* m) {
    typedef zk::RegularRecode<W> RR;
    std::unique_ptr<uint32_t[]> b(new uint32_t[RR::NW]);
    bool even;
    zk::regular_recode<W>(m, b.get(), even);
    uint64_t sum = 0;
    for (int i = RR::ND - 1; i >= 0; --i) {
        uint32_t index;
        bool negative;
        zk::regular_next<W>(b.get(), index, negative);
        if (index >= (1u << (W - 1))) return false;
        const uint64_t d = 2 * (uint64_t)index + 1;
        if (W * i < 64) sum += (negative ? 0 - d : d) << (W * i);
    }
    for (int i = 0; i < RR::NW; ++i) if (b[i]) return false;
    const uint64_t want = (m[0] | ((uint64_t)m[1] << 32)) + (even ? 1 : 0);
    return sum == want && even == !(m[0] & 1);
}

int main() {
    std::string s_before, s_sec, s_nonce, s_tag;
    std::cin >> s_before >> s_sec >> s_nonce >> s_tag;
    const std::vector<uint8_t> b_before = unhex(s_before), b_sec = unhex(s_sec), b_nonce = unhex(s_nonce), b_tag = unhex(s_tag);
    if (b_before.size() != 192 || b_sec.size() != 96 || b_nonce.size() != 96 || b_tag.size() != 32) { std::puts("bad request"); return 1; }
    auto before = heap<uint64_t>(b_before, 24), sec = heap<uint64_t>(b_sec, 12), nonce = heap<uint64_t>(b_nonce, 12);
    auto tag = heap<uint8_t>(b_tag, 32);
    std::unique_ptr<zk_powers_contribution> rec(new zk_powers_contribution);
    if (zk_powers_contribution_prove(before.get(), sec.get(), nonce.get(), tag.get(), rec.get()) != ZK_OK) { std::puts("prove failed"); return 1; }
    std::printf("record %s\n", hex(reinterpret_cast<const uint8_t*>(rec.get()), sizeof(zk_powers_contribution)).c_str());
    int ok = -1, wrongtag = -1, swapped = -1;
    if (zk_powers_contribution_verify(rec.get(), tag.get(), &ok) != ZK_OK) return 1;
    auto other = heap<uint8_t>(b_tag, 32);
    other[0] ^= 1;
    if (zk_powers_contribution_verify(rec.get(), other.get(), &wrongtag) != ZK_OK) return 1;
    std::unique_ptr<zk_powers_contribution> bad(new zk_powers_contribution(*rec));
    bad->tau = rec->alpha;
    bad->alpha = rec->tau;
    if (zk_powers_contribution_verify(bad.get(), tag.get(), &swapped) != ZK_OK) return 1;
    std::printf("verify %d wrongtag %d swapped %d\n", ok, wrongtag, swapped);

    uint64_t x = 0x9E3779B97F4A7C15ull, good = 0;
    for (int it = 0; it < 1200; ++it) {
        std::unique_ptr<uint32_t[]> k(new uint32_t[8]);
        for (int w = 0; w < 8; ++w) {
            x += 0x9E3779B97F4A7C15ull;
            uint64_t z = x;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            k[w] = (uint32_t)(z ^ (z >> 31));
        }
        k[7] &= it % 7 == 0 ? 0u : 0x1fffffffu;   // below r; every seventh scalar is short
        if (it == 0) for (int w = 0; w < 8; ++w) k[w] = 0;
        std::unique_ptr<uint32_t[]> k1(new uint32_t[5]), k2(new uint32_t[5]);
        bool n1, n2;
        zk::glv_split_nearest(k.get(), k1.get(), n1, k2.get(), n2);
        if (k1[4] == 0 && k2[4] == 0 && half_ok<zk::ME_W_G1>(k1.get()) && half_ok<zk::ME_W_G1>(k2.get()) && half_ok<zk::ME_W_G2>(k1.get()) &&
            half_ok<zk::ME_W_G2>(k2.get()))
            ++good;
    }
    std::printf("recoded %llu\n", (unsigned long long)good);
    return 0;
}
