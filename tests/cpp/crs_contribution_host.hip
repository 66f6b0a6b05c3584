// crs_contribution_host.hip -- csrc/crs_contribution.hip (SHA-256, the GLV split and recoding, the contribution record) under
// AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program, built and run by tests/test_crs_contribute_host.py
// (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined).
// stdin: delta_before (8 words, hex of their little-endian bytes) | d (4 words) | nonce (4 words) | tag (32 bytes), one per line.
// Prints "record <hex of the 224 bytes>", "verify V tampered T malformed M" (the record, the record with one response bit flipped,
// the record with delta_after = (0, 1)), "recoded N" (scalars, in heap buffers of their exact size, whose digits recompose to the
// two halves of the split, compared modulo 2^64) and "sha256 <digest of "abc">".
#include "crs_contribution.hip"
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

int main() {
    std::string s_delta, s_d, s_nonce, s_tag;
    std::cin >> s_delta >> s_d >> s_nonce >> s_tag;
    const std::vector<uint8_t> b_delta = unhex(s_delta), b_d = unhex(s_d), b_nonce = unhex(s_nonce), b_tag = unhex(s_tag);
    if (b_delta.size() != 64 || b_d.size() != 32 || b_nonce.size() != 32 || b_tag.size() != 32) { std::puts("bad request"); return 1; }
    auto delta = heap<uint64_t>(b_delta, 8), d = heap<uint64_t>(b_d, 4), nonce = heap<uint64_t>(b_nonce, 4);
    auto tag = heap<uint8_t>(b_tag, 32);
    std::unique_ptr<zk_crs_contribution> rec(new zk_crs_contribution);
    if (zk_crs_contribution_prove(delta.get(), d.get(), nonce.get(), tag.get(), rec.get()) != ZK_OK) { std::puts("prove failed"); return 1; }
    std::printf("record %s\n", hex(reinterpret_cast<const uint8_t*>(rec.get()), sizeof(zk_crs_contribution)).c_str());
    int ok = -1, tampered = -1, malformed = -1;
    if (zk_crs_contribution_verify(rec.get(), tag.get(), &ok) != ZK_OK) return 1;
    std::unique_ptr<zk_crs_contribution> bad(new zk_crs_contribution(*rec));
    bad->response[1] ^= 2;
    if (zk_crs_contribution_verify(bad.get(), tag.get(), &tampered) != ZK_OK) return 1;
    *bad = *rec;
    for (int i = 0; i < 8; ++i) bad->delta_after_g1[i] = i == 4 ? 1 : 0;
    if (zk_crs_contribution_verify(bad.get(), tag.get(), &malformed) != ZK_OK) return 1;
    std::printf("verify %d tampered %d malformed %d\n", ok, tampered, malformed);

    // the recoding: digits recompose to the halves (mod 2^64 is enough to catch a wrong digit: the low words see every carry) and stay
    // inside the struct; the scalars walk a SplitMix64 sequence reduced below r by clearing the top bits
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
        std::unique_ptr<zk::ScaleDigits> dg(new zk::ScaleDigits);
        zk::scalar_recode(k.get(), *dg);
        uint32_t k1[5], k2[5];
        bool n1, n2;
        zk::glv_split_host(k.get(), k1, n1, k2, n2);
        uint64_t s1 = 0, s2 = 0;
        for (int i = 0; i < 64 && i <= dg->top; ++i) { s1 += (uint64_t)(int64_t)dg->d1[i] << i; s2 += (uint64_t)(int64_t)dg->d2[i] << i; }
        const uint64_t m1 = k1[0] | ((uint64_t)k1[1] << 32), m2 = k2[0] | ((uint64_t)k2[1] << 32);
        if (s1 == (n1 ? 0 - m1 : m1) && s2 == (n2 ? 0 - m2 : m2) && dg->top < zk::SC_DIGITS) ++good;
    }
    std::printf("recoded %llu\n", (unsigned long long)good);

    zk::Sha256 h;
    h.update("abc", 3);
    uint8_t dgst[32];
    h.finish(dgst);
    std::printf("sha256 %s\n", hex(dgst, 32).c_str());
    return 0;
}
