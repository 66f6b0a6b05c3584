// vk_host_fuzz.hip -- csrc/vk.hip (the verifying key as a host object) under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, built and run by tests/test_vk_host.py (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined).
// stdin: the byte form of a key (hex) | a proof it accepts (hex) | "l" and the input row as hex words ("-" for none).
// Every malformed variant of the byte form goes through zk_vk_from_bytes in a heap buffer of its exact size, so that a byte read
// past the string is reported; then the proof and a tampered copy go through zk_vk_verify.
// Prints "malformed N" (variants refused with the expected status) and "verify V tampered T".
#include "vk.hip"
#include <iostream>
#include <string>

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}

static int from_bytes_status(const std::vector<uint8_t>& v) {
    // exact-size heap copy; an empty string still needs a non-null pointer
    std::unique_ptr<uint8_t[]> buf(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(buf.get(), v.data(), v.size());
    zk_vk* k = nullptr;
    const int rc = zk_vk_from_bytes(buf.get(), v.size(), &k);
    if (rc == ZK_OK) zk_vk_free(k);
    else if (k) return 12345;   // *out must stay NULL
    return rc;
}

static std::vector<uint8_t> with_checksum(std::vector<uint8_t> v) {
    const uint64_t sum = zk::vk_fnv1a(v.data() + 24, v.size() - 24);
    std::memcpy(v.data() + 16, &sum, 8);
    return v;
}

int main() {
    std::string key_hex, proof_hex, l_str, row_hex;
    std::cin >> key_hex >> proof_hex >> l_str >> row_hex;
    const std::vector<uint8_t> good = unhex(key_hex), proof = unhex(proof_hex);
    const size_t l = std::stoul(l_str);
    if (proof.size() != ZK_PROOF_BYTES || good.size() != zk_vk_bytes(l)) { std::puts("bad request"); return 1; }
    if (from_bytes_status(good) != ZK_OK) { std::puts("the honest key was refused"); return 1; }

    int refused = 0, wrong = 0;
    auto expect = [&](const std::vector<uint8_t>& v, int status) {
        if (from_bytes_status(v) == status) ++refused; else ++wrong;
    };
    for (size_t cut : {(size_t)0, (size_t)7, (size_t)8, (size_t)23, (size_t)24, good.size() / 2, good.size() - 1})
        expect(std::vector<uint8_t>(good.begin(), good.begin() + cut), ZK_ERR_IO);
    { auto v = good; v.push_back(0); expect(v, ZK_ERR_IO); }
    { auto v = good; v[5] = '2'; expect(v, ZK_ERR_IO); }
    { auto v = good; v[24 + 40] ^= 0x10; expect(v, ZK_ERR_IO); }
    { auto v = good; v[17] ^= 1; expect(v, ZK_ERR_IO); }
    for (uint64_t claimed : {(uint64_t)l + 1, (uint64_t)1 << 61, ~(uint64_t)0, (uint64_t)1 << 32}) {
        auto v = good;
        std::memcpy(v.data() + 8, &claimed, 8);
        expect(v, ZK_ERR_IO);
    }
    // points moved off their curves / out of range, checksum recomputed: alpha, beta, gamma, delta, the first and last base
    for (size_t word : {(size_t)0, (size_t)8, (size_t)24, (size_t)40, (size_t)56, (size_t)56 + 8 * l}) {
        auto v = good;
        v[24 + 8 * word] ^= 1;
        expect(with_checksum(v), ZK_ERR_RANGE);
        auto w = good;
        std::memset(w.data() + 24 + 8 * word, 0xff, 32);   // a coordinate >= q
        expect(with_checksum(w), ZK_ERR_RANGE);
    }
    std::printf("malformed %d\n", refused);
    if (wrong) { std::printf("%d variants answered with another status\n", wrong); return 1; }

    zk_vk* key = nullptr;
    if (zk_vk_from_bytes(good.data(), good.size(), &key) != ZK_OK) return 1;
    std::vector<uint8_t> rowb = row_hex == "-" ? std::vector<uint8_t>() : unhex(row_hex);
    std::vector<uint64_t> row(rowb.size() / 8);
    if (!rowb.empty()) std::memcpy(row.data(), rowb.data(), rowb.size());
    int ok = -1, bad = -1;
    if (zk_vk_verify(key, row.data(), row.size() / 4, proof.data(), &ok) != ZK_OK) return 1;
    std::vector<uint8_t> swapped(proof.begin() + 194, proof.end());
    swapped.insert(swapped.end(), proof.begin() + 65, proof.begin() + 194);
    swapped.insert(swapped.end(), proof.begin(), proof.begin() + 65);
    if (zk_vk_verify(key, row.data(), row.size() / 4, swapped.data(), &bad) != ZK_OK) return 1;
    // the byte form out again, into a buffer of the exact size
    std::vector<uint8_t> back(good.size());
    if (zk_vk_to_bytes(key, back.data(), back.size()) != ZK_OK || back != good) { std::puts("round trip differs"); return 1; }
    zk_vk_free(key);
    std::printf("verify %d tampered %d\n", ok, bad);
    return 0;
}
