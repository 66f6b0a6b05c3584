// vk.hip -- the verifying key as a host object: zk_vk_create / _free / _dims / _bytes / _to_bytes / _from_bytes / _save / _load and
// zk_vk_verify.  Nothing in this file needs a context or a device (as zk_pairing / zk_proof_compress); the batch forms over a key,
// zk_vk_from_crs and the device side are vk_batch.hip.  tests/cpp/vk_host_fuzz.hip compiles this file alone for the host.
//
// Byte form (zk_vk_to_bytes and the file are the same bytes):
//   offset  0   "ZKVKv1\0\0"
//           8   l                                u64 LE
//          16   FNV-1a 64 of the payload         u64 LE   (the checksum of ZKCRSv1)
//          24   payload: alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | sum_gamma_g1[0..l], canonical little-endian words
#include "vk.hpp"
#include "verify_host.hpp"

namespace zk {
namespace {

constexpr char VK_MAGIC[8] = {'Z', 'K', 'V', 'K', 'v', '1', '\0', '\0'};

uint64_t vk_fnv1a(const uint8_t* p, size_t len) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// host-only calls have no context to keep a text in: the status is all they report
template <class Fn>
int host_guarded(Fn&& fn) {
    try {
        fn();
        return ZK_OK;
    } catch (const StatusError& e) {
        return e.status;
    } catch (const std::bad_alloc&) {
        return ZK_ERR_SIZE;   // a host allocation the size asked for did not get: nothing here touches HIP
    } catch (...) {
        return ZK_ERR_ARG;
    }
}

// the key of a payload: every point through zk_verify's readers, then what depends only on the points, once
zk_vk* vk_build(size_t l, std::vector<uint64_t>&& words) {
    auto vk = std::make_unique<zk_vk>();
    vk->input = l;
    vk->words = std::move(words);
    const uint64_t* w = vk->words.data();
    ZK_REQUIRE(rd_g1(w, vk->alpha) && rd_g2(w + 8, vk->beta) && rd_g2(w + 24, vk->gamma) && rd_g2(w + 40, vk->delta), ZK_ERR_RANGE,
               "vk: point out of range, not on the curve or outside G2");
    vk->sg.resize(l + 1);
    for (size_t i = 0; i <= l; ++i) ZK_REQUIRE(rd_g1(w + 56 + 8 * i, vk->sg[i]), ZK_ERR_RANGE, "vk: point out of range or not on the curve");
    vk->fx = std::make_unique<VbaFixed>();
    const G2A* qs[3] = {&vk->beta, &vk->gamma, &vk->delta};
    for (int q = 0; q < 3; ++q) {
        ml_lines(*qs[q], vk->fx->lines[q]);
        vk->fx->finite[q] = qs[q]->is_inf() ? 0 : 1;
    }
    vk->fx->t0_alpha = G1A::infinity();
    vk->c = ml_proj(vk->alpha, vk->beta);
    return vk.release();
}

// ZK_ERR_IO unless `in` is exactly one byte form; ZK_ERR_RANGE for a point zk_vk_create would refuse
zk_vk* vk_parse(const uint8_t* in, size_t len) {
    ZK_REQUIRE(len >= VK_HEAD_BYTES && !std::memcmp(in, VK_MAGIC, 8), ZK_ERR_IO, "vk: not a ZKVKv1 string");
    uint64_t l, sum;
    std::memcpy(&l, in + 8, 8);
    std::memcpy(&sum, in + 16, 8);
    ZK_REQUIRE(l <= len / 64 && zk_vk_bytes((size_t)l) == len, ZK_ERR_IO, "vk: length does not match the header");
    ZK_REQUIRE(vk_fnv1a(in + VK_HEAD_BYTES, len - VK_HEAD_BYTES) == sum, ZK_ERR_IO, "vk: checksum mismatch");
    std::vector<uint64_t> words(vk_payload_words((size_t)l));
    std::memcpy(words.data(), in + VK_HEAD_BYTES, words.size() * 8);
    return vk_build((size_t)l, std::move(words));
}

struct File {
    FILE* f;
    explicit File(FILE* f_) : f(f_) {}
    ~File() { if (f) std::fclose(f); }
};

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

size_t zk_vk_bytes(size_t input) { return VK_HEAD_BYTES + 8 * vk_payload_words(input); }

int zk_vk_create(const zk_vk_desc* desc, zk_vk** out) {
    if (!desc || !out || !desc->alpha_g1 || !desc->beta_g2 || !desc->gamma_g2 || !desc->delta_g2 || !desc->sum_gamma_g1) return ZK_ERR_ARG;
    *out = nullptr;
    return host_guarded([&] {
        const size_t l = desc->input;
        ZK_REQUIRE(l < ((size_t)1 << 40), ZK_ERR_SIZE, "vk: implausible input count");
        std::vector<uint64_t> words(vk_payload_words(l));
        std::memcpy(words.data(), desc->alpha_g1, 64);
        std::memcpy(words.data() + 8, desc->beta_g2, 128);
        std::memcpy(words.data() + 24, desc->gamma_g2, 128);
        std::memcpy(words.data() + 40, desc->delta_g2, 128);
        std::memcpy(words.data() + 56, desc->sum_gamma_g1, (l + 1) * 64);
        *out = vk_build(l, std::move(words));
    });
}

void zk_vk_free(zk_vk* vk) {
    if (!vk) return;
    if (vk->binding && vk->binding->alive && vk->binding->retire) vk->binding->retire(*vk->binding);
    delete vk;
}

int zk_vk_dims(const zk_vk* vk, size_t* input) {
    if (!vk || !input) return ZK_ERR_ARG;
    *input = vk->input;
    return ZK_OK;
}

int zk_vk_to_bytes(const zk_vk* vk, uint8_t* out, size_t len) {
    if (!vk || !out || len < zk_vk_bytes(vk->input)) return ZK_ERR_ARG;
    const uint64_t l = vk->input, sum = vk_fnv1a(reinterpret_cast<const uint8_t*>(vk->words.data()), vk->words.size() * 8);
    std::memcpy(out, VK_MAGIC, 8);
    std::memcpy(out + 8, &l, 8);
    std::memcpy(out + 16, &sum, 8);
    std::memcpy(out + VK_HEAD_BYTES, vk->words.data(), vk->words.size() * 8);
    return ZK_OK;
}

int zk_vk_from_bytes(const uint8_t* in, size_t len, zk_vk** out) {
    if (!in || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return host_guarded([&] { *out = vk_parse(in, len); });
}

int zk_vk_save(const zk_vk* vk, const char* path) {
    if (!vk || !path) return ZK_ERR_ARG;
    return host_guarded([&] {
        std::vector<uint8_t> buf(zk_vk_bytes(vk->input));
        ZK_REQUIRE(zk_vk_to_bytes(vk, buf.data(), buf.size()) == ZK_OK, ZK_ERR_ARG, "vk_save");
        File f(std::fopen(path, "wb"));
        ZK_REQUIRE(f.f, ZK_ERR_IO, "vk_save: cannot open the file");
        ZK_REQUIRE(std::fwrite(buf.data(), 1, buf.size(), f.f) == buf.size() && std::fflush(f.f) == 0, ZK_ERR_IO, "vk_save: short write");
    });
}

int zk_vk_load(const char* path, zk_vk** out) {
    if (!path || !out) return ZK_ERR_ARG;
    *out = nullptr;
    return host_guarded([&] {
        File f(std::fopen(path, "rb"));
        ZK_REQUIRE(f.f, ZK_ERR_IO, "vk_load: cannot open the file");
        ZK_REQUIRE(std::fseek(f.f, 0, SEEK_END) == 0, ZK_ERR_IO, "vk_load: cannot size the file");
        const long size = std::ftell(f.f);
        ZK_REQUIRE(size >= (long)VK_HEAD_BYTES && std::fseek(f.f, 0, SEEK_SET) == 0, ZK_ERR_IO, "vk_load: not a ZKVKv1 file");
        std::vector<uint8_t> buf((size_t)size);
        ZK_REQUIRE(std::fread(buf.data(), 1, buf.size(), f.f) == buf.size(), ZK_ERR_IO, "vk_load: short read");
        *out = vk_parse(buf.data(), buf.size());
    });
}

// zk_verify's verdict from the key: the same decoder, range rule and input sum (verify_host.hpp); the pairings of the fixed
// arguments go over the key's lines, e(alpha, beta) is the key's c, and the final exponentiation is the exact one the batch
// kernels use -- the lines differ from zk_verify's affine ones only by factors in Fq2, which the final exponentiation sends to 1.
int zk_vk_verify(const zk_vk* vk, const uint64_t* inputs, size_t n_inputs, const uint8_t proof[ZK_PROOF_BYTES], int* ok) {
    if (!vk || !proof || !ok || (n_inputs && !inputs)) return ZK_ERR_ARG;
    *ok = 0;
    return host_guarded([&] {
        G1A A, C, S;
        G2A B;
        if (!verify_decode_sum(vk->sg_words(), vk->input, inputs, n_inputs, proof, A, B, C, S)) return;
        const VbaFixed& fx = *vk->fx;
        Fq12 f = vk->c * ml_fixed(S, fx.lines[1], fx.finite[1] && !S.is_inf());
        f = f * ml_fixed(C, fx.lines[2], fx.finite[2] && !C.is_inf());
        f = f * ml_proj(A.neg(), B);
        *ok = final_exp_exact(f) == Fq12::one() ? 1 : 0;
    });
}

}  // extern "C"
