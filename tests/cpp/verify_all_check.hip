// tests/cpp/verify_all_check.hip -- zk_verify_batch_all's per-lane step and final combination (csrc/verify_all.cuh,
// __host__ __device__) compiled for the HOST and driven from tests/test_verify_all_device_code.py:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -I zksnark_rs_amd/csrc tests/cpp/verify_all_check.hip -o verify_all_check
// stdin, numbers as 64-bit hex words (canonical, little-endian limbs):
//   crs <k> <8 words: alpha> <16: beta> <16: gamma> <16: delta> <(k + 1) x 8: sum_gamma>
//   batch <n> then n times: <518 hex digits: the proof bytes> <2 words: z> <k x 4 words: inputs>
//     -> "ok <0|1>" and "t <(k + 1) x 4 words>" (t_0 = sum z_j, t_i = sum z_j x_ji mod r, canonical)
// The lanes are combined as a tree over pairs, as the device's reductions do; a CRS point the reader refuses prints "bad".
#include <cstdio>
#include <cstring>
#include <vector>
#include "verify_all.cuh"

using namespace zk;
static constexpr size_t PROOF_BYTES = 259;   // A | B | C: 65 + 129 + 65

static bool read_words(uint64_t* w, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        unsigned long long v;
        if (std::scanf("%llx", &v) != 1) return false;
        w[i] = v;
    }
    return true;
}
static bool read_bytes(uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        unsigned v;
        if (std::scanf("%2x", &v) != 1) return false;
        p[i] = (uint8_t)v;
    }
    return true;
}
static void put_fr(const Fr& x) {
    for (int i = 0; i < 4; ++i) std::printf(" %016llx", (unsigned long long)((uint64_t)x.l[2 * i] | ((uint64_t)x.l[2 * i + 1] << 32)));
}
// the values combined pairwise, level by level, until one is left
static VbaAcc tree(std::vector<VbaAcc> v) {
    if (v.empty()) return vba_identity();
    while (v.size() > 1) {
        std::vector<VbaAcc> next;
        for (size_t i = 0; i < v.size(); i += 2) next.push_back(i + 1 < v.size() ? vba_combine(v[i], v[i + 1]) : v[i]);
        v.swap(next);
    }
    return v[0];
}

int main() {
    char cmd[16];
    size_t k = 0;
    G1A alpha;
    G2A q[3];
    std::vector<G1A> sg;
    bool crs_ok = false;
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "crs")) {
            unsigned long long kk;
            if (std::scanf("%llu", &kk) != 1) return 2;
            k = kk;
            uint64_t w[16];
            if (!read_words(w, 8)) return 2;
            crs_ok = rd_g1(w, alpha);
            for (int i = 0; i < 3; ++i) {
                if (!read_words(w, 16)) return 2;
                crs_ok = rd_g2(w, q[i]) && crs_ok;
            }
            sg.assign(k + 1, G1A::infinity());
            for (size_t i = 0; i <= k; ++i) {
                if (!read_words(w, 8)) return 2;
                crs_ok = rd_g1(w, sg[i]) && crs_ok;
            }
        } else if (!std::strcmp(cmd, "batch")) {
            unsigned long long n;
            if (std::scanf("%llu", &n) != 1) return 2;
            std::vector<VbaAcc> lanes;
            std::vector<Fr> t(k + 1, Fr::zero());
            uint8_t proof[PROOF_BYTES];
            std::vector<uint64_t> x(4 * k);
            for (size_t j = 0; j < n; ++j) {
                uint64_t z[2];
                if (!read_bytes(proof, PROOF_BYTES) || !read_words(z, 2) || !read_words(x.data(), 4 * k)) return 2;
                const uint32_t zw[4] = {(uint32_t)z[0], (uint32_t)(z[0] >> 32), (uint32_t)z[1], (uint32_t)(z[1] >> 32)};
                lanes.push_back(vba_lane(proof, zw));
                Fr zc = Fr::zero();
                for (int h = 0; h < 4; ++h) zc.l[h] = zw[h];
                t[0] = t[0] + zc;   // z < 2^128: canonical as it is
                const Fr zm = vba_z_mont(zw);
                for (size_t i = 0; i < k; ++i) t[i + 1] = t[i + 1] + vba_zx(zm, x.data() + 4 * i);
            }
            if (!crs_ok) { std::printf("bad\n"); continue; }
            std::vector<VbaAcc> terms(k + 1, vba_identity());
            for (size_t i = 0; i <= k; ++i) terms[i].c = vba_ts_term(t[i], sg[i]);
            VbaFixed* fx = new VbaFixed;
            for (int i = 0; i < 3; ++i) {
                ml_lines(q[i], fx->lines[i]);
                fx->finite[i] = q[i].is_inf() ? 0 : 1;
            }
            fx->t0_alpha = jac_to_affine(g1_mul_bits(alpha, t[0].l, 256));
            const bool ok = vba_finish(tree(lanes), tree(terms).c, *fx);
            delete fx;
            std::printf("ok %d\nt", ok ? 1 : 0);
            for (const Fr& v : t) put_fr(v);
            std::printf("\n");
        } else {
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
