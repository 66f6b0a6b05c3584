// tests/cpp/pairing_check.hip -- the device pairing code of csrc/pairing.cuh (__host__ __device__) compiled for the HOST and
// driven from tests/test_pairing_device_code.py:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -I zksnark_rs_amd/csrc tests/cpp/pairing_check.hip -o pairing_check
// stdin, one request per line, numbers as 64-bit hex words (canonical, little-endian limbs):
//   pair <8 words: P> <16 words: Q>   -> FE(ml_proj(P, Q)) and FE(ml_fixed(P, lines(Q))), 48 words each
//   fe <48 words: x in Fq12>          -> final_exp_exact(x) and x^((q^12 - 1) / r) by square-and-multiply, 48 words each
// A point off its curve or outside G2 prints "bad".
#include <cstdio>
#include <cstring>
#include <vector>
#include "pairing.cuh"

using namespace zk;

static Fq fq_canon(const uint64_t* w) { return Fq::from_canonical(fq_from_u64x4(w)); }
static void put(const Fq12& f) {
    const Fq2* parts[6] = {&f.c0.a0, &f.c0.a1, &f.c0.a2, &f.c1.a0, &f.c1.a1, &f.c1.a2};
    for (int k = 0; k < 6; ++k) {
        const Fq c[2] = {parts[k]->c0.to_canonical(), parts[k]->c1.to_canonical()};
        for (int h = 0; h < 2; ++h)
            for (int i = 0; i < 4; ++i) std::printf(" %016llx", (unsigned long long)((uint64_t)c[h].l[2 * i] | ((uint64_t)c[h].l[2 * i + 1] << 32)));
    }
    std::printf("\n");
}
static bool read_words(uint64_t* w, int n) {
    for (int i = 0; i < n; ++i) {
        unsigned long long v;
        if (std::scanf("%llx", &v) != 1) return false;
        w[i] = v;
    }
    return true;
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "pair")) {
            uint64_t a[8], b[16];
            if (!read_words(a, 8) || !read_words(b, 16)) return 2;
            G1A P;
            G2A Q;
            if (!rd_g1(a, P) || !rd_g2(b, Q)) { std::printf("bad\nbad\n"); continue; }
            put(final_exp_exact(ml_proj(P, Q)));
            std::vector<Line> lines(ATE_LINES);
            ml_lines(Q, lines.data());
            put(final_exp_exact(ml_fixed(P, lines.data(), !P.is_inf() && !Q.is_inf())));
        } else if (!std::strcmp(cmd, "fe")) {
            uint64_t w[48];
            if (!read_words(w, 48)) return 2;
            Fq2 c[6];
            for (int k = 0; k < 6; ++k) c[k] = Fq2{fq_canon(w + 8 * k), fq_canon(w + 8 * k + 4)};
            const Fq12 x{Fq6{c[0], c[1], c[2]}, Fq6{c[3], c[4], c[5]}};
            put(final_exp_exact(x));
            put(x.pow_words(FINAL_EXP, FINAL_EXP_WORDS));
        } else {
            return 2;
        }
        std::fflush(stdout);
    }
    return 0;
}
