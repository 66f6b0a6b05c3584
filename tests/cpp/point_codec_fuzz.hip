// point_codec_fuzz.hip -- the host side of csrc/point_codec.cuh under AddressSanitizer and UndefinedBehaviorSanitizer: a
// stand-alone program, built and run by tests/test_proof_codec_host.py (hipcc --cuda-host-only -O0 -Xarch_host -fsanitize=address,undefined: the unoptimised build keeps the compile short).
// 1000 seeded 128-byte strings, shaped so that a useful share decodes (valid flags, coordinates mostly < q, some infinities),
// in heap buffers of the exact sizes so that a byte read or written past a block is reported.  Every string that decompresses
// must compress back to itself; every other one must leave 259 x 0xFF.  Prints "decompressed D of N, round trips R".
#include "point_codec.cuh"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace zk;

int main() {
    uint64_t s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    const size_t n = 1000;
    size_t ok_d = 0, ok_rt = 0;
    for (size_t it = 0; it < n; ++it) {
        std::vector<uint8_t> in(128), out(259), back(128);
        for (auto& b : in) b = (uint8_t)rnd();
        in[0] = (in[0] & 0x1f) | ((it & 1) ? 0x80 : 0xc0);
        in[32] &= 0x1f;
        in[96] = (in[96] & 0x1f) | 0x80;
        if (it % 7 == 0) { std::memset(in.data() + 32, 0, 64); in[32] = 0x40; }
        if (it % 11 == 0) { std::memset(in.data(), 0, 32); in[0] = 0x40; }
        if (it % 13 == 0) in[64] |= 0x80;   // a flag bit in x.c0's first byte: refused
        const bool d = proof_decompress(in.data(), out.data());
        ok_d += d;
        if (d) {
            ok_rt += proof_compress(out.data(), back.data()) && !std::memcmp(back.data(), in.data(), 128);
        } else {
            for (uint8_t b : out)
                if (b != 0xff) { std::puts("bad fill"); return 1; }
            out[0] = 4;   // and the refused 259 bytes, nearly: tag 0xFF blocks left in place
            if (proof_compress(out.data(), back.data())) { std::puts("0xFF blocks compressed"); return 1; }
        }
    }
    std::printf("decompressed %zu of %zu, round trips %zu\n", ok_d, n, ok_rt);
    return ok_d == ok_rt && ok_d > 10 ? 0 : 1;
}
