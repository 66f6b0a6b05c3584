// builder_pack_api.cpp -- builder::Circuit::pack, Circuit::packed_wires and Boolgen::eval_fields of the C++ host API
// (include/zksnark.hpp).  Built with g++ and linked against libzkgpu.so by tests/test_cpp_builder_pack.py.  "host": the builder alone
// (no context, runs without a GPU); "gpu": bit-sliced witnesses with packed wires and the public inputs as field elements on the
// device.  Prints "ok <name>" per test and exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using builder::Gate;
using builder::WireId;
using builder::Word8;

#define ASSERT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static std::vector<FrLocal> bits_of(uint64_t v, int n) {
    std::vector<FrLocal> out;
    for (int i = 0; i < n; ++i) out.push_back(FrLocal((v >> i) & 1));
    return out;
}

static void pack_words_and_vectors() {
    builder::Circuit b;
    const Word8 x = b.new_word8(), y = b.new_word8();
    const Word8 both = b.u8_bitwise_op(x, y, Gate::Xor);
    const WireId px = b.pack(x);                                     // a Word8
    std::vector<WireId> wide(both.begin(), both.end());
    wide.push_back(b.unity_wire());
    wide.push_back(b.zero_wire());
    wide.push_back(x[0]);
    const WireId pw = b.pack(wide);                                  // a vector, constants and a repeated wire
    Circuit c = b.finish({pw, px});
    ASSERT(c.input() == 2 && c.is_boolean() && c.packed_wires() == 2 && c.gates() == 10 && c.wire_index(pw) == 1);
    for (uint64_t l : {0u, 5u, 200u, 255u})
        for (uint64_t r : {0u, 77u, 255u}) {
            auto in = bits_of(l, 8), in_r = bits_of(r, 8);
            in.insert(in.end(), in_r.begin(), in_r.end());
            const auto w = c.weights(in);
            ASSERT(w == c.weights_tape(in));
            ASSERT(w[1] == FrLocal((l ^ r) | 256 | ((l & 1) << 10)) && w[2] == FrLocal(l));
        }
    std::printf("ok pack_words_and_vectors\n");
}

static void pack_classification_and_refusals() {
    {
        builder::Circuit b;
        const Word8 x = b.new_word8();
        const WireId p = b.pack(x);
        b.new_and(p, x[0]);                                          // a packed wire that is read: legal, the circuit goes to the tape
        Circuit c = b.finish({p});
        ASSERT(!c.is_boolean() && c.packed_wires() == 1);
        ASSERT(c.weights(bits_of(0x81, 8))[1] == FrLocal(0x81));
    }
    builder::Circuit b;
    std::vector<WireId> many;
    for (int i = 0; i < 254; ++i) many.push_back(b.new_bit());
    int refused = 0;
    try { b.pack(many); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG && std::string(e.what()).find("253") != std::string::npos; }
    try { b.pack(std::vector<WireId>{}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    try { b.pack(std::vector<WireId>{many[0], 5000}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    many.pop_back();
    const WireId p = b.pack(many);
    Circuit c = b.finish({p});
    try { b.pack(many); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG && std::string(e.what()).find("finished") != std::string::npos; }
    ASSERT(refused == 4 && c.is_boolean() && c.packed_wires() == 1);
    Circuit parsed = ASTParser::try_parse("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n");
    ASSERT(parsed.packed_wires() == 0);
    std::printf("ok pack_classification_and_refusals\n");
}

// the three HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void packed_digest_on_the_device() {
    Context ctx;
    builder::Circuit b;
    auto msg = b.new_word8_vec(64);
    auto digest = b.keccak(msg, 136, 0x06, 2, 32);
    std::vector<WireId> lo, hi;
    for (int k = 0; k < 16; ++k) { lo.insert(lo.end(), digest[k].begin(), digest[k].end()); hi.insert(hi.end(), digest[16 + k].begin(), digest[16 + k].end()); }
    const WireId plo = b.pack(lo), phi = b.pack(hi);
    Circuit c = b.finish({plo, phi});
    ASSERT(c.input() == 2 && c.is_boolean() && c.packed_wires() == 2);
    const size_t m = c.wires(), count = 3;
    std::vector<uint8_t> in(count * 64);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (uint8_t)(i * 37 + 11);
    void *d_in = nullptr, *d_w = nullptr, *d_pub = nullptr;
    HIP_OK(hipMalloc(&d_in, in.size()));
    HIP_OK(hipMalloc(&d_w, count * m * 32));
    HIP_OK(hipMalloc(&d_pub, count * 3 * 32));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    Boolgen bg(ctx, c);
    bg.run(d_in, 64, count, d_w, m);
    bg.eval_fields(d_in, 64, count, {1, 2, 3}, d_pub);               // the two packed verify wires and the first input bit
    std::vector<FrLocal> pub(count * 3);
    HIP_OK(hipMemcpy(pub[0].w.data(), d_pub, count * 3 * 32, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < count; ++j) {
        std::vector<FrLocal> host_in;
        for (size_t i = 0; i < 64; ++i)
            for (int k = 0; k < 8; ++k) host_in.push_back(FrLocal((in[64 * j + i] >> k) & 1));
        const auto want = c.weights(host_in);
        std::vector<FrLocal> dev_w(m);
        HIP_OK(hipMemcpy(dev_w[0].w.data(), (const char*)d_w + j * m * 32, m * 32, hipMemcpyDeviceToHost));
        ASSERT(dev_w == want);
        ASSERT(pub[3 * j] == want[1] && pub[3 * j + 1] == want[2] && pub[3 * j + 2] == want[3]);
        ASSERT(want[1].w[2] == 0 && want[1].w[3] == 0 && (want[1].w[0] | want[1].w[1]) != 0);     // 128 bits of digest
    }
    bool refused = false;
    void* d_bits = nullptr;
    HIP_OK(hipMalloc(&d_bits, count));
    try { bg.eval(d_in, 64, count, {3, 1}, d_bits, 1); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG; }
    ASSERT(refused);
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_w)); HIP_OK(hipFree(d_pub)); HIP_OK(hipFree(d_bits));
    std::printf("ok packed_digest_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    pack_words_and_vectors();
    pack_classification_and_refusals();
    if (mode == "gpu") packed_digest_on_the_device();
    return 0;
}
