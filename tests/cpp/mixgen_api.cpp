// mixgen_api.cpp -- Circuit::mixed_dims, Circuit::weights_mixed and Mixgen of the C++ host API (include/zksnark.hpp).  Built with g++
// and linked against libzkgpu.so by tests/test_cpp_mixgen.py.  "host": the split and its host runner (no context, runs without a
// GPU); "gpu": the witnesses of a digest beside a field relation on the device.  Prints "ok <name>" per test and exits non-zero on the
// first failed assertion.
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

static FrLocal r_minus(uint64_t k) {
    FrLocal x;
    x.w = FrLocal::MODULUS;
    x.w[0] -= k;
    return x;
}

// x: 8 bits, f: a field input; p = pack(x ^ y-constant), g = x0 & f (field-class), t = (p + 3 f)(p + g)
static Circuit small_mixed() {
    builder::Circuit b;
    const Word8 x = b.new_word8();
    const WireId f = b.new_wire();
    const Word8 flipped = b.u8_bitwise_op(x, b.const_word8(0x5a), Gate::Xor);
    const WireId p = b.pack(flipped);
    const WireId g = b.new_and(x[0], f);
    const WireId t = b.new_sub_circuit({{FrLocal(1), p}, {FrLocal(3), f}}, {{FrLocal(1), p}, {FrLocal(1), g}});
    return b.finish({t, p});
}

static void split_and_host_runner() {
    Circuit c = small_mixed();
    const auto d = c.mixed_dims();
    ASSERT(!c.is_boolean() && d.n_bit_inputs == 8 && d.n_field_inputs == 1 && d.core_ops == 8 && d.core_levels == 1);
    ASSERT(d.tail_ops == 6 && d.tail_levels == 3);        // x0 f, the copy of p, 3 f | p + 3 f, p + g | the product
    ASSERT(d.tail_slots == 1 + 2 + 4);                    // f; g, t; the copy, 3 f and the two sums
    for (uint64_t x : {0u, 1u, 0x5au, 0xa5u, 0xffu})
        for (const FrLocal& f : {FrLocal(0), FrLocal(1), FrLocal(12345), r_minus(1)}) {
            std::vector<FrLocal> in;
            for (int i = 0; i < 8; ++i) in.push_back(FrLocal((x >> i) & 1));
            in.push_back(f);
            const auto want = c.weights(in);
            ASSERT(c.weights_mixed({(uint8_t)x}, {f}) == want && want == c.weights_tape(in));
            ASSERT(want[2] == FrLocal(x ^ 0x5a));
        }
    std::printf("ok split_and_host_runner\n");
}

static void refusals_and_boolean_circuits() {
    Circuit c = small_mixed();
    int refused = 0;
    try { c.weights_mixed({0}, {r_minus(0)}); } catch (const Error& e) { refused += e.status == ZK_ERR_RANGE; }
    try { c.weights_mixed({0, 0}, {FrLocal(1)}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG && std::string(e.what()).find("StructureErr") != std::string::npos; }
    try { c.weights_mixed({0}, {}); } catch (const Error& e) { refused += e.status == ZK_ERR_ARG; }
    Circuit parsed = ASTParser::try_parse("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n");
    try { parsed.mixed_dims(); } catch (const Error& e) { refused += e.status == ZK_ERR_UNSUPPORTED; }
    try { parsed.weights_mixed({}, {FrLocal(2), FrLocal(3)}); } catch (const Error& e) { refused += e.status == ZK_ERR_UNSUPPORTED; }
    ASSERT(refused == 5);
    builder::Circuit b;
    const Word8 x = b.new_word8(), y = b.new_word8();
    const Word8 z = b.u8_bitwise_op(x, y, Gate::Nand);                  // two sub-circuits per bit, two levels
    Circuit boolean = b.finish({b.pack(z)});
    const auto d = boolean.mixed_dims();
    ASSERT(boolean.is_boolean() && d.tail_ops == 0 && d.tail_slots == 0 && d.tail_levels == 0 && d.core_ops == 16 && d.core_levels == 2);
    std::vector<FrLocal> in;
    for (int i = 0; i < 16; ++i) in.push_back(FrLocal((0xc3a5u >> i) & 1));
    ASSERT(boolean.weights_mixed({0xa5, 0xc3}, {}) == boolean.weights(in));
    std::printf("ok refusals_and_boolean_circuits\n");
}

// the three HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void digest_beside_a_field_relation_on_the_device() {
    Context ctx;
    builder::Circuit b;
    auto msg = b.new_word8_vec(64);
    const WireId f = b.new_wire();
    auto digest = b.keccak(msg, 136, 0x06, 2, 32);
    std::vector<WireId> lo, hi;
    for (int k = 0; k < 16; ++k) { lo.insert(lo.end(), digest[k].begin(), digest[k].end()); hi.insert(hi.end(), digest[16 + k].begin(), digest[16 + k].end()); }
    const WireId plo = b.pack(lo), phi = b.pack(hi);
    WireId t = b.new_sub_circuit({{FrLocal(1), plo}, {FrLocal(1), f}}, {{FrLocal(1), phi}});
    for (int k = 0; k < 3; ++k) t = b.new_sub_circuit({{FrLocal(1), t}}, {{FrLocal(1), t}, {FrLocal(1), plo}});
    Circuit c = b.finish({t, plo, phi});
    const auto d = c.mixed_dims();
    ASSERT(c.input() == 3 && !c.is_boolean() && d.n_bit_inputs == 512 && d.n_field_inputs == 1 && d.core_ops == c.gates() - 6);
    const size_t m = c.wires(), count = 67;
    std::vector<uint8_t> in(count * 64);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (uint8_t)(i * 37 + 11);
    std::vector<FrLocal> fields(count);
    for (size_t j = 0; j < count; ++j) fields[j] = j == 0 ? r_minus(1) : FrLocal(j * 0x9e3779b97f4a7c15ull);
    void *d_in = nullptr, *d_f = nullptr, *d_w = nullptr, *d_pub = nullptr;
    HIP_OK(hipMalloc(&d_in, in.size()));
    HIP_OK(hipMalloc(&d_f, count * 32));
    HIP_OK(hipMalloc(&d_w, count * m * 32));
    HIP_OK(hipMalloc(&d_pub, count * 3 * 32));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_f, fields[0].w.data(), count * 32, hipMemcpyHostToDevice));
    Mixgen mg(ctx, c);
    mg.run(d_in, 64, d_f, count, d_w, m);
    mg.eval_fields(d_in, 64, d_f, count, {3, 1, 2}, d_pub);
    std::vector<FrLocal> pub(count * 3);
    HIP_OK(hipMemcpy(pub[0].w.data(), d_pub, count * 3 * 32, hipMemcpyDeviceToHost));
    for (size_t j : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, count - 1}) {
        const auto want = c.weights_mixed(std::vector<uint8_t>(in.begin() + 64 * j, in.begin() + 64 * j + 64), {fields[j]});
        std::vector<FrLocal> dev_w(m);
        HIP_OK(hipMemcpy(dev_w[0].w.data(), (const char*)d_w + j * m * 32, m * 32, hipMemcpyDeviceToHost));
        ASSERT(dev_w == want);
        ASSERT(pub[3 * j] == want[3] && pub[3 * j + 1] == want[1] && pub[3 * j + 2] == want[2]);
    }
    bool refused = false;
    fields[5] = r_minus(0);
    HIP_OK(hipMemcpy(d_f, fields[0].w.data(), count * 32, hipMemcpyHostToDevice));
    try { mg.run(d_in, 64, d_f, count, d_w, m); } catch (const Error& e) { refused = e.status == ZK_ERR_RANGE && std::string(e.what()).find("instance 5") != std::string::npos; }
    ASSERT(refused);
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_f)); HIP_OK(hipFree(d_w)); HIP_OK(hipFree(d_pub));
    std::printf("ok digest_beside_a_field_relation_on_the_device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    split_and_host_runner();
    refusals_and_boolean_circuits();
    if (mode == "gpu") digest_beside_a_field_relation_on_the_device();
    return 0;
}
