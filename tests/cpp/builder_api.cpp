// builder_api.cpp -- zksnark::builder::Circuit and zksnark::Boolgen of the C++ host API (include/zksnark.hpp).  Built with g++ and
// linked against libzkgpu.so by tests/test_cpp_builder.py.  "host": the builder alone (no context, runs without a GPU); "gpu": packed
// witnesses, proof and verification on the device.  Prints "ok <name>" per test and exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using builder::Gate;
using builder::WireId;
using builder::Word64;
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

static void gates_and_comparators() {
    builder::Circuit b;
    const Word8 x = b.new_word8(), y = b.new_word8();
    ASSERT(x[0] == 2 && y[7] == 17 && b.unity_wire() == 1 && b.zero_wire() == 0);
    const Word8 both = b.u8_bitwise_op(x, y, Gate::Xor);
    const WireId parity = b.fan_in(both, Gate::Xor);
    const WireId leq = b.less_than_eq(x, y);
    const WireId is5 = b.is_equal(x, b.const_word8(5));
    const WireId nor = b.new_nor(x[0], y[0]);
    b.assert_bit(x[0]);
    ASSERT(b.gates() > 8 + 7 + 8 + 1);
    Circuit c = b.finish({leq, parity, is5, nor});
    ASSERT(c.input() == 4 && c.assignments() == 16 && c.is_boolean() && c.wire_index(leq) == 1 && c.wire_index(x[0]) == 5);
    for (uint64_t l : {0u, 5u, 200u, 255u})
        for (uint64_t r : {0u, 5u, 201u, 255u}) {
            auto in = bits_of(l, 8), in_r = bits_of(r, 8);
            in.insert(in.end(), in_r.begin(), in_r.end());
            const auto w = c.weights(in);
            ASSERT(w == c.weights_tape(in));
            ASSERT(w[0] == FrLocal(1) && w[1] == FrLocal(l <= r) && w[2] == FrLocal(__builtin_parityll(l ^ r)) && w[3] == FrLocal(l == 5));
            ASSERT(w[4] == FrLocal(!((l | r) & 1)));
        }
    bool refused = false;
    try { b.new_and(2, 3); } catch (const Error& e) { refused = e.status == ZK_ERR_ARG && std::string(e.what()).find("finished") != std::string::npos; }
    ASSERT(refused);
    std::printf("ok gates_and_comparators\n");
}

static void general_sub_circuit() {
    builder::Circuit b;
    const WireId x = b.new_wire(), y = b.new_bit();
    const WireId t = b.new_sub_circuit({{FrLocal(3), x}, {FrLocal(2), b.unity_wire()}}, {{FrLocal(1), y}, {FrLocal(1), b.unity_wire()}});
    Circuit c = b.finish({t});
    ASSERT(!c.is_boolean());
    ASSERT((c.weights({FrLocal(10), FrLocal(1)}) == std::vector<FrLocal>{1, 64, 10, 1}));
    bool refused = false;
    try { c.weights({FrLocal(10), FrLocal(2)}); } catch (const Error& e) { refused = e.status == ZK_ERR_RANGE; }
    ASSERT(refused);
    std::printf("ok general_sub_circuit\n");
}

static void keccak_counts() {
    builder::Circuit b;
    auto msg = b.new_word8_vec(56);
    auto digest = b.keccak256(msg);
    ASSERT(b.gates() == 232400);
    const Word64 xw = b.new_word64(), yw = b.new_word64(), lo = b.new_word64(), hi = b.new_word64(), cw = b.new_word64();
    const size_t before = b.gates();
    auto vo = b.validate_order(xw, {lo, hi}, yw, cw);
    ASSERT(b.gates() - before > 8 * 16 + 16 + 9664 * 24);
    std::vector<WireId> verify{vo.is_x_within_range, vo.is_y_greater_than_c};
    for (const auto& w8 : digest) verify.insert(verify.end(), w8.begin(), w8.end());
    Circuit c = b.finish(verify);
    ASSERT(c.input() == 258 && c.is_boolean());
    std::printf("ok keccak_counts\n");
}

// the three HIP runtime calls the device test needs (libamdhip64), declared here so that the program builds with plain g++
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
}
enum { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
#define HIP_OK(expr) ASSERT((expr) == 0)

static void packed_witnesses_prove_and_verify() {
    Context ctx;
    builder::Circuit b;
    auto msg = b.new_word8_vec(64);
    auto digest = b.keccak(msg, 136, 0x06, 2, 32);
    std::vector<WireId> verify;
    for (const auto& w8 : digest) verify.insert(verify.end(), w8.begin(), w8.end());
    Circuit c = b.finish(verify);
    ASSERT(c.gates() == 8 * 64 + 16 + 2 * 9664);
    const size_t m = c.wires(), count = 2;
    std::vector<uint8_t> in(count * 64);
    for (size_t i = 0; i < in.size(); ++i) in[i] = (uint8_t)(i * 37 + 11);
    void *d_in = nullptr, *d_w = nullptr, *d_dig = nullptr;
    HIP_OK(hipMalloc(&d_in, in.size()));
    HIP_OK(hipMalloc(&d_w, count * m * 32));
    HIP_OK(hipMalloc(&d_dig, count * 32));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    Boolgen bg(ctx, c);
    bg.run(d_in, 64, count, d_w, m);
    std::vector<uint32_t> wires(256);
    for (uint32_t i = 0; i < 256; ++i) wires[i] = i + 1;
    bg.eval(d_in, 64, count, wires, d_dig, 32);
    std::vector<uint8_t> dig(count * 32);
    HIP_OK(hipMemcpy(dig.data(), d_dig, dig.size(), hipMemcpyDeviceToHost));
    // the packed digest is the witness's verify wires
    std::vector<FrLocal> host_in;
    for (size_t i = 0; i < 64; ++i)
        for (int k = 0; k < 8; ++k) host_in.push_back(FrLocal((in[64 + i] >> k) & 1));
    const auto w1 = c.weights(host_in);
    std::vector<FrLocal> public1;
    for (size_t i = 0; i < 256; ++i) {
        ASSERT(w1[1 + i] == FrLocal((dig[32 + i / 8] >> (i % 8)) & 1));
        public1.push_back(w1[1 + i]);
    }
    std::vector<FrLocal> dev_w(m);
    HIP_OK(hipMemcpy(dev_w[0].w.data(), (const char*)d_w + m * 32, m * 32, hipMemcpyDeviceToHost));
    ASSERT(dev_w == w1);
    QAP qap = QAP::from_sparse_unity(ctx, c);
    ASSERT(qap.degree() == 32768 && groth16::is_satisfied(ctx, qap, dev_w));
    auto sigma = groth16::setup(ctx, qap);
    auto proof = groth16::prove(ctx, qap, sigma, dev_w);
    ASSERT(groth16::verify(ctx, sigma, public1, proof));
    public1[9] = FrLocal(1) == public1[9] ? FrLocal(0) : FrLocal(1);
    ASSERT(!groth16::verify(ctx, sigma, public1, proof));
    bool refused = false;
    try { Circuit parsed = ASTParser::try_parse("(in a b)\n(out c)\n(verify c)\n(program\n  (= c (* a b)))\n"); Boolgen no(ctx, parsed); }
    catch (const Error& e) { refused = e.status == ZK_ERR_UNSUPPORTED; }
    ASSERT(refused);
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_w)); HIP_OK(hipFree(d_dig));
    std::printf("ok packed_witnesses_prove_and_verify\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    gates_and_comparators();
    general_sub_circuit();
    keccak_counts();
    if (mode == "gpu") packed_witnesses_prove_and_verify();
    return 0;
}
