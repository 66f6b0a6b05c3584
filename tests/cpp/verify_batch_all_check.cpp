// verify_batch_all_check.cpp -- groth16::verify_batch_all / verify_batch_all_with through the C++ host API
// (include/zksnark.hpp), built with g++ and linked against libzkgpu.so by tests/test_gpu_verify_batch_all.py.  simple.zk: four
// honest proofs, then the same with a wrong public input, then with a flipped byte; prints one line per batch,
// "<name> <batch_all> <batch_all_with z = 1..n> <every verify_batch entry>", 1 / 0.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;

int main(int argc, char** argv) {
    std::ifstream f(argc > 1 ? argv[1] : "tests/golden/zk/simple.zk");
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string code = ss.str();
    try {
        Context ctx(0);
        QAP qap = QAP::from(ctx, ASTParser::try_parse(code));
        auto weights = groth16::weights(code, {3, 2, 4});
        auto sigma = groth16::setup(ctx, qap);
        std::vector<groth16::Proof> proofs;
        std::vector<std::vector<FrLocal>> inputs;
        std::vector<std::array<uint64_t, 2>> z;
        for (int k = 0; k < 4; ++k) {
            proofs.push_back(groth16::prove(ctx, qap, sigma, weights));
            inputs.push_back({FrLocal(2), FrLocal(34)});
            z.push_back({(uint64_t)k + 1, 0});
        }
        const char* names[3] = {"honest", "wrong_input", "flipped_byte"};
        for (int c = 0; c < 3; ++c) {
            auto in = inputs;
            auto pf = proofs;
            if (c == 1) in[2] = {FrLocal(2), FrLocal(25)};
            if (c == 2) pf[1].bytes[40] ^= 1;
            std::printf("%s %d %d", names[c], groth16::verify_batch_all(ctx, sigma, in, pf) ? 1 : 0,
                        groth16::verify_batch_all_with(ctx, sigma, in, pf, z) ? 1 : 0);
            for (bool b : groth16::verify_batch(ctx, sigma, in, pf)) std::printf(" %d", b ? 1 : 0);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
