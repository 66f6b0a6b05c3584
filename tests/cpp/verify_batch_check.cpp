// verify_batch_check.cpp -- groth16::verify_batch through the C++ host API (include/zksnark.hpp), built with g++ and linked
// against libzkgpu.so by tests/test_gpu_verify_batch.py.  simple.zk: honest proofs, a wrong public input, a flipped byte;
// prints one line "batch <verdicts>" and one line "single <verdicts>" (groth16::verify per proof), 1 / 0 per proof.
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
        for (int k = 0; k < 6; ++k) {
            groth16::Proof p = groth16::prove(ctx, qap, sigma, weights);
            if (k == 4) p.bytes[40] ^= 1;
            proofs.push_back(p);
            inputs.push_back({FrLocal(2), FrLocal(k == 2 ? 25 : 34)});
        }
        const std::vector<bool> batch = groth16::verify_batch(ctx, sigma, inputs, proofs);
        std::printf("batch");
        for (bool b : batch) std::printf(" %d", b ? 1 : 0);
        std::printf("\nsingle");
        for (size_t j = 0; j < proofs.size(); ++j) std::printf(" %d", groth16::verify(ctx, sigma, inputs[j], proofs[j]) ? 1 : 0);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
