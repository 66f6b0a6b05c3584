// vk_api.cpp -- groth16::VerifyingKey through the C++ host API (include/zksnark.hpp), built with g++ and linked against
// libzkgpu.so by tests/test_gpu_vk.py.  simple.zk: honest proofs, a wrong public input, a flipped byte.  Prints verdict lines
// (1 / 0 per proof): "batch" (key on the GPU), "single" (key on the host), "crs" (groth16::verify_batch over sigma),
// "compressed", "restored" (a key through save / load, on the GPU); "all" / "all_honest" (one verdict), "sums_equal" (input sums
// with and without tables), "other_context" (status of a bound key on a second context).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;

static void line(const char* name, const std::vector<bool>& v) {
    std::printf("%s", name);
    for (bool b : v) std::printf(" %d", b ? 1 : 0);
    std::printf("\n");
}

int main(int argc, char** argv) {
    std::ifstream f(argc > 1 ? argv[1] : "tests/golden/zk/simple.zk");
    const std::string path = argc > 2 ? argv[2] : "key.zkvk";
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string code = ss.str();
    try {
        Context ctx(0);
        QAP qap = QAP::from(ctx, ASTParser::try_parse(code));
        auto weights = groth16::weights(code, {3, 2, 4});
        auto sigma = groth16::setup(ctx, qap);
        std::vector<groth16::Proof> proofs, honest;
        std::vector<std::vector<FrLocal>> inputs, good_inputs;
        for (int k = 0; k < 6; ++k) {
            groth16::Proof p = groth16::prove(ctx, qap, sigma, weights);
            honest.push_back(p);
            good_inputs.push_back({FrLocal(2), FrLocal(34)});
            if (k == 4) p.bytes[40] ^= 1;
            proofs.push_back(p);
            inputs.push_back({FrLocal(2), FrLocal(k == 2 ? 25 : 34)});
        }
        groth16::VerifyingKey key = groth16::VerifyingKey::from_sigma(ctx, sigma);
        if (key.input() != 2 || key.to_bytes().size() != zk_vk_bytes(2)) return 2;
        line("batch", key.verify_batch(ctx, inputs, proofs));
        std::vector<bool> single;
        for (size_t j = 0; j < proofs.size(); ++j) single.push_back(key.verify(inputs[j], proofs[j]));
        line("single", single);
        line("crs", groth16::verify_batch(ctx, sigma, inputs, proofs));
        // the compressed call: the flipped byte leaves no point on the curve, so that entry is compressed from the honest proof and
        // spoilt afterwards
        std::vector<groth16::CompressedProof> comp;
        for (size_t j = 0; j < proofs.size(); ++j) {
            comp.push_back(groth16::compress(honest[j]));
            if (j == 4) comp.back().bytes[40] ^= 1;
        }
        line("compressed", key.verify_batch_compressed(ctx, inputs, comp));
        key.save(path);
        groth16::VerifyingKey restored = groth16::VerifyingKey::load(path);
        if (restored.to_bytes() != key.to_bytes() || groth16::VerifyingKey::from_bytes(key.to_bytes()).to_bytes() != key.to_bytes()) return 3;
        line("restored", restored.verify_batch(ctx, inputs, proofs));
        std::printf("all %d\n", key.verify_batch_all(ctx, inputs, proofs) ? 1 : 0);
        std::printf("all_honest %d\n", key.verify_batch_all(ctx, good_inputs, honest) ? 1 : 0);
        std::printf("sums_equal %d\n", key.input_sums(ctx, inputs, true) == key.input_sums(ctx, inputs, false) ? 1 : 0);
        {
            Context second(0);
            int status = 0;
            try {
                key.verify_batch(second, inputs, proofs);
            } catch (const Error& e) {
                status = e.status;
            }
            std::printf("other_context %d\n", status);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
