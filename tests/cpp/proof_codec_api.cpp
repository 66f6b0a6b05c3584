// proof_codec_api.cpp -- groth16::compress / decompress / verify_batch_compressed through the C++ host API
// (include/zksnark.hpp), built with g++ and linked against libzkgpu.so by tests/test_gpu_proof_codec.py.  simple.zk: four honest
// proofs, one with a wrong public input, one with A's sign flag flipped, one malformed string.  Prints
//   roundtrip <1 per proof whose decompress(compress(p)) == p>
//   compressed <verdicts of verify_batch_compressed>
//   plain <verdicts of verify_batch on the decompressed proofs, 0 where decompress throws>
//   refused <status of decompress on the malformed string> <status of compress on a proof with A off its curve>
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
        std::vector<groth16::CompressedProof> packed;
        std::vector<std::vector<FrLocal>> inputs;
        std::printf("roundtrip");
        for (int k = 0; k < 6; ++k) {
            const groth16::Proof p = groth16::prove(ctx, qap, sigma, weights);
            groth16::CompressedProof c = groth16::compress(p);
            std::printf(" %d", groth16::decompress(c) == p ? 1 : 0);
            if (k == 3) c.bytes[0] ^= 0x40;    // the other y: still a point, no longer the proof's A
            if (k == 4) c.bytes[32] &= 0x3f;   // flag 00 on B
            packed.push_back(c);
            inputs.push_back({FrLocal(2), FrLocal(k == 2 ? 25 : 34)});
        }
        const std::vector<bool> got = groth16::verify_batch_compressed(ctx, sigma, inputs, packed);
        std::printf("\ncompressed");
        for (bool b : got) std::printf(" %d", b ? 1 : 0);
        std::printf("\nplain");
        int refused = 0;
        for (size_t j = 0; j < packed.size(); ++j) {
            bool ok = false;
            try {
                ok = groth16::verify_batch(ctx, sigma, {inputs[j]}, {groth16::decompress(packed[j])})[0];
            } catch (const Error& e) {
                refused = e.status;
            }
            std::printf(" %d", ok ? 1 : 0);
        }
        groth16::Proof off = groth16::decompress(packed[0]);
        off.bytes[64] ^= 1;   // A.y changed: off the curve
        int refused_c = 0;
        try {
            groth16::compress(off);
        } catch (const Error& e) {
            refused_c = e.status;
        }
        std::printf("\nrefused %d %d\n", refused, refused_c);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
