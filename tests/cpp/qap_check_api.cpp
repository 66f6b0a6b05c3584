// qap_check_api.cpp -- groth16::is_satisfied / which_is_unsatisfied of the C++ host API (include/zksnark.hpp) on simple.zk.
// Built with g++ and linked against libzkgpu.so by tests/test_qap_check_host.py (compiles and links) and run by
// tests/test_gpu_qap_check.py (-m gpu); prints "ok" and exits non-zero on the first failed assertion.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;

static_assert(sizeof(zk_qap_check_result) == 12, "zk_qap_check_result is three 32-bit words");

#define ASSERT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <path to simple.zk>\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string code = ss.str();   // x = 4ab + c + 6: gate 0 is temp = a b, gate 1 (the last) is x = 1 (4 temp + c + 6)

    Context ctx;
    Circuit circuit = ASTParser::try_parse(code);
    QAP qap = QAP::from_sparse(ctx, circuit);
    auto weights = groth16::weights(code, {3, 2, 4});   // a, b, c
    ASSERT((weights == std::vector<FrLocal>{1, 2, 34, 6, 3, 4}));
    ASSERT(groth16::is_satisfied(ctx, qap, weights));
    ASSERT(!groth16::which_is_unsatisfied(ctx, qap, weights).has_value());

    auto wrong_out = weights;
    wrong_out[2] = FrLocal(35);                          // the output wire x: only W of the last gate reads it
    ASSERT(!groth16::is_satisfied(ctx, qap, wrong_out));
    ASSERT(groth16::which_is_unsatisfied(ctx, qap, wrong_out) == std::optional<size_t>(circuit.gates() - 1));
    zk_qap_check_result r = groth16::check(ctx, qap, wrong_out);
    ASSERT(r.bad_gates == 1 && r.first_bad == 1 && r.flags == 0);

    auto wrong_temp = weights;
    wrong_temp[3] = FrLocal(7);                          // temp: W of gate 0 and V of gate 1
    r = groth16::check(ctx, qap, wrong_temp);
    ASSERT(r.bad_gates == 2 && r.first_bad == 0 && r.flags == 0);

    auto wrong_one = weights;
    wrong_one[0] = FrLocal(2);                           // the constant wire
    ASSERT(!groth16::is_satisfied(ctx, qap, wrong_one));
    ASSERT(groth16::check(ctx, qap, wrong_one).flags == ZK_QAP_CHECK_WIRE0);

    // the dense form holds no rows: the check says so instead of guessing
    QAP dense = QAP::from(ctx, circuit);
    try {
        groth16::is_satisfied(ctx, dense, weights);
        ASSERT(!"the dense form must be refused");
    } catch (const Error& e) {
        ASSERT(e.status == ZK_ERR_UNSUPPORTED);
    }
    std::puts("ok");
    return 0;
}
