// groth16::check_setup / check_setup_with (include/zksnark.hpp, over zk_crs_check): the spelling a C++ caller uses.  Run by
// tests/test_cpp_crs_check.py; argv[1] = the directory of the .zk programs, ZK_TEST_TMP = a directory for the CRS file.
//   check_setup_dense_and_parsed     the CRS setup made passes, for the struct-literal QAP (a non-monic t) and for a parsed program in
//                                    its dense and its sparse (integer-roots) form; the latter reports its Lagrange-basis arrays
//   check_setup_other_circuit        the CRS of a circuit with the same dimensions that differs in one entry of w fails WIRES
//   check_setup_file                 a CRS saved and loaded again passes
//   check_setup_errors               a CRS of other dimensions, a zero challenge and one >= r throw with the ABI's status
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using groth16::check_setup;
using groth16::check_setup_with;
using groth16::setup;

static std::string programs_dir;
static std::string read_to_string(const std::string& name) {
    std::ifstream f(programs_dir + "/" + name);
    if (!f) { std::fprintf(stderr, "cannot read %s/%s\n", programs_dir.c_str(), name.c_str()); std::exit(2); }
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}
#define ASSERT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "assertion failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static QAP one_gate(const Context& ctx, uint64_t w_out) {
    auto constant = [](uint64_t v) { return std::vector<FrLocal>{FrLocal(v)}; };
    return QAP::from_dense(ctx, {constant(0), constant(0), constant(1), constant(0)}, {constant(0), constant(0), constant(0), constant(1)},
                           {constant(0), constant(w_out), constant(0), constant(0)}, {FrLocal(500), FrLocal(2)}, 2);   // t = 2 x + 500
}

static void check_setup_dense_and_parsed(const Context& ctx) {
    QAP qap = one_gate(ctx, 1);
    auto sigma = setup(ctx, qap);
    auto res = check_setup(ctx, qap, sigma);
    ASSERT(res.ok() && res.failed == 0 && res.flags == 0);
    ASSERT(check_setup_with(ctx, qap, sigma, FrLocal(12345)).ok());
    std::string code = read_to_string("simple.zk");
    QAP dense = QAP::from(ctx, ASTParser::try_parse(code));
    auto s_dense = setup(ctx, dense);
    ASSERT(check_setup(ctx, dense, s_dense).ok());
    QAP sparse = QAP::from_sparse(ctx, ASTParser::try_parse(code));
    auto s_sparse = setup(ctx, sparse);
    res = check_setup(ctx, sparse, s_sparse);
    ASSERT(res.ok() && (res.flags & ZK_CRS_CHECK_LAGRANGE_PRESENT));
    // the two forms are one QAP: either CRS passes against either handle
    ASSERT(check_setup(ctx, sparse, s_dense).ok() && check_setup(ctx, dense, s_sparse).ok());
    std::puts("ok check_setup_dense_and_parsed");
}

static void check_setup_other_circuit(const Context& ctx) {
    QAP qap = one_gate(ctx, 1), other = one_gate(ctx, 2);
    auto sigma = setup(ctx, other);
    auto res = check_setup(ctx, qap, sigma);
    ASSERT(!res.ok() && res.has(ZK_CRS_CHECK_WIRES) && res.has(ZK_CRS_CHECK_WIRES_GAMMA) && !res.has(ZK_CRS_CHECK_WIRES_DELTA));
    ASSERT(!res.has(ZK_CRS_CHECK_XI_T) && !res.has(ZK_CRS_CHECK_TWINS) && !res.has(ZK_CRS_CHECK_GENERATORS));
    ASSERT(check_setup(ctx, other, sigma).ok());
    std::puts("ok check_setup_other_circuit");
}

static void check_setup_file(const Context& ctx) {
    const char* tmp = std::getenv("ZK_TEST_TMP");
    ASSERT(tmp);
    const std::string path = std::string(tmp) + "/check_setup.crs";
    QAP qap = one_gate(ctx, 1);
    setup(ctx, qap).save(ctx, path);
    auto loaded = groth16::Sigma::load(ctx, path);
    ASSERT(check_setup(ctx, qap, loaded).ok());
    std::puts("ok check_setup_file");
}

static void check_setup_errors(const Context& ctx) {
    QAP qap = one_gate(ctx, 1);
    QAP parsed = QAP::from(ctx, ASTParser::try_parse(read_to_string("simple.zk")));
    auto sigma = setup(ctx, qap);
    auto status_of = [&](auto&& call) {
        try { call(); } catch (const Error& e) { return e.status; }
        return (int)ZK_OK;
    };
    ASSERT(status_of([&] { check_setup(ctx, parsed, sigma); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { check_setup_with(ctx, qap, sigma, FrLocal(0)); }) == ZK_ERR_ARG);
    FrLocal big;
    big.w = FrLocal::MODULUS;
    ASSERT(status_of([&] { check_setup_with(ctx, qap, sigma, big); }) == ZK_ERR_RANGE);
    ASSERT(check_setup(ctx, qap, sigma).ok());
    std::puts("ok check_setup_errors");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <dir of .zk programs>\n", argv[0]); return 2; }
    programs_dir = argv[1];
    try {
        Context ctx(0);
        check_setup_dense_and_parsed(ctx);
        check_setup_other_circuit(ctx);
        check_setup_file(ctx);
        check_setup_errors(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
