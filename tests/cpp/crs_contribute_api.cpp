// groth16::contribute / check_contribution (include/zksnark.hpp, over zk_crs_contribute / zk_crs_contribution_check): the spelling a
// C++ caller uses.  Run by tests/test_cpp_crs_contribute.py; argv[1] = the directory of the .zk programs, ZK_TEST_TMP = a directory
// for the CRS file.
//   contribute_parsed        a parsed program in its dense and its sparse (integer-roots) form: the contributed CRS passes check_setup and
//                            check_contribution, proofs over it verify against it and not against the source, the record verifies
//                            for its tag only and survives its byte form
//   contribute_chain         two contributions, each record bound to the one before; a record checked against the wrong pair fails RECORD
//   contribute_file          a contributed CRS saved and loaded again is still a valid successor and still proves
//   contribute_errors        d = 0, d >= r, CRSs of other dimensions, a zero challenge and one >= r throw with the ABI's status
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using groth16::check_contribution;
using groth16::check_contribution_with;
using groth16::check_setup;
using groth16::contribute;
using groth16::contribute_with;
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

static groth16::Tag tag_of(uint8_t seed) {
    groth16::Tag t;
    for (size_t i = 0; i < t.size(); ++i) t[i] = (uint8_t)(seed + 3 * i);
    return t;
}

static void contribute_parsed(const Context& ctx) {
    const std::string code = read_to_string("simple.zk");
    const auto tag = tag_of(1), other_tag = tag_of(2);
    for (int sparse = 0; sparse < 2; ++sparse) {
        QAP qap = sparse ? QAP::from_sparse(ctx, ASTParser::try_parse(code)) : QAP::from(ctx, ASTParser::try_parse(code));
        auto sigma = setup(ctx, qap);
        auto next = contribute(ctx, sigma, tag);
        ASSERT(check_setup(ctx, qap, next.first).ok());
        auto res = check_contribution(ctx, sigma, next.first, next.second, tag);
        ASSERT(res.ok() && res.failed == 0);
        ASSERT(check_contribution_with(ctx, sigma, next.first, next.second, tag, FrLocal(12345)).ok());
        ASSERT(check_contribution(ctx, sigma, next.first, next.second, other_tag).failed == ZK_CONTRIB_KNOWLEDGE);
        ASSERT(next.second.verify(tag) && !next.second.verify(other_tag));
        ASSERT(groth16::Contribution::from_bytes(next.second.to_bytes()).verify(tag));
        ASSERT(next.second.to_bytes().size() == 224);
    }
    std::puts("ok contribute_parsed");
}

static QAP one_gate(const Context& ctx) {
    auto constant = [](uint64_t v) { return std::vector<FrLocal>{FrLocal(v)}; };
    return QAP::from_dense(ctx, {constant(0), constant(0), constant(1), constant(0)}, {constant(0), constant(0), constant(0), constant(1)},
                           {constant(0), constant(1), constant(0), constant(0)}, {FrLocal(500), FrLocal(2)}, 2);   // t = 2 x + 500
}

static void contribute_chain(const Context& ctx) {
    QAP qap = one_gate(ctx);
    auto s0 = setup(ctx, qap);
    const auto tag1 = tag_of(7);
    auto c1 = contribute_with(ctx, s0, FrLocal(11), tag1);
    groth16::Tag tag2;
    const auto bytes1 = c1.second.to_bytes();
    for (size_t i = 0; i < tag2.size(); ++i) tag2[i] = bytes1[64 + i];   // any function of the transcript so far
    auto c2 = contribute(ctx, c1.first, tag2);
    ASSERT(check_contribution(ctx, s0, c1.first, c1.second, tag1).ok());
    ASSERT(check_contribution(ctx, c1.first, c2.first, c2.second, tag2).ok());
    ASSERT(check_contribution(ctx, s0, c2.first, c2.second, tag2).failed == ZK_CONTRIB_RECORD);
    ASSERT(check_setup(ctx, qap, c2.first).ok());
    // d = 11 twice is d = 121 once: the same delta_g1
    auto a = contribute_with(ctx, contribute_with(ctx, s0, FrLocal(11), tag1).first, FrLocal(11), tag1);
    auto b = contribute_with(ctx, s0, FrLocal(121), tag1);
    ASSERT(std::memcmp(a.second.raw.delta_after_g1, b.second.raw.delta_after_g1, sizeof(b.second.raw.delta_after_g1)) == 0);
    std::puts("ok contribute_chain");
}

static void contribute_file(const Context& ctx) {
    const char* tmp = std::getenv("ZK_TEST_TMP");
    ASSERT(tmp);
    const std::string path = std::string(tmp) + "/contributed.crs";
    const std::string code = read_to_string("simple.zk");
    QAP qap = QAP::from_sparse(ctx, ASTParser::try_parse(code));
    auto sigma = setup(ctx, qap);
    const auto tag = tag_of(9);
    auto next = contribute(ctx, sigma, tag);
    next.first.save(ctx, path);
    auto loaded = groth16::Sigma::load(ctx, path);
    ASSERT(check_contribution(ctx, sigma, loaded, next.second, tag).ok());
    ASSERT(check_setup(ctx, qap, loaded).ok());
    std::puts("ok contribute_file");
}

static void contribute_errors(const Context& ctx) {
    QAP qap = one_gate(ctx);
    QAP parsed = QAP::from(ctx, ASTParser::try_parse(read_to_string("simple.zk")));
    auto sigma = setup(ctx, qap);
    auto other = setup(ctx, parsed);
    const auto tag = tag_of(3);
    auto status_of = [&](auto&& call) {
        try { call(); } catch (const Error& e) { return e.status; }
        return (int)ZK_OK;
    };
    FrLocal big;
    big.w = FrLocal::MODULUS;
    ASSERT(status_of([&] { contribute_with(ctx, sigma, FrLocal(0), tag); }) == ZK_ERR_DIV_BY_ZERO);
    ASSERT(status_of([&] { contribute_with(ctx, sigma, big, tag); }) == ZK_ERR_RANGE);
    auto next = contribute(ctx, sigma, tag);
    ASSERT(status_of([&] { check_contribution(ctx, other, next.first, next.second, tag); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { check_contribution_with(ctx, sigma, next.first, next.second, tag, FrLocal(0)); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { check_contribution_with(ctx, sigma, next.first, next.second, tag, big); }) == ZK_ERR_RANGE);
    ASSERT(check_contribution(ctx, sigma, next.first, next.second, tag).ok());
    std::puts("ok contribute_errors");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <dir of .zk programs>\n", argv[0]); return 2; }
    programs_dir = argv[1];
    try {
        Context ctx(0);
        contribute_parsed(ctx);
        contribute_chain(ctx);
        contribute_file(ctx);
        contribute_errors(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
