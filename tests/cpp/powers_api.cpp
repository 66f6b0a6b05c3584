// groth16::ResidentPowers, check_powers, contribute_powers, check_powers_contribution (include/zksnark.hpp, over zk_powers_*): the
// spelling a C++ caller uses, and the C ABI's argument refusals.  Run by tests/test_cpp_powers.py; argv[1] = the directory of the .zk
// programs.
//   powers_ceremony   initial -> two contributions, each checked and bound to its tag -> download -> setup_from_powers on a parsed
//                     program (sparse form) -> check_setup -> a proof that verifies
//   powers_records    a record checked against the wrong pair fails RECORD, under another tag KNOWLEDGE; fixed secrets twice are the
//                     product once; an uploaded download is the same transcript
//   powers_errors     secrets 0 and >= r, a zero challenge and one >= r, other dims, bad shapes throw with the ABI's status; the C
//                     calls refuse null pointers, leave *out NULL and results untouched
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "zksnark.hpp"

using namespace zksnark;
using groth16::check_powers;
using groth16::check_powers_contribution;
using groth16::check_powers_contribution_with;
using groth16::check_powers_with;
using groth16::contribute_powers;
using groth16::contribute_powers_with;
using groth16::ResidentPowers;

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
    for (size_t i = 0; i < t.size(); ++i) t[i] = (uint8_t)(seed + 5 * i);
    return t;
}

static void powers_ceremony(const Context& ctx) {
    QAP qap = QAP::from_sparse(ctx, ASTParser::try_parse(read_to_string("simple.zk")));
    size_t n = 0, m = 0, input = 0;
    int kind = 0;
    ctx.check(zk_qap_dims(qap.get(), &n, &m, &input, &kind), "zk_qap_dims");
    auto head = ResidentPowers::initial(ctx, 2 * n - 1 < 2 ? 2 : 2 * n - 1, n < 2 ? 2 : n);
    ASSERT(check_powers(ctx, head).ok());
    const auto tag1 = tag_of(1), tag2 = tag_of(2);
    auto c1 = contribute_powers(ctx, head, tag1);
    auto c2 = contribute_powers(ctx, c1.first, tag2);
    ASSERT(check_powers_contribution(ctx, head, c1.first, c1.second, tag1).ok());
    ASSERT(check_powers_contribution(ctx, c1.first, c2.first, c2.second, tag2).ok());
    ASSERT(c2.second.verify(tag2) && !c2.second.verify(tag1));
    ASSERT(check_powers(ctx, c2.first).ok());
    auto sigma = groth16::setup_from_powers(ctx, qap, c2.first.download(ctx));
    ASSERT(groth16::check_setup(ctx, qap, sigma).ok());
    std::puts("ok powers_ceremony");
}

static void powers_records(const Context& ctx) {
    auto head = ResidentPowers::initial(ctx, 9, 4);
    ASSERT(head.dims().first == 9 && head.dims().second == 4);
    const auto tag = tag_of(3), other_tag = tag_of(4);
    auto a = contribute_powers_with(ctx, head, {FrLocal(3), FrLocal(5), FrLocal(7)}, tag);
    auto b = contribute_powers_with(ctx, a.first, {FrLocal(11), FrLocal(13), FrLocal(17)}, tag);
    auto once = contribute_powers_with(ctx, head, {FrLocal(33), FrLocal(65), FrLocal(119)}, tag);
    const auto pb = b.first.download(ctx), po = once.first.download(ctx);
    ASSERT(pb.tau_g1 == po.tau_g1 && pb.tau_g2 == po.tau_g2 && pb.alpha_tau_g1 == po.alpha_tau_g1 && pb.beta_tau_g1 == po.beta_tau_g1 && pb.beta_g2 == po.beta_g2);
    ASSERT(check_powers_contribution_with(ctx, head, a.first, a.second, tag, FrLocal(12345)).failed == 0);
    ASSERT(check_powers_contribution(ctx, head, b.first, b.second, tag).failed == ZK_POWERS_CHECK_RECORD);
    ASSERT(check_powers_contribution(ctx, head, a.first, a.second, other_tag).failed == ZK_POWERS_CHECK_KNOWLEDGE);
    auto again = ResidentPowers::upload(ctx, pb);
    ASSERT(check_powers_with(ctx, again, FrLocal(777)).ok());
    const auto pa = again.download(ctx);
    ASSERT(pa.tau_g1 == pb.tau_g1 && pa.beta_g2 == pb.beta_g2);
    // an entry of alpha_tau_g1 replaced by another point of the curve: the check names the array
    auto bad = pb;
    for (size_t w = 0; w < ZK_G1_WORDS; ++w) bad.alpha_tau_g1[2 * ZK_G1_WORDS + w] = pb.tau_g1[3 * ZK_G1_WORDS + w];
    ASSERT(check_powers_with(ctx, ResidentPowers::upload(ctx, bad), FrLocal(777)).failed == ZK_POWERS_CHECK_ALPHA);
    std::puts("ok powers_records");
}

static void powers_errors(const Context& ctx) {
    auto head = ResidentPowers::initial(ctx, 5, 3);
    auto other = ResidentPowers::initial(ctx, 6, 3);
    const auto tag = tag_of(5);
    auto status_of = [&](auto&& call) {
        try { call(); } catch (const Error& e) { return e.status; }
        return (int)ZK_OK;
    };
    FrLocal big;
    big.w = FrLocal::MODULUS;
    ASSERT(status_of([&] { ResidentPowers::initial(ctx, 1, 1); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { ResidentPowers::initial(ctx, 2, 3); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { contribute_powers_with(ctx, head, {FrLocal(0), FrLocal(1), FrLocal(1)}, tag); }) == ZK_ERR_DIV_BY_ZERO);
    ASSERT(status_of([&] { contribute_powers_with(ctx, head, {FrLocal(1), FrLocal(1), big}, tag); }) == ZK_ERR_RANGE);
    ASSERT(status_of([&] { check_powers_with(ctx, head, FrLocal(0)); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { check_powers_with(ctx, head, big); }) == ZK_ERR_RANGE);
    auto next = contribute_powers(ctx, head, tag);
    ASSERT(status_of([&] { check_powers_contribution(ctx, other, next.first, next.second, tag); }) == ZK_ERR_ARG);
    ASSERT(status_of([&] { check_powers_contribution_with(ctx, head, next.first, next.second, tag, FrLocal(0)); }) == ZK_ERR_ARG);
    // the C ABI itself
    zk_powers* out = reinterpret_cast<zk_powers*>(0x10);
    zk_powers_contribution rec;
    std::memset(&rec, 0x5a, sizeof(rec));
    const zk_powers_contribution untouched = rec;
    ASSERT(zk_powers_contribute(ctx.get(), nullptr, nullptr, nullptr, &out, &rec) == ZK_ERR_ARG && out == nullptr);
    out = reinterpret_cast<zk_powers*>(0x10);
    ASSERT(zk_powers_contribute(ctx.get(), head.get(), nullptr, nullptr, &out, nullptr) == ZK_ERR_ARG && out == nullptr);
    ASSERT(zk_powers_contribute(ctx.get(), head.get(), nullptr, nullptr, nullptr, &rec) == ZK_ERR_ARG);
    ASSERT(std::memcmp(&rec, &untouched, sizeof(rec)) == 0);
    out = reinterpret_cast<zk_powers*>(0x10);
    ASSERT(zk_powers_upload(ctx.get(), nullptr, &out) == ZK_ERR_ARG && out == nullptr);
    out = reinterpret_cast<zk_powers*>(0x10);
    ASSERT(zk_powers_initial(nullptr, 5, 3, &out) == ZK_ERR_ARG && out == nullptr);
    zk_powers_check_result res{0xAAAAAAAAu, 0xBBBBBBBBu};
    ASSERT(zk_powers_check(ctx.get(), nullptr, nullptr, &res) == ZK_ERR_ARG);
    ASSERT(zk_powers_check(ctx.get(), head.get(), nullptr, nullptr) == ZK_ERR_ARG);
    ASSERT(zk_powers_contribution_check(ctx.get(), head.get(), next.first.get(), nullptr, nullptr, nullptr, &res) == ZK_ERR_ARG);
    ASSERT(res.failed == 0xAAAAAAAAu && res.flags == 0xBBBBBBBBu);
    ASSERT(zk_powers_dims(nullptr, nullptr, nullptr) == ZK_ERR_ARG);
    ASSERT(zk_powers_download(ctx.get(), head.get(), nullptr) == ZK_ERR_ARG);
    ASSERT(zk_powers_contribution_verify(nullptr, nullptr, nullptr) == ZK_ERR_ARG);
    ASSERT(zk_g1_mul_each(nullptr, nullptr, nullptr, nullptr, 0) == ZK_ERR_ARG);
    zk_powers_free(nullptr);
    ASSERT(check_powers(ctx, head).ok());
    std::puts("ok powers_errors");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <dir of .zk programs>\n", argv[0]); return 2; }
    programs_dir = argv[1];
    try {
        Context ctx(0);
        powers_ceremony(ctx);
        powers_records(ctx);
        powers_errors(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
