// groth16::setup_from_powers (include/zksnark.hpp) and zk_crs_from_powers (include/zkgpu.h): the spelling a C++ and a C caller use.
// Run by tests/test_cpp_crs_from_powers.py; argv[1] = the directory of the .zk programs.
//   from_powers_equals_setup     the CRS derived from a transcript of a known (alpha, beta, x) is, array by array, the CRS
//                                setup_with(alpha, beta, 1, 1, x) makes; check_setup accepts it and both CRSs give the same proof bytes
//   from_powers_refusals         the C entry point and the wrapper refuse with the ABI's statuses and leave *out NULL
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "zksnark.hpp"

using namespace zksnark;
using groth16::PowersOfTau;
using groth16::setup_from_powers;
using groth16::setup_with;

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

struct Arrays {
    std::vector<uint64_t> alpha_g1, beta_g1, delta_g1, xi_g1, sum_gamma_g1, sum_delta_g1, xi_t_g1, beta_g2, gamma_g2, delta_g2, xi_g2;
    bool operator==(const Arrays& o) const {
        return alpha_g1 == o.alpha_g1 && beta_g1 == o.beta_g1 && delta_g1 == o.delta_g1 && xi_g1 == o.xi_g1 && sum_gamma_g1 == o.sum_gamma_g1 &&
               sum_delta_g1 == o.sum_delta_g1 && xi_t_g1 == o.xi_t_g1 && beta_g2 == o.beta_g2 && gamma_g2 == o.gamma_g2 && delta_g2 == o.delta_g2 &&
               xi_g2 == o.xi_g2;
    }
};
static Arrays download(const Context& ctx, const groth16::Sigma& s) {
    size_t n, m, l;
    ASSERT(zk_crs_dims(s.get(), &n, &m, &l) == ZK_OK);
    Arrays a;
    a.alpha_g1.resize(8); a.beta_g1.resize(8); a.delta_g1.resize(8); a.xi_g1.resize(8 * n); a.sum_gamma_g1.resize(8 * (l + 1));
    a.sum_delta_g1.resize(8 * (m - l - 1)); a.xi_t_g1.resize(8 * (n - 1)); a.beta_g2.resize(16); a.gamma_g2.resize(16); a.delta_g2.resize(16);
    a.xi_g2.resize(16 * n);
    zk_crs_out o{a.alpha_g1.data(), a.beta_g1.data(), a.delta_g1.data(), a.xi_g1.data(), a.sum_gamma_g1.data(), a.sum_delta_g1.data(),
                 a.xi_t_g1.data(), a.beta_g2.data(), a.gamma_g2.data(), a.delta_g2.data(), a.xi_g2.data()};
    ctx.check(zk_crs_download(ctx.get(), s.get(), &o), "download");
    return a;
}

// the transcript of (alpha, beta, x) for n gates: the generators (xi_g1[0], xi_g2[0] of any CRS) times x^k, alpha x^k, beta x^k
static PowersOfTau transcript(const Context& ctx, const Arrays& any, const FrLocal& alpha, const FrLocal& beta, const FrLocal& x, size_t n) {
    Field f(ctx);
    std::vector<FrLocal> xs(2 * n - 1);
    xs[0] = FrLocal(1);
    for (size_t k = 1; k < xs.size(); ++k) xs[k] = f.mul(xs[k - 1], x);
    auto words = [](const std::vector<FrLocal>& v) {
        std::vector<uint64_t> w;
        for (const auto& e : v) w.insert(w.end(), e.w.begin(), e.w.end());
        return w;
    };
    auto times = [&](const FrLocal& k, size_t count) {
        std::vector<FrLocal> out(count);
        for (size_t i = 0; i < count; ++i) out[i] = f.mul(xs[i], k);
        return out;
    };
    auto repeat = [](const uint64_t* p, size_t words_per_point, size_t count) {
        std::vector<uint64_t> out;
        for (size_t i = 0; i < count; ++i) out.insert(out.end(), p, p + words_per_point);
        return out;
    };
    PowersOfTau p;
    const std::vector<uint64_t> g1 = repeat(any.xi_g1.data(), 8, 2 * n - 1), g2 = repeat(any.xi_g2.data(), 16, n);
    const std::vector<uint64_t> sx = words(xs), sa = words(times(alpha, n)), sb = words(times(beta, n));
    p.tau_g1.resize(8 * (2 * n - 1)); p.tau_g2.resize(16 * n); p.alpha_tau_g1.resize(8 * n); p.beta_tau_g1.resize(8 * n);
    ctx.check(zk_g1_mul_batch(ctx.get(), g1.data(), sx.data(), p.tau_g1.data(), 2 * n - 1), "tau_g1");
    ctx.check(zk_g2_mul_batch(ctx.get(), g2.data(), sx.data(), p.tau_g2.data(), n), "tau_g2");
    ctx.check(zk_g1_mul_batch(ctx.get(), g1.data(), sa.data(), p.alpha_tau_g1.data(), n), "alpha_tau_g1");
    ctx.check(zk_g1_mul_batch(ctx.get(), g1.data(), sb.data(), p.beta_tau_g1.data(), n), "beta_tau_g1");
    ctx.check(zk_g2_mul_batch(ctx.get(), g2.data(), beta.w.data(), p.beta_g2.data(), 1), "beta_g2");
    return p;
}

static void from_powers_equals_setup(const Context& ctx) {
    const std::string code = read_to_string("simple.zk");
    Circuit circuit = ASTParser::try_parse(code);
    QAP qap = QAP::from_sparse(ctx, circuit);
    const size_t n = qap.degree();
    const FrLocal alpha = FrLocal::random_elem(), beta = FrLocal::random_elem(), x = FrLocal::random_elem();
    auto want = setup_with(ctx, qap, {alpha, beta, FrLocal(1), FrLocal(1), x});
    const Arrays w = download(ctx, want);
    const PowersOfTau p = transcript(ctx, w, alpha, beta, x, n);
    auto got = setup_from_powers(ctx, qap, p);
    ASSERT(download(ctx, got) == w);
    auto res = groth16::check_setup(ctx, qap, got);
    ASSERT(res.ok() && (res.flags & ZK_CRS_CHECK_LAGRANGE_PRESENT));
    std::vector<FrLocal> in(circuit.assignments());
    for (auto& e : in) e = FrLocal::random_elem();
    const auto wts = circuit.weights(in);
    const FrLocal r = FrLocal::random_elem(), s = FrLocal::random_elem();
    ASSERT(groth16::prove_with(ctx, qap, got, wts, r, s) == groth16::prove_with(ctx, qap, want, wts, r, s));
    std::puts("ok from_powers_equals_setup");
}

static void from_powers_refusals(const Context& ctx) {
    const std::string code = read_to_string("simple.zk");
    Circuit circuit = ASTParser::try_parse(code);
    QAP qap = QAP::from_sparse(ctx, circuit), dense = QAP::from(ctx, circuit);
    const size_t n = qap.degree();
    const FrLocal alpha(3), beta(5), x(1000003);
    auto any = setup_with(ctx, qap, {alpha, beta, FrLocal(1), FrLocal(1), x});
    const Arrays w = download(ctx, any);
    const PowersOfTau p = transcript(ctx, w, alpha, beta, x, n);
    auto status_of = [&](auto&& call) {
        try { call(); } catch (const Error& e) { return e.status; }
        return (int)ZK_OK;
    };
    // the wrapper
    ASSERT(status_of([&] { setup_from_powers(ctx, dense, p); }) == ZK_ERR_UNSUPPORTED);
    PowersOfTau shorter = p;
    shorter.tau_g1.resize(p.tau_g1.size() - 8);
    ASSERT(status_of([&] { setup_from_powers(ctx, qap, shorter); }) == ZK_ERR_ARG);
    PowersOfTau uneven = p;
    uneven.alpha_tau_g1.resize(p.alpha_tau_g1.size() - 8);
    ASSERT(status_of([&] { setup_from_powers(ctx, qap, uneven); }) == ZK_ERR_ARG);
    PowersOfTau off = p;
    off.beta_tau_g1[0] ^= 1;                                    // x + 1 or x - 1 with the same y: off the curve
    ASSERT(status_of([&] { setup_from_powers(ctx, qap, off); }) == ZK_ERR_RANGE);
    // the C entry point
    zk_powers_desc d{2 * n - 1, n, p.tau_g1.data(), p.tau_g2.data(), p.alpha_tau_g1.data(), p.beta_tau_g1.data(), p.beta_g2.data()};
    zk_crs* out = reinterpret_cast<zk_crs*>(&d);
    ASSERT(zk_crs_from_powers(ctx.get(), qap.get(), nullptr, &out) == ZK_ERR_ARG && out == nullptr);
    ASSERT(zk_crs_from_powers(ctx.get(), qap.get(), &d, nullptr) == ZK_ERR_ARG);
    out = reinterpret_cast<zk_crs*>(&d);
    ASSERT(zk_crs_from_powers(nullptr, qap.get(), &d, &out) == ZK_ERR_ARG && out == nullptr);
    zk_powers_desc few = d;
    few.n_rest = n - 1;
    out = reinterpret_cast<zk_crs*>(&d);
    ASSERT(zk_crs_from_powers(ctx.get(), qap.get(), &few, &out) == ZK_ERR_ARG && out == nullptr);
    ASSERT(std::strstr(zk_last_error(ctx.get()), "zk_crs_from_powers") != nullptr);
    zk_powers_desc hole = d;
    hole.tau_g2 = nullptr;
    out = reinterpret_cast<zk_crs*>(&d);
    ASSERT(zk_crs_from_powers(ctx.get(), qap.get(), &hole, &out) == ZK_ERR_ARG && out == nullptr);
    // and the context still derives
    ASSERT(zk_crs_from_powers(ctx.get(), qap.get(), &d, &out) == ZK_OK && out != nullptr);
    zk_crs_free(out);
    ASSERT(download(ctx, setup_from_powers(ctx, qap, p)) == w);
    std::puts("ok from_powers_refusals");
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <dir of .zk programs>\n", argv[0]); return 2; }
    programs_dir = argv[1];
    try {
        Context ctx(0);
        from_powers_equals_setup(ctx);
        from_powers_refusals(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
