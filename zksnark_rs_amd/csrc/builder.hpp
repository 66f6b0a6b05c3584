// builder.hpp -- the reference's gate-level circuit builder (host code, as in the reference) and what a finished circuit needs to be an
// ordinary zk_circuit: rows, the two host evaluators' program, the field tape of witgen.hip, the boolean tape of boolgen.hip, and the
// split into a boolean core and a field tail that mixgen.hip runs (built_split), with its host runner (mixed_run_host).
//
//   Circuit::new, zero / unity wire, new_wire        circuit/builder/mod.rs:91-125
//   new_sub_circuit                                  mod.rs:491-557 (weights and wires of (sum left) * (sum right) = out)
//   new_bit_checker .. new_xnor, fan_in, bitwise_op  mod.rs:723-827
//   new_less_than, new_greater_than, new_equality    mod.rs:939-957
//   is_equal .. greater_than                         mod.rs:995-1241
//   keccakf_1600, absorb, xorin, pad, squeeze        mod.rs:1247-1398, tables types.rs:295-328
//
// Every constructor emits exactly the reference's sub-circuits in the reference's order, so gate counts and weights are its own.
// What differs, on purpose: wires are numbered and ordered deterministically (the reference iterates a HashMap); entries on the
// constant-zero wire are dropped instead of becoming a witness wire that no constraint pins; its builder -> DummyRep conversion
// (num_wires empty rows in front) is not reproduced; zk_builder_assert_bit and zk_builder_pack exist, and so do the Poseidon
// gadgets (zk_builder_poseidon, zk_builder_merkle_root: general sub-circuits over linear forms, see BuilderOps::Form) and the Baby Jubjub
// gadgets over the same forms (zk_builder_babyjub_*), and zk_builder_eddsa_verify composes them.  Header-only and free of device code, so tests/cpp/builder_host.hip compiles it alone under the sanitizers.
#pragma once
#include <array>
#include <map>
#include "circuit.hpp"
#include "babyjub.hpp"
#include "poseidon.hpp"
#include "eddsa.hpp"

struct zk_builder {
    struct Term { zk::Fr w; uint32_t wire; };
    struct Sub { uint32_t l0, r0, end, out, bkind, a, b; };
    // per wire id: 0 = a constant (ids 0 and 1), 1 = bit input, 2 = field input, 3 = a sub-circuit's output, 4 = a packed wire (zk_builder_pack)
    std::vector<uint8_t> kind{0, 0};
    std::vector<Term> terms;
    std::vector<Sub> subs;
    bool boolean = true, finished = false;
    std::string last_error;
};

namespace zk {

static const uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
static const unsigned KECCAK_RHO[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
static const unsigned KECCAK_PI[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};

struct BuilderOps {
    zk_builder& b;
    typedef std::pair<int, uint32_t> T;   // (+1 | -1, wire)

    [[noreturn]] static void fail(const std::string& m) { throw ParseError{ZK_ERR_ARG, "builder: " + m}; }
    void live() const { if (b.finished) fail("the circuit is finished; only zk_builder_free may follow zk_builder_finish"); }
    void known(uint32_t w) const { if (w >= b.kind.size()) fail("unknown wire id " + std::to_string(w)); }
    uint32_t new_wire(uint8_t kind) {
        if (b.kind.size() >= 0x7ffffff0u) fail("too many wires");
        b.kind.push_back(kind);
        return (uint32_t)(b.kind.size() - 1);
    }
    uint32_t close_sub(uint32_t l0, uint32_t r0, bool with_out, uint32_t bkind, uint32_t x, uint32_t y) {
        if (b.subs.size() >= 0x7ffffff0u || b.terms.size() >= 0xfffffff0u) fail("too many sub-circuits");
        for (size_t e = l0; e < b.terms.size(); ++e)      // a packed wire is a field element: whatever reads one is no boolean operation
            if (b.kind[b.terms[e].wire] == 4) b.boolean = false;
        const uint32_t out = with_out ? new_wire(3) : WIT_NONE;
        b.subs.push_back({l0, r0, (uint32_t)b.terms.size(), out, bkind, x, y});
        return out;
    }
    uint32_t sub(std::initializer_list<T> l, std::initializer_list<T> r, uint32_t bkind, uint32_t x, uint32_t y, bool with_out = true) {
        const Fr one = Fr::one(), minus = -Fr::one();
        const uint32_t l0 = (uint32_t)b.terms.size();
        for (const T& t : l) b.terms.push_back({t.first > 0 ? one : minus, t.second});
        const uint32_t r0 = (uint32_t)b.terms.size();
        for (const T& t : r) b.terms.push_back({t.first > 0 ? one : minus, t.second});
        return close_sub(l0, r0, with_out, bkind, x, y);
    }
    // new_sub_circuit with the caller's weights (canonical words): the circuit is no longer boolean
    uint32_t general(const uint64_t* lw, const uint32_t* lwire, size_t nl, const uint64_t* rw, const uint32_t* rwire, size_t nr) {
        for (size_t i = 0; i < nl; ++i) known(lwire[i]);
        for (size_t i = 0; i < nr; ++i) known(rwire[i]);
        for (size_t i = 0; i < nl + nr; ++i) {
            const Fr x = fr_from_words((i < nl ? lw + 4 * i : rw + 4 * (i - nl)));
            if (!x.raw_in_range()) throw ParseError{ZK_ERR_RANGE, "builder: weight >= r"};
        }
        const uint32_t l0 = (uint32_t)b.terms.size();
        for (size_t i = 0; i < nl; ++i) b.terms.push_back({Fr::from_canonical(fr_from_words(lw + 4 * i)), lwire[i]});
        const uint32_t r0 = (uint32_t)b.terms.size();
        for (size_t i = 0; i < nr; ++i) b.terms.push_back({Fr::from_canonical(fr_from_words(rw + 4 * i)), rwire[i]});
        b.boolean = false;
        return close_sub(l0, r0, true, BOOL_NONE, 0, 0);
    }
    // (sum 2^i bits[i]) * (1) = out: a general sub-circuit whose output boolgen.hip gathers from the operands' bits, so the circuit stays
    // boolean as long as the operands are bit-valued (a field input or a general sub-circuit has cleared the flag already, a packed
    // operand clears it in close_sub)
    uint32_t pack(const uint32_t* bits, size_t n) {
        if (n < 1 || n > ZK_PACK_MAX_BITS) fail("pack: n_bits must be in 1.." + std::to_string(ZK_PACK_MAX_BITS) + ", got " + std::to_string(n));
        for (size_t i = 0; i < n; ++i) known(bits[i]);
        const uint32_t l0 = (uint32_t)b.terms.size();
        for (size_t i = 0; i < n; ++i) {
            uint64_t w[4] = {0, 0, 0, 0};
            w[i / 64] = 1ull << (i % 64);
            b.terms.push_back({Fr::from_canonical(fr_from_words(w)), bits[i]});
        }
        const uint32_t r0 = (uint32_t)b.terms.size();
        b.terms.push_back({Fr::one(), 1});
        const uint32_t out = close_sub(l0, r0, true, BOOL_PACK, 0, 0);
        b.kind[out] = 4;
        return out;
    }

    // ---- Poseidon (poseidon.hpp) as general sub-circuits over linear forms ----
    // A form is a sum of weighted wires: one term per wire, weights mod r in Montgomery form, no zero weight, the constant carried on
    // wire 1; the constant-zero wire is the empty form.  Terms are emitted in the order of their wire ids.
    typedef std::map<uint32_t, Fr> Form;
    static Form form_of(uint32_t wire) {
        Form f;
        if (wire != 0) f[wire] = Fr::one();
        return f;
    }
    static void form_add(Form& a, const Form& x, const Fr& scale) {
        for (const auto& e : x) {
            auto it = a.find(e.first);
            const Fr v = (it == a.end() ? Fr::zero() : it->second) + e.second * scale;
            if (v.is_zero()) { if (it != a.end()) a.erase(it); }
            else if (it == a.end()) a.emplace(e.first, v);
            else it->second = v;
        }
    }
    void push_form(const Form& f) { for (const auto& e : f) b.terms.push_back({e.second, e.first}); }
    uint32_t sub_forms(const Form& l, const Form& r) {
        const uint32_t l0 = (uint32_t)b.terms.size();
        push_form(l);
        const uint32_t r0 = (uint32_t)b.terms.size();
        push_form(r);
        b.boolean = false;
        return close_sub(l0, r0, true, BOOL_NONE, 0, 0);
    }
    // L^5 as L * L = a, a * a = c, c * L = e
    uint32_t sbox(const Form& f) {
        const Form a = form_of(sub_forms(f, f));
        const Form c = form_of(sub_forms(a, a));
        return sub_forms(c, f);
    }
    // The state is t forms.  Round constants and the mix are folded into the forms and cost no gate; an S-box makes its element a
    // wire again, so in the partial rounds elements 1 .. t-1 grow by one term a round, to t + R_P + 1 at most.  One closing
    // sub-circuit (state[0]) * 1 = out makes the digest a wire: 3 (R_F t + R_P) + 1 gates.
    uint32_t poseidon_forms(const Form* in, size_t arity) {
        const PoseidonParams* p = poseidon_params(arity);
        if (!p) fail("poseidon: the arity must be 1, 2 or 4, got " + std::to_string(arity));
        return poseidon_forms_over(in, p);
    }
    // over any parameter set: width 6 (poseidon_params_t6) reaches the builder through eddsa_verify only
    uint32_t poseidon_forms_over(const Form* in, const PoseidonParams* p) {
        const unsigned t = p->t;
        Form state[POSEIDON_MAX_T], next[POSEIDON_MAX_T];
        for (unsigned i = 1; i < t; ++i) state[i] = in[i - 1];
        const Form unity = form_of(1);
        for (unsigned rnd = 0; rnd < p->rounds(); ++rnd) {
            for (unsigned i = 0; i < t; ++i) form_add(state[i], unity, p->c[(size_t)rnd * t + i]);
            const bool full = rnd < p->rf / 2 || rnd >= p->rf / 2 + p->rp;
            for (unsigned i = 0; i < (full ? t : 1u); ++i) state[i] = form_of(sbox(state[i]));
            for (unsigned i = 0; i < t; ++i) {
                next[i].clear();
                for (unsigned j = 0; j < t; ++j) form_add(next[i], state[j], p->m[i * t + j]);
            }
            for (unsigned i = 0; i < t; ++i) state[i].swap(next[i]);
        }
        return sub_forms(state[0], unity);
    }
    uint32_t poseidon(const uint32_t* in, size_t arity) {
        if (!poseidon_rp(arity)) fail("poseidon: the arity must be 1, 2 or 4, got " + std::to_string(arity));
        Form f[POSEIDON_MAX_T - 1];
        for (size_t i = 0; i < arity; ++i) { known(in[i]); f[i] = form_of(in[i]); }
        return poseidon_forms(f, arity);
    }
    // per level: dir is a bit; d = dir * (sib - cur); the next cur = Poseidon(cur + d, sib - d), the pair in the order the bit says
    uint32_t merkle_root(uint32_t leaf, const uint32_t* siblings, const uint32_t* dirs, size_t depth) {
        known(leaf);
        for (size_t k = 0; k < depth; ++k) { known(siblings[k]); known(dirs[k]); }
        const Fr one = Fr::one(), minus = -Fr::one();
        uint32_t cur = leaf;
        for (size_t k = 0; k < depth; ++k) {
            assert_bit(dirs[k]);
            Form diff = form_of(siblings[k]);
            form_add(diff, form_of(cur), minus);
            Form dir;
            dir[dirs[k]] = one;                 // an entry on the constant-zero wire is dropped at finish, like everywhere
            const Form d = form_of(sub_forms(dir, diff));
            Form pair[2] = {form_of(cur), form_of(siblings[k])};
            form_add(pair[0], d, one);
            form_add(pair[1], d, minus);
            cur = poseidon_forms(pair, 2);
        }
        return cur;
    }

    // ---- Baby Jubjub (babyjub.hpp) as general sub-circuits over linear forms ----
    // A point is three wires (X : Y : Z); an affine point is (x, y, wire 1).  Nothing here divides: the gadgets evaluate the projective
    // formulas forward, and zk_builder_babyjub_affine pins affine coordinates the caller supplies.
    static Form form_const(const Fr& c) {
        Form f;
        if (!c.is_zero()) f[1] = c;
        return f;
    }
    static Form form_sum(const Form& a, const Form& x, const Fr& scale) {
        Form f = a;
        form_add(f, x, scale);
        return f;
    }
    // (l) * (r) = 0: a sub-circuit without output, as assert_bit
    void assert_forms(const Form& l, const Form& r) {
        const uint32_t l0 = (uint32_t)b.terms.size();
        push_form(l);
        const uint32_t r0 = (uint32_t)b.terms.size();
        push_form(r);
        b.boolean = false;
        close_sub(l0, r0, false, BOOL_NONE, 0, 0);
    }
    // x x = u, y y = v, u v = w, (a u + v - 1 - d w) * 1 = 0
    void babyjub_assert_on_curve(uint32_t x, uint32_t y) {
        const BjConsts k = babyjub_consts();
        const Fr one = Fr::one();
        const Form u = form_of(sub_forms(form_of(x), form_of(x))), v = form_of(sub_forms(form_of(y), form_of(y)));
        const Form w = form_of(sub_forms(u, v));
        Form eq;
        form_add(eq, u, k.a);
        form_add(eq, v, one);
        form_add(eq, form_const(one), -one);
        form_add(eq, w, -k.d);
        assert_forms(eq, form_of(1));
    }
    // add-2008-bbjlp; z2 == nullptr: the second operand is affine and A = Z1 costs no gate (10 gates instead of 11)
    void babyjub_add_forms(const Form& x1, const Form& y1, const Form& z1, const Form& x2, const Form& y2, const Form* z2, uint32_t out[3]) {
        const BjConsts k = babyjub_consts();
        const Fr one = Fr::one(), minus = -Fr::one();
        const Form A = z2 ? form_of(sub_forms(z1, *z2)) : z1;
        const Form B = form_of(sub_forms(A, A));
        const Form C = form_of(sub_forms(x1, x2)), D = form_of(sub_forms(y1, y2));
        const Form E = form_of(sub_forms(C, D));
        const Form H = form_of(sub_forms(form_sum(x1, y1, one), form_sum(x2, y2, one)));
        const Form F = form_sum(B, E, -k.d), G = form_sum(B, E, k.d);
        const Form AF = form_of(sub_forms(A, F)), AG = form_of(sub_forms(A, G));
        out[0] = sub_forms(AF, form_sum(form_sum(H, C, minus), D, minus));
        out[1] = sub_forms(AG, form_sum(D, C, -k.a));
        out[2] = sub_forms(F, G);
    }
    // dbl-2008-bbjlp: 7 gates
    void babyjub_dbl_forms(const Form& x, const Form& y, const Form& z, uint32_t out[3]) {
        const BjConsts k = babyjub_consts();
        const Fr one = Fr::one(), minus = -Fr::one();
        const Form s = form_sum(x, y, one);
        const Form B = form_of(sub_forms(s, s)), C = form_of(sub_forms(x, x)), D = form_of(sub_forms(y, y)), H = form_of(sub_forms(z, z));
        const Form E = form_sum(Form(), C, k.a);
        const Form F = form_sum(E, D, one), J = form_sum(F, H, -(one + one));
        out[0] = sub_forms(form_sum(form_sum(B, C, minus), D, minus), J);
        out[1] = sub_forms(F, form_sum(E, D, minus));
        out[2] = sub_forms(F, J);
    }
    void babyjub_add(const uint32_t p[3], const uint32_t q[3], uint32_t out[3]) {
        for (int i = 0; i < 3; ++i) { known(p[i]); known(q[i]); }
        const Form z2 = form_of(q[2]);
        uint32_t o[3];                                      // out may alias p or q
        babyjub_add_forms(form_of(p[0]), form_of(p[1]), form_of(p[2]), form_of(q[0]), form_of(q[1]), q[2] == 1 ? nullptr : &z2, o);
        std::copy(o, o + 3, out);
    }
    // x Z = t, (t - X) * 1 = 0, and the same for y
    void babyjub_affine(const uint32_t p[3], const uint32_t xy[2]) {
        for (int i = 0; i < 3; ++i) known(p[i]);
        known(xy[0]); known(xy[1]);
        for (int i = 0; i < 2; ++i) {
            const Form t = form_of(sub_forms(form_of(xy[i]), form_of(p[2])));
            assert_forms(form_sum(t, form_of(p[i]), -Fr::one()), form_of(1));
        }
    }
    // The point table[sum 2^i bits[i]] of a table of 2^n affine points, n <= 3, as two forms: multilinear in the bits, the coefficient of
    // a product of bits is the alternating sum of the entries below it; the products b0 b1, b0 b2, b1 b2, (b0 b1) b2 are the gates.
    void babyjub_select(const uint32_t* bits, size_t n, const BjAffine* table, Form& x, Form& y) {
        Form prod[8];
        prod[0] = form_of(1);
        for (size_t i = 0; i < n; ++i) prod[(size_t)1 << i] = form_of(bits[i]);
        if (n >= 2) prod[3] = form_of(sub_forms(form_of(bits[0]), form_of(bits[1])));
        if (n == 3) {
            prod[5] = form_of(sub_forms(form_of(bits[0]), form_of(bits[2])));
            prod[6] = form_of(sub_forms(form_of(bits[1]), form_of(bits[2])));
            prod[7] = form_of(sub_forms(prod[3], form_of(bits[2])));
        }
        x.clear(); y.clear();
        for (unsigned mask = 0; mask < (1u << n); ++mask) {
            Fr cx = Fr::zero(), cy = Fr::zero();
            for (unsigned s = 0; s < (1u << n); ++s) {
                if (s & ~mask) continue;
                const bool odd = __builtin_popcount(mask ^ s) & 1;
                cx = odd ? cx - table[s].x : cx + table[s].x;
                cy = odd ? cy - table[s].y : cy + table[s].y;
            }
            form_add(x, prod[mask], cx);
            form_add(y, prod[mask], cy);
        }
    }
    static constexpr unsigned BABYJUB_GADGET_WINDOW = 3;
    // [sum 2^i bits[i]] Base8: every bit asserted, 3-bit windows from the least significant, the window's point selected from constant
    // multiples of Base8, one mixed addition per further window; the first window is the accumulator itself
    void babyjub_mul_fixed(const uint32_t* bits, size_t n, uint32_t out[3]) {
        if (n < 1 || n > 256) fail("babyjub_mul_fixed: n_bits must be in 1..256, got " + std::to_string(n));
        for (size_t i = 0; i < n; ++i) known(bits[i]);
        const std::vector<uint32_t> bit(bits, bits + n);   // out may alias bits
        const unsigned W = BABYJUB_GADGET_WINDOW;
        static const std::vector<BjAffine> table = babyjub_window_table(W, (256 + W - 1) / W);
        for (size_t i = 0; i < n; ++i) assert_bit(bit[i]);
        Form acc[3], x2, y2;
        for (size_t at = 0; at < n; at += W) {
            babyjub_select(bit.data() + at, std::min<size_t>(W, n - at), table.data() + ((at / W) << W), x2, y2);
            if (at == 0) { acc[0] = x2; acc[1] = y2; acc[2] = form_of(1); continue; }
            babyjub_add_forms(acc[0], acc[1], acc[2], x2, y2, nullptr, out);
            for (int i = 0; i < 3; ++i) acc[i] = form_of(out[i]);
        }
        if (n <= W) {                                       // one window: the two forms become wires
            out[0] = sub_forms(acc[0], form_of(1));
            out[1] = sub_forms(acc[1], form_of(1));
            out[2] = 1;
        }
    }
    // [sum 2^i bits[i]] P for an affine P the caller supplies: P asserted on the curve, every bit asserted, from the most significant
    // bit: the selection b Px, b (Py - 1) of P or the identity, and per further bit a doubling, the selection and a mixed addition
    void babyjub_mul(const uint32_t p_xy[2], const uint32_t* bits, size_t n, uint32_t out[3]) {
        if (n < 1 || n > 256) fail("babyjub_mul: n_bits must be in 1..256, got " + std::to_string(n));
        known(p_xy[0]); known(p_xy[1]);
        for (size_t i = 0; i < n; ++i) known(bits[i]);
        const std::vector<uint32_t> bit(bits, bits + n);
        const uint32_t px = p_xy[0], py = p_xy[1];
        babyjub_assert_on_curve(px, py);
        for (size_t i = 0; i < n; ++i) assert_bit(bit[i]);
        const Fr one = Fr::one();
        const Form fx = form_of(px), fy1 = form_sum(form_of(py), form_const(one), -one);
        Form x2, y2;
        auto select = [&](uint32_t bw) {
            x2 = form_of(sub_forms(form_of(bw), fx));
            y2 = form_sum(form_of(sub_forms(form_of(bw), fy1)), form_const(one), one);
        };
        select(bit[n - 1]);
        if (n == 1) {
            out[0] = x2.begin()->first;
            out[1] = sub_forms(y2, form_of(1));
            out[2] = 1;
            return;
        }
        Form acc[3] = {x2, y2, form_of(1)};
        for (size_t i = n - 1; i-- > 0;) {
            uint32_t d[3];
            babyjub_dbl_forms(acc[0], acc[1], acc[2], d);
            select(bit[i]);
            babyjub_add_forms(form_of(d[0]), form_of(d[1]), form_of(d[2]), x2, y2, nullptr, out);
            for (int k = 0; k < 3; ++k) acc[k] = form_of(out[k]);
        }
    }

    // ---- EdDSA-Poseidon (eddsa.hpp): [S] Base8 = R8 + [8] ([hm] A) with hm = H6(R8, A, M), from the gadgets above ----
    static constexpr size_t EDDSA_S_BITS = 251, EDDSA_HM_BITS = 254;
    // bits < bound through the comparator against constant wires, the result pinned to 1
    void assert_below(const uint32_t* bits, size_t n, const uint64_t* bound) {
        std::vector<uint32_t> k(n);
        for (size_t i = 0; i < n; ++i) k[i] = (uint32_t)((bound[i / 64] >> (i % 64)) & 1);   // ZK_WIRE_ONE or ZK_WIRE_ZERO
        const uint32_t lt = compare(ZK_CMP_LESS, bits, k.data(), n);
        assert_forms(form_sum(form_of(lt), form_const(Fr::one()), -Fr::one()), form_of(1));
    }
    // In this order: R8 on the curve; S < l; hm < r (circomlib's alias check: without it hm + r passes where it is below 2^254); the
    // digest; (sum 2^i hm_bits[i] - digest) * 1 = 0; [hm] A, which asserts A on the curve and every hm bit; three doublings; + R8;
    // [S] Base8, which asserts every S bit; and per coordinate X1 Z2 = t1, X2 Z1 = t2, (t1 - t2) * 1 = 0.
    void eddsa_verify(const uint32_t a_xy[2], const uint32_t r8_xy[2], uint32_t msg, const uint32_t* s_bits, const uint32_t* hm_bits) {
        known(a_xy[0]); known(a_xy[1]); known(r8_xy[0]); known(r8_xy[1]); known(msg);
        for (size_t i = 0; i < EDDSA_S_BITS; ++i) known(s_bits[i]);
        for (size_t i = 0; i < EDDSA_HM_BITS; ++i) known(hm_bits[i]);
        const Fr minus = -Fr::one();
        babyjub_assert_on_curve(r8_xy[0], r8_xy[1]);
        uint64_t r[4];
        for (int i = 0; i < 4; ++i) r[i] = (uint64_t)FrParams::P[2 * i] | ((uint64_t)FrParams::P[2 * i + 1] << 32);
        assert_below(s_bits, EDDSA_S_BITS, BABYJUB_ORDER);
        assert_below(hm_bits, EDDSA_HM_BITS, r);
        const Form in[5] = {form_of(r8_xy[0]), form_of(r8_xy[1]), form_of(a_xy[0]), form_of(a_xy[1]), form_of(msg)};
        const uint32_t digest = poseidon_forms_over(in, &poseidon_params_t6());
        Form sum;
        for (size_t i = 0; i < EDDSA_HM_BITS; ++i) {
            uint64_t w[4] = {0, 0, 0, 0};
            w[i / 64] = 1ull << (i % 64);
            form_add(sum, form_of(hm_bits[i]), Fr::from_canonical(fr_from_words(w)));
        }
        assert_forms(form_sum(sum, form_of(digest), minus), form_of(1));
        uint32_t p[3], q[3], left[3];
        babyjub_mul(a_xy, hm_bits, EDDSA_HM_BITS, p);
        for (int k = 0; k < 3; ++k) {
            babyjub_dbl_forms(form_of(p[0]), form_of(p[1]), form_of(p[2]), q);
            std::copy(q, q + 3, p);
        }
        babyjub_add_forms(form_of(p[0]), form_of(p[1]), form_of(p[2]), form_of(r8_xy[0]), form_of(r8_xy[1]), nullptr, q);
        babyjub_mul_fixed(s_bits, EDDSA_S_BITS, left);
        for (int k = 0; k < 2; ++k) {
            const Form t1 = form_of(sub_forms(form_of(left[k]), form_of(q[2]))), t2 = form_of(sub_forms(form_of(q[k]), form_of(left[2])));
            assert_forms(form_sum(t1, t2, minus), form_of(1));
        }
    }

    // ---- mod.rs:723-798, 939-950 ----
    uint32_t bit_check(uint32_t x) { return sub({{1, x}}, {{1, x}, {-1, 1}}, BOOL_ZERO, x, x); }
    uint32_t not_(uint32_t x) { return sub({{1, 1}}, {{1, 1}, {-1, x}}, BOOL_NOT, x, x); }
    uint32_t and_(uint32_t x, uint32_t y) { return sub({{1, x}}, {{1, y}}, BOOL_AND, x, y); }
    uint32_t or_(uint32_t x, uint32_t y) {
        const uint32_t t = and_(x, y);
        return sub({{-1, t}, {1, x}, {1, y}}, {{1, 1}}, BOOL_OR, x, y);
    }
    uint32_t xor_(uint32_t x, uint32_t y) { return sub({{1, x}, {-1, y}}, {{1, x}, {-1, y}}, BOOL_XOR, x, y); }
    uint32_t nand(uint32_t x, uint32_t y) { return not_(and_(x, y)); }
    uint32_t nor(uint32_t x, uint32_t y) {
        const uint32_t t = and_(x, y);
        return sub({{1, 1}, {1, t}, {-1, x}, {-1, y}}, {{1, 1}}, BOOL_NOR, x, y);
    }
    uint32_t xnor(uint32_t x, uint32_t y) { return sub({{1, 1}, {-1, x}, {1, y}}, {{1, 1}, {1, x}, {-1, y}}, BOOL_XNOR, x, y); }
    uint32_t less(uint32_t x, uint32_t y) { return sub({{1, 1}, {-1, x}}, {{1, y}}, BOOL_LESS, x, y); }
    uint32_t greater(uint32_t x, uint32_t y) { return sub({{1, 1}, {-1, y}}, {{1, x}}, BOOL_GREATER, x, y); }
    void assert_bit(uint32_t x) { sub({{1, x}}, {{1, x}, {-1, 1}}, BOOL_NONE, x, x, false); }

    uint32_t gate(int kind, uint32_t x, uint32_t y) {
        switch (kind) {
            case ZK_GATE_BIT_CHECK: return bit_check(x);
            case ZK_GATE_NOT: return not_(x);
            case ZK_GATE_AND: return and_(x, y);
            case ZK_GATE_OR: return or_(x, y);
            case ZK_GATE_XOR: return xor_(x, y);
            case ZK_GATE_NAND: return nand(x, y);
            case ZK_GATE_NOR: return nor(x, y);
            case ZK_GATE_XNOR: return xnor(x, y);
            case ZK_GATE_LESS: return less(x, y);
            case ZK_GATE_GREATER: return greater(x, y);
        }
        fail("unknown gate kind " + std::to_string(kind));
    }
    static bool unary(int kind) { return kind == ZK_GATE_BIT_CHECK || kind == ZK_GATE_NOT; }

    // ---- mod.rs:995-1241 ----
    uint32_t is_equal(const uint32_t* l, const uint32_t* r, size_t n) {
        uint32_t acc = xnor(l[0], r[0]);
        for (size_t i = 1; i < n; ++i) {
            const uint32_t eq = xnor(l[i], r[i]);
            acc = and_(eq, acc);
        }
        return acc;
    }
    uint32_t is_equal_zero(const uint32_t* x, size_t n) {
        uint32_t acc = xnor(x[0], 0);
        for (size_t i = 1; i < n; ++i) {
            const uint32_t eq = xnor(x[i], 0);
            acc = and_(eq, acc);
        }
        return acc;
    }
    // one bit: the reference's fold runs fan_in over an empty list of equalities and panics; the single new_greater_than gate is the answer
    uint32_t greater_than(const uint32_t* l, const uint32_t* r, size_t n) {
        const uint32_t cmp0 = greater(l[0], r[0]);
        if (n == 1) return cmp0;
        std::vector<uint32_t> cmp, eq;
        for (size_t i = 1; i < n; ++i) {
            cmp.push_back(greater(l[i], r[i]));
            eq.push_back(xnor(l[i], r[i]));
        }
        uint32_t acc = cmp.back();
        cmp.pop_back();
        cmp.insert(cmp.begin(), cmp0);
        for (size_t k = 0; k < cmp.size(); ++k) {
            uint32_t all_eq = eq[k];
            for (size_t i = k + 1; i < eq.size(); ++i) all_eq = and_(all_eq, eq[i]);
            const uint32_t both = and_(cmp[k], all_eq);
            acc = or_(acc, both);
        }
        return acc;
    }
    uint32_t compare(int kind, const uint32_t* l, const uint32_t* r, size_t n) {
        switch (kind) {
            case ZK_CMP_EQUAL: return is_equal(l, r, n);
            case ZK_CMP_EQUAL_ZERO: return is_equal_zero(l, n);
            case ZK_CMP_GREATER: return greater_than(l, r, n);
            case ZK_CMP_LESS: {
                const uint32_t neg = not_(greater_than(l, r, n));
                const uint32_t neg_eq = not_(is_equal(l, r, n));
                return and_(neg, neg_eq);
            }
            case ZK_CMP_LESS_EQ: {
                const uint32_t neg = not_(greater_than(l, r, n));
                return or_(neg, is_equal(l, r, n));
            }
            case ZK_CMP_GREATER_EQ: {
                const uint32_t gt = greater_than(l, r, n);
                return or_(gt, is_equal(l, r, n));
            }
        }
        fail("unknown comparator " + std::to_string(kind));
    }

    // ---- mod.rs:1247-1398 ----
    typedef std::array<uint32_t, 64> Lane;   // a Word64, least significant bit first
    static Lane rotl(const Lane& x, unsigned by) {
        Lane o;
        for (unsigned i = 0; i < 64; ++i) o[i] = x[(i + 64 - by % 64) % 64];
        return o;
    }
    Lane xor64(const Lane& x, const Lane& y) {
        Lane o;
        for (unsigned i = 0; i < 64; ++i) o[i] = xor_(x[i], y[i]);
        return o;
    }
    void keccak_f(Lane* a, unsigned rounds) {
        for (unsigned rnd = 0; rnd < rounds; ++rnd) {
            Lane col[5];
            for (auto& c : col) c.fill(0);
            for (unsigned x = 0; x < 5; ++x)                 // theta: column parities, folded from the zero word
                for (unsigned y = 0; y < 25; y += 5) col[x] = xor64(col[x], a[x + y]);
            for (unsigned x = 0; x < 5; ++x)
                for (unsigned y = 0; y < 25; y += 5) {
                    const Lane t = xor64(a[y + x], col[(x + 4) % 5]);
                    a[y + x] = xor64(t, rotl(col[(x + 1) % 5], 1));
                }
            Lane last = a[1];                                // rho and pi: a renaming
            for (unsigned x = 0; x < 24; ++x) {
                const Lane keep = a[KECCAK_PI[x]];
                a[KECCAK_PI[x]] = rotl(last, KECCAK_RHO[x]);
                last = keep;
            }
            for (unsigned y = 0; y < 25; y += 5) {           // chi
                Lane row[5];
                for (unsigned x = 0; x < 5; ++x) row[x] = a[y + x];
                for (unsigned x = 0; x < 5; ++x) {
                    Lane n, c;
                    for (unsigned i = 0; i < 64; ++i) n[i] = not_(row[(x + 1) % 5][i]);
                    for (unsigned i = 0; i < 64; ++i) c[i] = and_(n[i], row[(x + 2) % 5][i]);
                    a[y + x] = xor64(row[x], c);
                }
            }
            Lane rc;                                         // iota
            for (unsigned i = 0; i < 64; ++i) rc[i] = (uint32_t)((KECCAK_RC[rnd] >> i) & 1);
            a[0] = xor64(a[0], rc);
        }
    }
    void keccak(const uint32_t* in, size_t n_bytes, unsigned rate, unsigned delim, unsigned rounds, uint32_t* out, size_t out_bytes) {
        if (rate < 1 || rate > 200) fail("keccak: rate_bytes must be in 1..200");
        if (rounds < 1 || rounds > 24) fail("keccak: rounds must be in 1..24");
        if (delim > 0xff) fail("keccak: delim is one byte");
        for (size_t i = 0; i < 8 * n_bytes; ++i) known(in[i]);
        Lane a[25];
        for (auto& l : a) l.fill(0);
        auto xor_byte = [&](unsigned at, const uint32_t* src) {
            for (unsigned i = 0; i < 8; ++i) a[at / 8][8 * (at % 8) + i] = xor_(a[at / 8][8 * (at % 8) + i], src[i]);
        };
        unsigned offset = 0;
        for (size_t k = 0; k < n_bytes; ++k) {
            xor_byte(offset, in + 8 * k);
            if (++offset == rate) { keccak_f(a, rounds); offset = 0; }
        }
        uint32_t cst[8];
        for (unsigned i = 0; i < 8; ++i) cst[i] = (delim >> i) & 1;
        xor_byte(offset, cst);
        for (unsigned i = 0; i < 8; ++i) cst[i] = (0x80u >> i) & 1;
        xor_byte(rate - 1, cst);
        keccak_f(a, rounds);
        size_t op = 0, left = out_bytes;
        auto copy = [&](size_t count) {
            for (size_t k = 0; k < count; ++k)
                for (unsigned i = 0; i < 8; ++i) out[8 * (op + k) + i] = a[k / 8][8 * (k % 8) + i];
        };
        while (left >= rate) {
            copy(rate);
            keccak_f(a, rounds);
            op += rate;
            left -= rate;
        }
        copy(left);
    }
};

// ---- finishing ------------------------------------------------------------------------------------
// stable counting sort of operations by level; returns level_ptr (levels + 1 entries)
template <class Op>
static std::vector<uint32_t> sort_by_level(std::vector<Op>& ops, const std::vector<uint32_t>& op_level) {
    uint32_t levels = 0;
    for (uint32_t lv : op_level) levels = std::max(levels, lv);
    std::vector<uint32_t> ptr(levels + 1, 0);
    for (uint32_t lv : op_level) ++ptr[lv];
    for (uint32_t l = 1; l <= levels; ++l) ptr[l] += ptr[l - 1];
    std::vector<uint32_t> at(ptr.begin(), ptr.end());
    std::vector<Op> sorted(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) sorted[at[op_level[i] - 1]++] = ops[i];
    ops.swap(sorted);
    return ptr;
}

// Sub-circuits as operations of a zk::Tape (witgen_tape.hpp): a scaled sum is MUL by a pooled constant and ADD into fresh temporaries,
// a weight of one reads the operand itself, an entry on the constant 1 is the pooled weight, and a side that repeats the other (XOR)
// is summed once.  `take(k)` says whether sub-circuit k is compiled, `ref(i, copy)` is the operand word of witness index i > 0 (for
// an output, its slot), where copy(x) emits a COPY of operand word x into a fresh temporary and returns that slot; `tags` are the bits
// that mark an operand word as no slot.  Returns the level of every operation, in order.
template <class Take, class Ref>
static std::vector<uint32_t> built_compile_subs(const Built& p, Tape& t, uint32_t tags, Take&& take, Ref&& ref) {
    std::vector<uint32_t> slot_level(t.slots, 0), op_level;
    std::map<std::array<uint32_t, 8>, uint32_t> pool;
    auto constant = [&](const Fr& v) {
        std::array<uint32_t, 8> key;
        for (int i = 0; i < 8; ++i) key[i] = v.l[i];
        auto it = pool.find(key);
        if (it == pool.end()) { it = pool.emplace(key, (uint32_t)t.consts.size()).first; t.consts.push_back(v); }
        return it->second | TAPE_CONST;
    };
    auto fresh = [&]() { slot_level.push_back(0); return (uint32_t)t.slots++; };
    auto level_of = [&](uint32_t x) { return (x & tags) ? 0u : slot_level[x]; };
    auto emit = [&](uint32_t kind, uint32_t dst, uint32_t a, uint32_t b) {
        const uint32_t lv = 1 + std::max(level_of(a), level_of(b));
        t.ops.push_back({dst, a, b, kind});
        op_level.push_back(lv);
        slot_level[dst] = lv;
        return dst;
    };
    const Fr one = Fr::one();
    auto copy = [&](uint32_t x) { return emit(TAPE_COPY, fresh(), x, constant(Fr::zero())); };   // (b is not read)
    auto side = [&](uint32_t from, uint32_t to) {
        uint32_t acc = 0;
        bool any = false;
        for (uint32_t e = from; e < to; ++e) {
            const BuiltTerm& x = p.terms[e];
            uint32_t v;
            if (x.wit == 0) v = constant(x.w);
            else if (x.w == one) v = ref(x.wit, copy);
            else v = emit(TAPE_MUL, fresh(), constant(x.w), ref(x.wit, copy));
            acc = any ? emit(TAPE_ADD, fresh(), acc, v) : v;
            any = true;
        }
        return any ? acc : constant(Fr::zero());
    };
    auto same_sides = [&](const BuiltSub& s) {
        if (s.r0 - s.l0 != s.end - s.r0) return false;
        for (uint32_t i = 0; i < s.r0 - s.l0; ++i)
            if (p.terms[s.l0 + i].wit != p.terms[s.r0 + i].wit || p.terms[s.l0 + i].w != p.terms[s.r0 + i].w) return false;
        return true;
    };
    for (size_t k = 0; k < p.subs.size(); ++k) {
        const BuiltSub& s = p.subs[k];
        if (s.out == WIT_NONE || !take(k)) continue;   // an assertion computes nothing
        const uint32_t l = side(s.l0, s.r0);
        const uint32_t r = same_sides(s) ? l : side(s.r0, s.end);
        emit(TAPE_MUL, ref(s.out, copy), l, r);
    }
    return op_level;
}

// The whole circuit as the tape of witgen.hip: slot = witness index, temporaries behind the witness.
static void built_compile_tape(zk_circuit& c) {
    const Built& p = *c.built;
    Tape& t = c.tape;
    const size_t m = c.u.size();
    t.n_in = p.in_wit.size();
    t.m = m;
    t.slots = m;
    t.in_slot = p.in_wit;
    t.in_bit.resize(t.n_in);
    for (size_t i = 0; i < t.n_in; ++i) t.in_bit[i] = p.in_bit[i] ? p.in_wire[i] + 1 : 0;
    const std::vector<uint32_t> op_level = built_compile_subs(p, t, TAPE_CONST, [](size_t) { return true; }, [](uint32_t i, auto&&) { return i; });
    std::vector<uint32_t> node_level(m, 0), per_level;
    for (const BuiltSub& s : p.subs) {
        if (s.out == WIT_NONE) continue;
        uint32_t node = 0;
        for (uint32_t e = s.l0; e < s.end; ++e) node = std::max(node, node_level[p.terms[e].wit]);
        node_level[s.out] = ++node;
        if (per_level.size() < node) per_level.resize(node, 0);
        ++per_level[node - 1];
    }
    if (t.slots >= TAPE_CONST || t.ops.size() >= TAPE_CONST) {
        t.status = ZK_ERR_SIZE;
        t.error = "circuit too large for the witness tape";
        t.ops.clear(); t.consts.clear(); t.in_slot.clear(); t.in_bit.clear();
        t.slots = 0;
        return;
    }
    t.depth = per_level.size();
    for (uint32_t n : per_level) t.width = std::max<size_t>(t.width, n);
    t.level_ptr = sort_by_level(t.ops, op_level);
}

// The split into a boolean core and a field tail (circuit.hpp: Mixed), for every built circuit.  `wit` maps the builder's wire ids
// to witness indices; b.subs and p.subs run in parallel.
static void built_split(zk_circuit& c, const zk_builder& b, const std::vector<uint32_t>& wit) {
    Built& p = *c.built;
    Mixed& x = p.mix;
    Tape& t = x.tail;
    const size_t m = c.u.size();
    const char* too_large = "builder: circuit too large: its indices leave no room for the operand tags of the field tail";
    if (m + 1 >= MIX_BIT || p.pack_out.size() >= MIX_BIT) throw ParseError{ZK_ERR_SIZE, too_large};
    auto idx = [&](uint32_t wire) { return wit[wire] == WIT_NONE ? (uint32_t)m : wit[wire]; };   // index m stands for the constant 0
    x.field.assign(m + 1, 0);
    std::vector<uint32_t> ref(m, 0);                          // per witness index: its operand word in the tail
    for (size_t i = 0; i < m; ++i) ref[i] = MIX_BIT | (uint32_t)i;
    auto new_slot = [&](uint32_t index) {
        x.field[index] = 1;
        ref[index] = (uint32_t)x.slot_wit.size();
        x.slot_wit.push_back(index);
    };
    for (size_t i = 0; i < p.in_wit.size(); ++i) {
        if (p.in_bit[i]) { x.bit_in_wit.push_back(p.in_wit[i]); continue; }
        t.in_slot.push_back((uint32_t)x.slot_wit.size());
        new_slot(p.in_wit[i]);
    }
    t.n_in = t.in_slot.size();
    std::vector<uint32_t> level(m + 1, 0), op_level;
    std::vector<uint8_t> in_tail(b.subs.size(), 0);
    for (size_t k = 0; k < b.subs.size(); ++k) {
        const zk_builder::Sub& s = b.subs[k];
        if (s.out == WIT_NONE) continue;
        const uint32_t out = wit[s.out];
        if (s.bkind <= BOOL_GREATER && !x.field[idx(s.a)] && !x.field[idx(s.b)]) {
            const BoolOp op{out, idx(s.a), idx(s.b), s.bkind};
            const uint32_t lv = 1 + std::max(level[op.a], level[op.b]);
            level[out] = lv;
            x.core_ops.push_back(op);
            op_level.push_back(lv);
            continue;
        }
        bool core = s.bkind == BOOL_PACK;
        for (uint32_t e = s.l0; core && e < s.r0; ++e) core = !x.field[idx(b.terms[e].wire)];
        if (s.bkind == BOOL_PACK) x.pack_core.push_back(core);
        if (core) {                                           // gathered from the operands' bits: no tail slot
            x.field[out] = 1;
            ref[out] = MIX_PACK | (uint32_t)x.cpack_out.size();
            x.cpack_out.push_back(out);
            for (uint32_t e = s.l0; e < s.r0; ++e) x.cpack_bits.push_back(idx(b.terms[e].wire));
            x.cpack_ptr.push_back((uint32_t)x.cpack_bits.size());
        } else {
            new_slot(out);
            in_tail[k] = 1;
        }
    }
    x.core_level_ptr = sort_by_level(x.core_ops, op_level);
    t.m = m;
    t.slots = x.slot_wit.size();
    const std::vector<uint32_t> tail_level = built_compile_subs(p, t, MIX_TAG, [&](size_t k) { return in_tail[k] != 0; },
                                                                 [&](uint32_t i, auto&& copy) {   // a core pack is gathered once, at its first reader
                                                                     if ((ref[i] & MIX_TAG) == MIX_PACK) ref[i] = copy(ref[i]);
                                                                     return ref[i];
                                                                 });
    if (t.slots >= MIX_BIT || t.ops.size() >= MIX_BIT || t.consts.size() >= MIX_BIT) throw ParseError{ZK_ERR_SIZE, too_large};
    t.level_ptr = sort_by_level(t.ops, tail_level);
}

static zk_circuit* builder_finish(zk_builder& b, const uint32_t* verify, size_t n_verify) {
    BuilderOps ops{b};
    ops.live();
    const size_t wires = b.kind.size();
    const uint32_t UNSET = 0xfffffffeu;
    std::vector<uint32_t> wit(wires, UNSET);
    uint32_t next = 1;
    for (size_t i = 0; i < n_verify; ++i) {
        ops.known(verify[i]);
        if (verify[i] < 2) BuilderOps::fail("verify wire " + std::to_string(verify[i]) + " is a constant");
        if (wit[verify[i]] != UNSET) BuilderOps::fail("verify wire " + std::to_string(verify[i]) + " is named twice");
        wit[verify[i]] = next++;
    }
    for (size_t w = 2; w < wires; ++w)
        if ((b.kind[w] == 1 || b.kind[w] == 2) && wit[w] == UNSET) wit[w] = next++;
    for (size_t w = 2; w < wires; ++w)
        if (wit[w] == UNSET) wit[w] = next++;
    wit[0] = WIT_NONE;   // the constant zero: no witness wire, its entries are dropped
    wit[1] = 0;
    const size_t m = next;

    std::unique_ptr<zk_circuit> c(new zk_circuit());
    c->u.resize(m); c->v.resize(m); c->w.resize(m);
    c->input = n_verify;
    c->n_gates = b.subs.size();
    c->built.reset(new Built());
    Built& p = *c->built;
    const Fr one = Fr::one();
    p.subs.reserve(b.subs.size());
    p.terms.reserve(b.terms.size());
    for (size_t k = 0; k < b.subs.size(); ++k) {
        const zk_builder::Sub& s = b.subs[k];
        BuiltSub o;
        o.l0 = (uint32_t)p.terms.size();
        for (uint32_t e = s.l0; e < s.r0; ++e) {
            const uint32_t x = wit[b.terms[e].wire];
            if (x == WIT_NONE) continue;
            p.terms.push_back({b.terms[e].w, x});
            c->u[x].push_back({(uint32_t)k, b.terms[e].w});
        }
        o.r0 = (uint32_t)p.terms.size();
        for (uint32_t e = s.r0; e < s.end; ++e) {
            const uint32_t x = wit[b.terms[e].wire];
            if (x == WIT_NONE) continue;
            p.terms.push_back({b.terms[e].w, x});
            c->v[x].push_back({(uint32_t)k, b.terms[e].w});
        }
        o.end = (uint32_t)p.terms.size();
        o.out = s.out == WIT_NONE ? WIT_NONE : wit[s.out];
        if (o.out != WIT_NONE) c->w[o.out].push_back({(uint32_t)k, one});
        p.subs.push_back(o);
        if (s.bkind == BOOL_PACK) {
            p.pack_out.push_back(o.out);
            for (uint32_t e = s.l0; e < s.r0; ++e) p.pack_bits.push_back(wit[b.terms[e].wire] == WIT_NONE ? (uint32_t)m : wit[b.terms[e].wire]);
            p.pack_ptr.push_back((uint32_t)p.pack_bits.size());
        }
    }
    p.boolean = b.boolean;
    p.wire_wit = wit;
    for (size_t w = 2; w < wires; ++w)
        if (b.kind[w] == 1 || b.kind[w] == 2) {
            p.in_wit.push_back(wit[w]);
            p.in_wire.push_back((uint32_t)w);
            p.in_bit.push_back(b.kind[w] == 1);
            if (b.kind[w] == 2) p.boolean = false;
        }
    if (p.boolean) {
        // witness index m stands for the constant 0
        auto idx = [&](uint32_t wire) { return wit[wire] == WIT_NONE ? (uint32_t)m : wit[wire]; };
        std::vector<uint32_t> level(m + 1, 0), op_level;
        for (const zk_builder::Sub& s : b.subs) {
            if (s.out == WIT_NONE || s.bkind == BOOL_PACK) continue;   // an assertion computes nothing; a pack is no boolean operation
            const BoolOp op{wit[s.out], idx(s.a), idx(s.b), s.bkind};
            const uint32_t lv = 1 + std::max(level[op.a], level[op.b]);
            level[op.dst] = lv;
            p.bool_ops.push_back(op);
            op_level.push_back(lv);
        }
        p.bool_level_ptr = sort_by_level(p.bool_ops, op_level);
    }
    built_compile_tape(*c);
    built_split(*c, b, wit);
    b.finished = true;
    b.terms.clear(); b.terms.shrink_to_fit();
    b.subs.clear(); b.subs.shrink_to_fit();
    return c.release();
}

// ---- the two host evaluators ----------------------------------------------------------------------
// inputs of a built circuit: canonical words < r, and 0 or 1 where the wire was made as a bit
static void built_check_inputs(const Tape& t, const uint64_t* inputs, size_t n_in) {
    for (size_t i = 0; i < n_in; ++i)
        if (!fr_from_words(inputs + 4 * i).raw_in_range()) throw ParseError{ZK_ERR_RANGE, "input value >= r"};
    for (size_t i = 0; i < n_in && i < t.in_bit.size(); ++i)
        if (t.in_bit[i] && (inputs[4 * i] > 1 || inputs[4 * i + 1] || inputs[4 * i + 2] || inputs[4 * i + 3]))
            throw ParseError{ZK_ERR_RANGE, bit_input_error(0, i, t.in_bit[i] - 1)};
}
// the sub-circuits in creation order: what the reference's memoised `evaluate` (mod.rs:559-595) computes for every wire
static void built_weights(const zk_circuit& c, const uint64_t* inputs, size_t n_in, uint64_t* out, size_t m) {
    const Built& p = *c.built;
    auto serr = [](const std::string& s) { return ParseError{ZK_ERR_ARG, "StructureErr(None, " + s + ")"}; };
    if (p.in_wit.size() != n_in) throw serr("Wrong number of values supplied");
    if (m != c.u.size()) throw serr("weights buffer size mismatch");
    built_check_inputs(c.tape, inputs, n_in);
    std::vector<Fr> vals(m, Fr::zero());
    vals[0] = Fr::one();
    for (size_t i = 0; i < n_in; ++i) vals[p.in_wit[i]] = Fr::from_canonical(fr_from_words(inputs + 4 * i));
    for (const BuiltSub& s : p.subs) {
        if (s.out == WIT_NONE) continue;
        Fr l = Fr::zero(), r = Fr::zero();
        for (uint32_t e = s.l0; e < s.r0; ++e) l = l + p.terms[e].w * vals[p.terms[e].wit];
        for (uint32_t e = s.r0; e < s.end; ++e) r = r + p.terms[e].w * vals[p.terms[e].wit];
        vals[s.out] = l * r;
    }
    for (size_t i = 0; i < m; ++i) fr_to_words(vals[i].to_canonical(), out + 4 * i);
}

// One witness through the split (circuit.hpp: Mixed): what mixgen.hip's kernels compute for one instance, without a GPU.  Bit inputs
// are bits (bit k of in_bits = the k-th ZK_WIRE_BIT input), the core is uint64_t logic on one word whose bit 0 is the instance, a
// core pack is its operands' bits gathered, the tail runs over Fr.  Field inputs: 4 canonical words each, in input order.
static void mixed_run_host(const zk_circuit& c, const uint8_t* in_bits, size_t n_bit_bytes, const uint64_t* in_fields, size_t n_field, uint64_t* out,
                           size_t m) {
    const Mixed& x = c.built->mix;
    const Tape& t = x.tail;
    auto serr = [](const std::string& s) { return ParseError{ZK_ERR_ARG, "StructureErr(None, " + s + ")"}; };
    if (n_bit_bytes != (x.bit_in_wit.size() + 7) / 8 || n_field != t.n_in) throw serr("Wrong number of values supplied");
    if (m != c.u.size()) throw serr("weights buffer size mismatch");
    for (size_t i = 0; i < n_field; ++i)
        if (!fr_from_words(in_fields + 4 * i).raw_in_range()) throw ParseError{ZK_ERR_RANGE, "input value >= r"};
    std::vector<uint64_t> state(m + 1, 0);
    state[0] = ~0ull;
    for (size_t k = 0; k < x.bit_in_wit.size(); ++k) state[x.bit_in_wit[k]] = (in_bits[k / 8] >> (k % 8)) & 1 ? ~0ull : 0;
    for (const BoolOp& op : x.core_ops) state[op.dst] = bool_apply(op.kind, state[op.a], state[op.b]);
    auto gather = [&](uint32_t pk, uint64_t* w) {
        w[0] = w[1] = w[2] = w[3] = 0;
        for (uint32_t e = x.cpack_ptr[pk]; e < x.cpack_ptr[pk + 1]; ++e) {
            const uint32_t at = e - x.cpack_ptr[pk];
            w[at / 64] |= (state[x.cpack_bits[e]] & 1) << (at % 64);
        }
    };
    std::vector<Fr> vals(t.slots);
    for (size_t i = 0; i < n_field; ++i) vals[t.in_slot[i]] = Fr::from_canonical(fr_from_words(in_fields + 4 * i));
    auto operand = [&](uint32_t r) {
        const uint32_t i = r & MIX_INDEX;
        switch (r & MIX_TAG) {
            case TAPE_CONST: return t.consts[i];
            case MIX_BIT: return state[i] & 1 ? Fr::one() : Fr::zero();
            case MIX_PACK: { uint64_t w[4]; gather(i, w); return Fr::from_canonical(fr_from_words(w)); }
            default: return vals[i];
        }
    };
    for (const TapeOp& op : t.ops) {
        const Fr a = operand(op.a), b = operand(op.b);
        vals[op.dst] = op.kind == TAPE_COPY ? a : op.kind == TAPE_MUL ? a * b : a + b;
    }
    for (size_t i = 0; i < m; ++i) {
        out[4 * i] = state[i] & 1;
        out[4 * i + 1] = out[4 * i + 2] = out[4 * i + 3] = 0;
    }
    for (size_t pk = 0; pk < x.cpack_out.size(); ++pk) gather((uint32_t)pk, out + 4 * (size_t)x.cpack_out[pk]);
    for (size_t s = 0; s < x.slot_wit.size(); ++s) fr_to_words(vals[s].to_canonical(), out + 4 * (size_t)x.slot_wit[s]);
}

}  // namespace zk
