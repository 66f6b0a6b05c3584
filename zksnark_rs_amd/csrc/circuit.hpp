// circuit.hpp -- zk_circuit, the handle both front ends produce: the .zk parser (frontend.hip) and the gate-level builder
// (builder.hpp).  Rows, dimensions and the witness tape are common; a parsed circuit also keeps its program, a built one its
// sub-circuits over witness indices and, where every gate is boolean, the bit-sliced tape of boolgen.hip.
#pragma once
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "witgen_tape.hpp"

namespace zk {

struct ParseError {
    int status;
    std::string msg;
};

struct Node {
    enum Kind { In, Out, Verify, Program, Assign, Mul, Add, Var, Literal } kind;
    std::vector<Node> kids;
    std::string var;
    Fr lit{};
};

// ---- what zk_builder_finish leaves behind (builder.hpp) -----------------------------------------
constexpr uint32_t WIT_NONE = 0xffffffffu;   // a sub-circuit without output wire (zk_builder_assert_bit)
struct BuiltTerm {
    Fr w;            // weight, Montgomery form
    uint32_t wit;    // witness index; entries on the constant-zero wire are dropped at finish
};
struct BuiltSub {    // (sum of terms[l0, r0)) * (sum of terms[r0, end)) = witness[out]
    uint32_t l0, r0, end, out;
};
// one boolean operation per sub-circuit of a boolean circuit: dst, a, b are witness indices; index m is the constant 0, index 0 the
// constant 1.  LESS = !a & b, GREATER = a & !b (builder/mod.rs:939-950); ZERO is the bit checker's output x (x - 1).
// NONE marks a sub-circuit that is no boolean operation, PACK the one of zk_builder_pack: its output is a field element, not a bit.
enum BoolKind : uint32_t { BOOL_ZERO = 0, BOOL_NOT, BOOL_AND, BOOL_OR, BOOL_XOR, BOOL_NOR, BOOL_XNOR, BOOL_LESS, BOOL_GREATER, BOOL_NONE, BOOL_PACK };
struct BoolOp {
    uint32_t dst, a, b, kind;
};
struct Built {
    std::vector<BuiltTerm> terms;
    std::vector<BuiltSub> subs;            // creation order = a topological order
    std::vector<uint32_t> in_wit, in_wire; // per input: witness index, the builder's wire id
    std::vector<uint8_t> in_bit;           // per input: 1 = ZK_WIRE_BIT (values other than 0 and 1 are refused)
    std::vector<uint32_t> wire_wit;        // per builder wire id: witness index, WIT_NONE for the constant zero
    bool boolean = false;
    std::vector<BoolOp> bool_ops;          // sorted by level (stable), as the field tape
    std::vector<uint32_t> bool_level_ptr;  // levels + 1 entries
    // zk_builder_pack, in CSR form: pack p has output witness index pack_out[p] and operands pack_bits[pack_ptr[p] .. pack_ptr[p + 1]),
    // witness indices in bit order (position in the list = bit position; index m is the constant 0 and keeps its place, index 0 the
    // constant 1).  Kept whether the circuit is boolean or not.
    std::vector<uint32_t> pack_out, pack_ptr{0}, pack_bits;
};

static inline std::string bit_input_error(size_t instance, size_t input, uint32_t wire) {
    return "input " + std::to_string(input) + " (bit wire " + std::to_string(wire) + ") of instance " + std::to_string(instance) + " is not 0 or 1";
}

}  // namespace zk

// DummyRep (dummy_rep.rs:6-13) for Fr + what circuit::weights needs
struct zk_circuit {
    typedef std::vector<std::pair<uint32_t, zk::Fr>> Row;   // (gate index 0-based, value in Montgomery form)
    std::vector<Row> u, v, w;
    size_t n_gates = 0, input = 0;
    std::vector<zk::Node> exprs;
    std::vector<std::string> order;    // variable_order (ast.rs:62-83)
    std::string last_error;
    zk::Tape tape;                     // circuit::weights compiled once (witgen_tape.hpp), or its static error
    std::unique_ptr<zk::Built> built;  // set by zk_builder_finish, null for a parsed circuit
};
