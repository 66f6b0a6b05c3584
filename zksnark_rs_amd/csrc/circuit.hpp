// circuit.hpp -- zk_circuit, the handle both front ends produce: the .zk parser (frontend.hip) and the gate-level builder
// (builder.hpp).  Rows, dimensions and the witness tape are common; a parsed circuit also keeps its program, a built one its
// sub-circuits over witness indices, where every gate is boolean the bit-sliced tape of boolgen.hip, and always the split into a
// boolean core and a field tail that mixgen.hip runs.
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
// one boolean operation on 64 instances at once (boolgen_kernels.cuh) or on one (mixed_run_host)
ZK_HD uint64_t bool_apply(uint32_t kind, uint64_t a, uint64_t b) {
    switch (kind) {
        case BOOL_NOT: return ~a;
        case BOOL_AND: return a & b;
        case BOOL_OR: return a | b;
        case BOOL_XOR: return a ^ b;
        case BOOL_NOR: return ~(a | b);
        case BOOL_XNOR: return ~(a ^ b);
        case BOOL_LESS: return ~a & b;
        case BOOL_GREATER: return a & ~b;
        default: return 0;                    // BOOL_ZERO
    }
}

// ---- the split of a built circuit into a boolean core and a field tail (builder.hpp: built_split; mixgen.hip) -------------
// A witness index is BIT-class if it is the constant 1, a ZK_WIRE_BIT input, or the output of a sub-circuit of a boolean kind whose
// operands a, b are bit-class; every other index is FIELD-class (field inputs, general sub-circuits, packed wires, whatever reads
// one of these).  Nothing bit-class reads anything field-class, so the circuit is a core followed by a tail.
// A tail operand is a 32-bit word whose two top bits say what the other 30 are:
constexpr uint32_t MIX_TAG = 0xc0000000u, MIX_INDEX = ~MIX_TAG;
constexpr uint32_t MIX_SLOT = 0;              // a tail slot (an operation's dst is always one: a word without tag bits)
constexpr uint32_t MIX_BIT = 0x40000000u;     // a bit-class witness index; index m = the constant 0, index 0 = the constant 1
constexpr uint32_t MIX_PACK = 0xc0000000u;    // a core pack's number: the field element gathered from its operands' bits
static_assert(TAPE_CONST == 0x80000000u, "a pooled constant keeps the tape's own tag");
struct Mixed {
    std::vector<uint8_t> field;            // per witness index: 1 = field-class
    std::vector<uint32_t> bit_in_wit;      // the k-th ZK_WIRE_BIT input's witness index, in input order
    std::vector<BoolOp> core_ops;          // the bit-class sub-circuits, sorted by level; Built::bool_ops where the circuit is boolean
    std::vector<uint32_t> core_level_ptr;
    std::vector<uint8_t> pack_core;        // per pack of Built: 1 = every operand bit-class, gathered; 0 = a tail operation
    std::vector<uint32_t> cpack_out, cpack_ptr{0}, cpack_bits;   // the core packs alone, as Built's CSR lists
    // The tail: a Tape over tail slots.  Slots are dense: the n_in field inputs in input order, then the field-class witness wires
    // the tail computes, then temporaries; slot_wit maps the first two groups to their witness indices.  in_slot[i] = i.
    Tape tail;
    std::vector<uint32_t> slot_wit;
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
    Mixed mix;                             // recorded for every built circuit, boolean or not
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
