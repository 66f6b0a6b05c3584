// witgen_tape.hpp -- circuit::weights (circuit/mod.rs:529-637) compiled once per program into a flat tape of field operations over
// numbered slots.  frontend.hip builds it inside zk_circuit_parse; the host interpreter below (zk_circuit_weights_tape) and the device
// kernel (witgen.hip: one instance per lane) run the same tape, so the interpreter is the kernel's model without a GPU.
//
//   slots     0 = the constant 1, i + 1 = variable_order[i] (the witness in its output order, m slots), then from m on the `in`
//             variables that never reach the witness and the temporaries of nested expressions
//   operand   a slot, or with TAPE_CONST set an index into the constant pool (the program's literals, Montgomery form)
//   op        dst = a * b | dst = a + b | dst = a.  Single assignment: no slot is written twice (the program's own variables by the
//             reference's "already assigned" rule, temporaries because each is fresh), so levels are well defined:
//   level     inputs and constants are level 0, an operation is 1 + the highest level among the operations whose results it reads.
//             ops are sorted by level (stable: program order inside a level); level_ptr[L] .. level_ptr[L + 1] are the operations of
//             level L + 1.  Operations of one level are independent of each other.
// Field arithmetic is exact, so any order of evaluation gives the canonical words of the reference's recursive `evaluate`.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/zkgpu.h"
#include "ff.cuh"

namespace zk {

constexpr uint32_t TAPE_CONST = 0x80000000u;
enum TapeKind : uint32_t { TAPE_MUL = 0, TAPE_ADD = 1, TAPE_COPY = 2 };
struct TapeOp {
    uint32_t dst, a, b, kind;   // b is unused by a copy
};

struct Tape {
    // the static part of circuit::weights' errors: a program that fails for every input keeps status and text here in place of a tape
    int status = 0;
    std::string error;
    size_t n_in = 0, m = 0, slots = 0;
    size_t depth = 0, width = 0;          // shape of the program with each `=` as one node (zk_circuit_tape_dims)
    std::vector<uint32_t> in_slot;        // slot of input i (every input owns one, read or not: all are range-checked)
    std::vector<uint32_t> in_bit;         // built circuits only (else empty): 1 + the builder's wire id where input i must be 0 or 1, 0 where any field element
    std::vector<TapeOp> ops;              // sorted by level
    std::vector<uint32_t> level_ptr;      // levels + 1 entries
    std::vector<Fr> consts;
    size_t levels() const { return level_ptr.empty() ? 0 : level_ptr.size() - 1; }
    size_t max_level_width() const {
        size_t w = 0;
        for (size_t l = 0; l + 1 < level_ptr.size(); ++l) w = std::max<size_t>(w, level_ptr[l + 1] - level_ptr[l]);
        return w;
    }
};

static inline Fr fr_from_words(const uint64_t* w) {
    Fr x;
    for (int k = 0; k < 4; ++k) { x.l[2 * k] = (uint32_t)w[k]; x.l[2 * k + 1] = (uint32_t)(w[k] >> 32); }
    return x;
}
static inline void fr_to_words(const Fr& x, uint64_t* w) {
    for (int k = 0; k < 4; ++k) w[k] = (uint64_t)x.l[2 * k] | ((uint64_t)x.l[2 * k + 1] << 32);
}

// One witness on the host: `inputs` already range-checked by the caller.  `vals` is the caller's scratch of tape.slots elements.
static inline void tape_run_host(const Tape& t, const uint64_t* inputs, Fr* vals, uint64_t* out) {
    vals[0] = Fr::one();
    for (size_t i = 0; i < t.n_in; ++i) vals[t.in_slot[i]] = Fr::from_canonical(fr_from_words(inputs + 4 * i));
    const Fr* cp = t.consts.data();
    for (const TapeOp& op : t.ops) {
        const Fr a = (op.a & TAPE_CONST) ? cp[op.a & ~TAPE_CONST] : vals[op.a];
        if (op.kind == TAPE_COPY) { vals[op.dst] = a; continue; }
        const Fr b = (op.b & TAPE_CONST) ? cp[op.b & ~TAPE_CONST] : vals[op.b];
        vals[op.dst] = op.kind == TAPE_MUL ? a * b : a + b;
    }
    for (size_t i = 0; i < t.m; ++i) fr_to_words(vals[i].to_canonical(), out + 4 * i);
}

}  // namespace zk

const zk::Tape& zk_circuit_tape(const zk_circuit* c);   // frontend.hip
