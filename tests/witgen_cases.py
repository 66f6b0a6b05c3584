"""Programs and helpers shared by test_witgen_tape.py (host) and test_gpu_witgen.py (device)."""
import ctypes as C
import os
import re

import numpy as np

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib

ZK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zk")
GOLDEN = ["simple.zk", "lispesque_quad.zk", "lispesque_cubic.zk", "deg_15.zk", "8bit_comparator.zk"]
R = zk.R_MODULUS

# (the tokenizer splits on white space: top-level groups are separated by a blank)
STATIC_ERRORS = [
    ("(in a) (out b) (verify b) (program (= a (* b b)))", "StructureErr(None, Attempted to assign to an already assigned variable)"),
    ("(in a) (out b) (verify b) (program (= b (* c c)))", "StructureErr(None, Under constrained expression)"),
    ("(in a) (out b) (verify b) (program (= b (+ a a)))", "panic: variable order does not cover every wire"),
]
UNUSED_INPUT = "(in a z) (out b) (verify b) (program (= b (* a a)))"                       # inputs 3, 4 -> [1, 9, 3]
NESTED = "(in a) (out b c) (verify b) (program (= c (+ a (* a (+ a 2)))) (= b (* c a)))"    # input 3 -> [1, 54, 18, 3]
BIG_LITERAL = int("9" * 80)                                                               # 80 decimal digits: wraps mod r
DEEP = "(in a) (out b c) (verify b) (program (= c (+ a (* (+ a 1) (+ (* 2 a) (* a (+ a %d)))))) (= b (* c a)))" % BIG_LITERAL


def deep_expected(a):
    c = (a + (a + 1) * (2 * a + a * (a + BIG_LITERAL))) % R
    return [1, c * a % R, c, a % R]                       # order: b (verify), then c, a by first appearance


def golden(name):
    return open(os.path.join(ZK_DIR, name)).read()


def squares_zk(k=200):
    """k independent squares (one level, k wide), then their running sum (k - 1 levels, 1 wide)."""
    lines = ["(in %s)" % " ".join("a%d" % i for i in range(k)), "(out %s)" % " ".join("s%d" % i for i in range(1, k)), "(verify s%d)" % (k - 1),
             "(program"]
    lines += ["(= q%d (* a%d a%d))" % (i, i, i) for i in range(k)]
    lines.append("(= s1 (* 1 (+ q0 q1)))")
    lines += ["(= s%d (* 1 (+ s%d q%d)))" % (i, i - 1, i) for i in range(2, k)]
    return "\n".join(lines) + ")"


def random_inputs(seed, count, n_in):
    """(count, n_in, 4) limbs: instance 0 all zero, instance 1 all r - 1, the rest SplitMix64 field elements."""
    rng = zk.SplitMix64(seed)
    rows = []
    for j in range(count):
        if j == 0:
            rows.append([0] * n_in)
        elif j == 1:
            rows.append([R - 1] * n_in)
        else:
            rows.append([rng.fr() for _ in range(n_in)])
    return np.stack([zk.ints_to_limbs(r) if n_in else np.zeros((0, 4), np.uint64) for r in rows])


def call_weights(c, fn_name, inputs, n_in=None, m=None):
    """(status, text, words) of zk_circuit_weights / zk_circuit_weights_tape called directly."""
    a = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, 4)
    m = c.m if m is None else m
    out = np.zeros((max(m, 1), 4), np.uint64)
    rc = getattr(c.lib, fn_name)(c.ptr, a.ctypes.data_as(_lib.u64p), a.shape[0] if n_in is None else n_in, out.ctypes.data_as(_lib.u64p), m)
    return rc, c.lib.zk_circuit_last_error(c.ptr).decode(), out


def assignment_shape(code):
    """(assignments, depth, width) of a program read from its text, each `=` one node: level = 1 + the highest level among the
    variables its right-hand side reads, `in` variables are level 0."""
    body = code[code.index("(program"):]
    heads = [m.start() for m in re.finditer(r"\(=\s", body)]
    level, per_level = {}, {}
    for i, h in enumerate(heads):
        text = body[h:heads[i + 1] if i + 1 < len(heads) else len(body)]
        names = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", text)
        lv = 1 + max([level.get(v, 0) for v in names[1:]] or [0])
        level[names[0]] = lv
        per_level[lv] = per_level.get(lv, 0) + 1
    return len(heads), max(per_level), max(per_level.values())
