"""The reference's .zk front end behind the C ABI (host code, as in the reference).

    ASTParser::try_parse      circuit/mod.rs:224-527   -> Circuit(code)
    circuit::weights          circuit/mod.rs:529-637   -> Circuit.weights(inputs), Circuit.weights_tape(inputs) (compiled tape),
                                                          Witgen(ctx, circuit).run(...) (the tape for many input sets on the GPU)
    QAP::from(root_rep)       fr.rs:140-173            -> Circuit.qap(ctx)   (Lagrange interpolation on the GPU)

and its gate-level circuit builder (circuit/builder/mod.rs, types.rs; host code as well):

    Circuit<T>, new_word8 .. keccak256, validate_order       -> Builder, whose finish() is an ordinary Circuit
    bit-sliced witnesses of any built circuit                -> Mixgen(ctx, circuit).run(...) / .eval_fields(...) (csrc/mixgen.hip):
                                                                the boolean core bit-sliced, the field tail one instance per lane;
                                                                Circuit.mixed_dims / .weights_mixed are the split and its host model
    bit-sliced witnesses of a boolean built circuit          -> Boolgen(ctx, circuit).run(...) / .eval(...) / .eval_fields(...)
                                                                (csrc/boolgen.hip); Builder.pack makes one field element of up to
                                                                253 bit wires, so a digest is two public inputs instead of 256
"""
import ctypes as C

import numpy as np

from . import _lib, ZkError, ints_to_limbs, Qap, R_MODULUS


class ParseErr(ValueError):
    """ParseErr::SyntaxErr / ParseErr::StructureErr (circuit/ast.rs:290-293)."""


class Circuit:
    def __init__(self, code):
        self.lib = _lib.load()
        p = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self.lib.zk_circuit_parse(code.encode(), C.byref(p), err, len(err))
        if rc != 0:
            raise ParseErr(err.value.decode())
        self._adopt(p)

    @classmethod
    def _from_ptr(cls, p):
        """a zk_circuit handle made elsewhere (Builder.finish)"""
        c = cls.__new__(cls)
        c.lib = _lib.load()
        c._adopt(p)
        return c

    def _adopt(self, p):
        self.ptr = p
        m, n, l, n_in = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.lib.zk_circuit_dims(p, C.byref(m), C.byref(n), C.byref(l), C.byref(n_in))
        self.m, self.n, self.input, self.n_in = m.value, n.value, l.value, n_in.value

    @property
    def boolean(self):
        """True where Boolgen takes the circuit: built, every input a bit wire, every sub-circuit from a boolean constructor or a
        pack over bit-valued wires whose output nothing reads."""
        return bool(self.lib.zk_circuit_is_boolean(self.ptr))

    @property
    def packed_wires(self):
        """the number of packed wires (Builder.pack calls); 0 for parsed circuits"""
        out = C.c_size_t()
        self.lib.zk_circuit_packed_wires(self.ptr, C.byref(out))
        return out.value

    def wire_index(self, wire):
        """witness index of a Builder wire id (built circuits only; the constant-zero wire has none)"""
        out = C.c_size_t()
        if self.lib.zk_circuit_wire_index(self.ptr, wire, C.byref(out)) != 0:
            raise ValueError("wire %d has no witness index in this circuit" % wire)
        return out.value

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_circuit_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self, which):
        """DummyRep rows of u (0), v (1) or w (2): (ptr[m+1], gate[nnz] 0-based, val[nnz,4])."""
        nnz = C.c_size_t()
        self.lib.zk_circuit_rows(self.ptr, which, None, None, None, C.byref(nnz))
        ptr = np.zeros(self.m + 1, np.uint64)
        gate = np.zeros(max(nnz.value, 1), np.uint32)
        val = np.zeros((max(nnz.value, 1), 4), np.uint64)
        self.lib.zk_circuit_rows(self.ptr, which, ptr.ctypes.data_as(_lib.u64p), gate.ctypes.data_as(_lib.u32p),
                                 val.ctypes.data_as(_lib.u64p), C.byref(nnz))
        return ptr, gate[:nnz.value], val[:nnz.value]

    def weights(self, inputs):
        """inputs: ints or (n_in, 4) limbs in `in` order -> (m, 4) witness, [1] first."""
        a = ints_to_limbs(list(inputs)) if not isinstance(inputs, np.ndarray) else np.ascontiguousarray(inputs, dtype=np.uint64)
        out = np.zeros((self.m, 4), np.uint64)
        rc = self.lib.zk_circuit_weights(self.ptr, a.ctypes.data_as(_lib.u64p), a.shape[0], out.ctypes.data_as(_lib.u64p), self.m)
        if rc != 0:
            raise ParseErr(self.lib.zk_circuit_last_error(self.ptr).decode())
        return out

    def weights_tape(self, inputs):
        """weights() through the tape compiled at parse time: same words, same errors, no parsing or name lookup per call."""
        a = ints_to_limbs(list(inputs)) if not isinstance(inputs, np.ndarray) else np.ascontiguousarray(inputs, dtype=np.uint64)
        out = np.zeros((self.m, 4), np.uint64)
        rc = self.lib.zk_circuit_weights_tape(self.ptr, a.ctypes.data_as(_lib.u64p), a.shape[0], out.ctypes.data_as(_lib.u64p), self.m)
        if rc != 0:
            raise ParseErr(self.lib.zk_circuit_last_error(self.ptr).decode())
        return out

    def tape_dims(self):
        """dict(ops, slots, consts: what the tape holds; depth, width: the program's shape with each `=` as one node)."""
        v = [C.c_size_t() for _ in range(5)]
        rc = self.lib.zk_circuit_tape_dims(self.ptr, *[C.byref(x) for x in v])
        if rc != 0:
            raise ParseErr(self.lib.zk_circuit_last_error(self.ptr).decode())
        return dict(zip(("ops", "slots", "consts", "depth", "width"), (x.value for x in v)))

    def mixed_dims(self):
        """the split of a built circuit into a boolean core and a field tail (zk_circuit_mixed_dims): dict(n_bit_inputs,
        n_field_inputs, core_ops, core_levels, tail_ops, tail_levels, tail_slots)"""
        v = [C.c_size_t() for _ in range(7)]
        rc = self.lib.zk_circuit_mixed_dims(self.ptr, *[C.byref(x) for x in v])
        if rc != 0:
            raise ParseErr(self.lib.zk_circuit_last_error(self.ptr).decode())
        return dict(zip(("n_bit_inputs", "n_field_inputs", "core_ops", "core_levels", "tail_ops", "tail_levels", "tail_slots"), (x.value for x in v)))

    def weights_mixed(self, in_bits, in_fields=()):
        """weights() through the split, the host model of Mixgen.run: in_bits the bit inputs packed (bytes or uint8 array, bit k % 8 of
        byte k / 8 = the k-th bit input), in_fields the field inputs in input order (ints or (n, 4) limbs) -> (m, 4) witness"""
        bits = np.ascontiguousarray(np.frombuffer(bytes(in_bits), np.uint8) if not isinstance(in_bits, np.ndarray) else in_bits, dtype=np.uint8)
        if isinstance(in_fields, np.ndarray):
            f = np.ascontiguousarray(in_fields, dtype=np.uint64).reshape(-1, 4)
        else:
            f = ints_to_limbs(list(in_fields)) if len(in_fields) else np.zeros((0, 4), np.uint64)
        out = np.zeros((self.m, 4), np.uint64)
        rc = self.lib.zk_circuit_weights_mixed(self.ptr, bits.ctypes.data_as(C.c_void_p), bits.size, f.ctypes.data_as(_lib.u64p), f.shape[0],
                                               out.ctypes.data_as(_lib.u64p), self.m)
        if rc != 0:
            raise ParseErr(self.lib.zk_circuit_last_error(self.ptr).decode())
        return out

    def qap(self, ctx):
        p = C.c_void_p()
        ctx._check(self.lib.zk_circuit_qap(ctx.ptr, self.ptr, C.byref(p)))
        q = Qap(ctx, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense = self.n, self.m, self.input, True
        return q

    def qap_sparse(self, ctx):
        """The same QAP kept as rows over the integer roots 1..n (no interpolation, any size)."""
        p = C.c_void_p()
        ctx._check(self.lib.zk_circuit_qap_sparse(ctx.ptr, self.ptr, C.byref(p)))
        q = Qap(ctx, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense, q.roots = self.n, self.m, self.input, False, "integers"
        return q

    def qap_sparse_unity(self, ctx):
        """The same rows over the roots of unity: gate k at w^k, n padded to a power of two by empty gates (zk_qap_upload_sparse)."""
        p = C.c_void_p()
        ctx._check(self.lib.zk_circuit_qap_sparse_unity(ctx.ptr, self.ptr, C.byref(p)))
        q = Qap(ctx, p, self.lib.zk_qap_free)
        n = 1
        while n < self.n:
            n *= 2
        q.n, q.m, q.input, q.dense, q.roots = n, self.m, self.input, False, "unity"
        return q


class BuildErr(ValueError):
    """a refusal of the circuit builder (status and text of zk_builder_last_error)"""

    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


class Builder:
    """Circuit<T> of circuit/builder/mod.rs behind zk_builder_*.  A wire is its id (int): ZERO = 0 and ONE = 1 are the constants
    (mod.rs:91-114).  A Word8 is a list of 8 wires, a Word64 a list of 64, least significant bit first (types.rs:135-150: little
    endian).  Gate arguments of fan_in / bitwise_op are the bound method (b.new_xor), as the reference passes Circuit::new_xor, or the
    kind's name ("xor").  finish() gives an ordinary Circuit; see include/zkgpu.h for what differs from the reference."""
    ZERO, ONE = 0, 1
    GATES = {"bit_checker": 0, "not": 1, "and": 2, "or": 3, "xor": 4, "nand": 5, "nor": 6, "xnor": 7, "less_than": 8, "greater_than": 9}
    CMPS = {"is_equal": 0, "is_equal_zero": 1, "less_than": 2, "less_than_eq": 3, "greater_than": 4, "greater_than_eq": 5}

    def __init__(self):
        self.lib = _lib.load()
        p = C.c_void_p()
        if self.lib.zk_builder_create(C.byref(p)) != 0:
            raise MemoryError("zk_builder_create")
        self.ptr = p

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_builder_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise BuildErr(rc, self.lib.zk_builder_last_error(self.ptr).decode())

    @staticmethod
    def _wires(ws):
        a = np.ascontiguousarray(np.asarray(list(ws), dtype=np.int64).reshape(-1))
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: wire id out of range")
        a = a.astype(np.uint32)
        return a, a.ctypes.data_as(_lib.u32p)

    def _kind(self, gate):
        name = gate if isinstance(gate, str) else getattr(gate, "__name__", "")
        name = name[4:] if name.startswith("new_") else name
        if name not in self.GATES:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: unknown gate %r" % (gate,))
        return self.GATES[name]

    def dims(self):
        """(wires handed out so far, the two constants included; sub-circuits = gates so far)"""
        w, g = C.c_size_t(), C.c_size_t()
        self._check(self.lib.zk_builder_dims(self.ptr, C.byref(w), C.byref(g)))
        return w.value, g.value

    # ---- wires ----
    def _new(self, kind, count):
        out = np.zeros(max(count, 1), np.uint32)
        self._check(self.lib.zk_builder_new_wires(self.ptr, kind, count, out.ctypes.data_as(_lib.u32p)))
        return [int(x) for x in out[:count]]

    def new_wire(self):
        """an input that is any field element (mod.rs:120-125); the circuit is then not boolean"""
        return self._new(1, 1)[0]

    def new_bit(self):
        return self._new(0, 1)[0]

    def new_bits(self, count):
        return self._new(0, count)

    def new_word8(self):
        return self._new(0, 8)

    def new_word64(self):
        return self._new(0, 64)

    def new_word8_vec(self, size):
        return [self.new_word8() for _ in range(size)]

    def const_word8(self, value):
        return [(value >> i) & 1 for i in range(8)]

    def const_word64(self, value):
        return [(value >> i) & 1 for i in range(64)]

    # ---- sub-circuits and gates ----
    def new_sub_circuit(self, left, right):
        """left, right: lists of (weight, wire); -> the output wire of (sum left) * (sum right)"""
        lw, lwp = _limbs([w % R_MODULUS for w, _ in left])
        rw, rwp = _limbs([w % R_MODULUS for w, _ in right])
        li, lip = self._wires([x for _, x in left])
        ri, rip = self._wires([x for _, x in right])
        out = C.c_uint32()
        self._check(self.lib.zk_builder_sub_circuit(self.ptr, lwp, lip, len(left), rwp, rip, len(right), C.byref(out)))
        return out.value

    def _gate(self, kind, x, y=0):
        out = C.c_uint32()
        self._check(self.lib.zk_builder_gate(self.ptr, kind, x, y, C.byref(out)))
        return out.value

    def new_bit_checker(self, x):
        return self._gate(0, x)

    def new_not(self, x):
        return self._gate(1, x)

    def new_and(self, x, y):
        return self._gate(2, x, y)

    def new_or(self, x, y):
        return self._gate(3, x, y)

    def new_xor(self, x, y):
        return self._gate(4, x, y)

    def new_nand(self, x, y):
        return self._gate(5, x, y)

    def new_nor(self, x, y):
        return self._gate(6, x, y)

    def new_xnor(self, x, y):
        return self._gate(7, x, y)

    def new_less_than(self, x, y):
        return self._gate(8, x, y)

    def new_greater_than(self, x, y):
        return self._gate(9, x, y)

    def assert_bit(self, wire):
        """the gate w (w - 1) = 0 without output wire: what forces an input to be 0 or 1 (not in the reference)"""
        self._check(self.lib.zk_builder_assert_bit(self.ptr, wire))

    def pack(self, bits):
        """-> the packed wire sum 2^i bits[i] of 1..253 wires, least significant first: one sub-circuit, a field element"""
        a, ap = self._wires(bits)
        out = C.c_uint32()
        self._check(self.lib.zk_builder_pack(self.ptr, ap, a.size, C.byref(out)))
        return out.value

    def poseidon(self, wires):
        """-> the wire Poseidon(wires) of 1, 2 or 4 wires (zksnark_rs_amd.poseidon.hash on their values): 217 / 244 / 301 general
        sub-circuits over linear forms; the output is a field element"""
        a, ap = self._wires(wires)
        out = C.c_uint32()
        self._check(self.lib.zk_builder_poseidon(self.ptr, ap, a.size, C.byref(out)))
        return out.value

    def merkle_root(self, leaf, siblings, dirs):
        """-> the root wire of the Merkle path leaf, siblings[k], dirs[k] (1: the path's node is the right child at level k) over
        Poseidon of arity 2: 246 gates a level, each direction asserted to be a bit.  Inputs created in the order leaf, siblings,
        dirs (dirs as bit wires) read PoseidonTree.paths' two outputs as Mixgen.run's field and bit inputs."""
        s, sp = self._wires(siblings)
        d, dp = self._wires(dirs)
        if s.size != d.size:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: merkle_root takes one direction per sibling")
        out = C.c_uint32()
        self._check(self.lib.zk_builder_merkle_root(self.ptr, leaf, sp, dp, s.size, C.byref(out)))
        return out.value

    # Baby Jubjub (zksnark_rs_amd.babyjub): a point is a list of three wires [X, Y, Z], projective; an affine point is [x, y, ONE]
    def _point(self, p, n):
        a, ap = self._wires(p)
        if a.size != n:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: expected %d wires, got %d" % (n, a.size))
        return a, ap

    def babyjub_assert_on_curve(self, xy):
        """a x^2 + y^2 = 1 + d x^2 y^2 on the wires (x, y): 4 gates, the last one an assertion without output"""
        _, ap = self._point(xy, 2)
        self._check(self.lib.zk_builder_babyjub_assert_on_curve(self.ptr, ap))

    def babyjub_add(self, p, q):
        """-> [X, Y, Z] of p + q: 11 gates, 10 when q[2] is ONE; right for all pairs of curve points; the operands are not asserted"""
        _, pp = self._point(p, 3)
        _, qp = self._point(q, 3)
        out = np.zeros(3, np.uint32)
        self._check(self.lib.zk_builder_babyjub_add(self.ptr, pp, qp, out.ctypes.data_as(_lib.u32p)))
        return [int(x) for x in out]

    def babyjub_mul_fixed(self, bits):
        """-> [X, Y, Z] of [sum 2^i bits[i]] Base8 for 1..256 bit wires, each asserted to be a bit: 1414 gates for 251 bits"""
        a, ap = self._wires(bits)
        out = np.zeros(3, np.uint32)
        self._check(self.lib.zk_builder_babyjub_mul_fixed(self.ptr, ap, a.size, out.ctypes.data_as(_lib.u32p)))
        return [int(x) for x in out]

    def babyjub_mul(self, p_xy, bits):
        """-> [X, Y, Z] of [sum 2^i bits[i]] P for the affine wires p_xy, asserted on the curve, for 1..256 bit wires, each asserted
        to be a bit: 4 + n_bits + 2 + 19 (n_bits - 1) gates"""
        _, pp = self._point(p_xy, 2)
        a, ap = self._wires(bits)
        out = np.zeros(3, np.uint32)
        self._check(self.lib.zk_builder_babyjub_mul(self.ptr, pp, ap, a.size, out.ctypes.data_as(_lib.u32p)))
        return [int(x) for x in out]

    def babyjub_affine(self, p, xy):
        """pins the existing wires xy as the affine form of the point p: x Z = X and y Z = Y, 4 gates"""
        _, pp = self._point(p, 3)
        _, ap = self._point(xy, 2)
        self._check(self.lib.zk_builder_babyjub_affine(self.ptr, pp, ap))

    def eddsa_verify(self, a_xy, r8_xy, msg, s_bits, hm_bits):
        """the statement [S] Base8 = R8 + [8] ([hm] A), hm = H6(R8, A, M) (zksnark_rs_amd.eddsa): the affine wires of A and R8, the
        message wire, the 251 bit wires of S and the 254 bit wires of hm, which the caller supplies (Context.eddsa_verify_batch
        writes them).  Asserts everything a verifier checks, S < l and hm < r included: 73384 gates, the two comparators 66536 of
        them, boolean-class."""
        _, ap = self._point(a_xy, 2)
        _, rp = self._point(r8_xy, 2)
        _, sp = self._point(s_bits, 251)
        _, hp = self._point(hm_bits, 254)
        self._check(self.lib.zk_builder_eddsa_verify(self.ptr, ap, rp, int(msg), sp, hp))

    def pack_bytes(self, wires, bytes_per_element=16):
        """Word8s (or their wires, flat) -> a list of packed wires, bytes_per_element (at most 31) bytes each, little-endian per
        element: a 32-byte digest is [int.from_bytes(d[:16], "little"), int.from_bytes(d[16:], "little")]"""
        flat = self._flat(wires)
        if bytes_per_element < 1 or len(flat) % 8:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: pack_bytes takes whole bytes of 8 wires and at least one byte per element")
        step = 8 * bytes_per_element
        return [self.pack(flat[i:i + step]) for i in range(0, len(flat), step)]

    def fan_in(self, wires, gate):
        a, ap = self._wires(wires)
        out = C.c_uint32()
        self._check(self.lib.zk_builder_fan_in(self.ptr, self._kind(gate), ap, a.size, C.byref(out)))
        return out.value

    def bitwise_op(self, left, right, gate):
        kind = self._kind(gate)
        l, lp = self._wires(left)
        r, rp = self._wires(right if right is not None else [])
        if right is not None and l.size != r.size:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: bitwise_op over arrays of different lengths")
        out = np.zeros(max(l.size, 1), np.uint32)
        self._check(self.lib.zk_builder_bitwise(self.ptr, kind, lp, rp if right is not None else None, l.size, out.ctypes.data_as(_lib.u32p)))
        return [int(x) for x in out[:l.size]]

    def _sized(self, bits, *words):
        for w in words:
            if len(w) != bits:
                raise BuildErr(_lib.ZK_ERR_ARG, "builder: expected a word of %d wires" % bits)

    def u8_bitwise_op(self, left, right, gate):
        self._sized(8, left, right)
        return self.bitwise_op(left, right, gate)

    def u64_bitwise_op(self, left, right, gate):
        self._sized(64, left, right)
        return self.bitwise_op(left, right, gate)

    def u8_unary_op(self, word, gate):
        self._sized(8, word)
        return self.bitwise_op(word, None, gate)

    def u64_unary_op(self, word, gate):
        self._sized(64, word)
        return self.bitwise_op(word, None, gate)

    # ---- comparators (mod.rs:995-1241) ----
    def _cmp(self, kind, left, right):
        l, lp = self._wires(left)
        r, rp = self._wires(right if right is not None else [])
        if right is not None and l.size != r.size:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: comparator over arrays of different lengths")
        out = C.c_uint32()
        self._check(self.lib.zk_builder_compare(self.ptr, kind, lp, rp if right is not None else None, l.size, C.byref(out)))
        return out.value

    def is_equal(self, left, right):
        return self._cmp(0, left, right)

    def is_equal_zero(self, word):
        return self._cmp(1, word, None)

    def less_than(self, left, right):
        return self._cmp(2, left, right)

    def less_than_eq(self, left, right):
        return self._cmp(3, left, right)

    def greater_than(self, left, right):
        return self._cmp(4, left, right)

    def greater_than_eq(self, left, right):
        return self._cmp(5, left, right)

    # ---- Keccak (mod.rs:1247-1457) ----
    @staticmethod
    def _flat(words):
        out = []
        for w in words:
            out.extend(w) if isinstance(w, (list, tuple, np.ndarray)) else out.append(w)
        return out

    def keccak(self, message, rate=136, delim=0x01, rounds=24, out_bytes=32):
        """message: Word8s (or their wires, flat) -> out_bytes Word8s of the sponge (rate bytes, delim, rounds of Keccak-f[1600])"""
        a, ap = self._wires(self._flat(message))
        if a.size % 8:
            raise BuildErr(_lib.ZK_ERR_ARG, "builder: a message is whole bytes of 8 wires")
        out = np.zeros(max(8 * out_bytes, 1), np.uint32)
        self._check(self.lib.zk_builder_keccak(self.ptr, ap, a.size // 8, rate, delim, rounds, out.ctypes.data_as(_lib.u32p), out_bytes))
        return [[int(x) for x in out[8 * k:8 * k + 8]] for k in range(out_bytes)]

    def keccak256(self, message):
        return self.keccak(message, 136, 0x01, 24, 32)

    def keccak256_stream(self, message):
        """the reference absorbs a stream byte by byte; the sub-circuits and their order are those of keccak256"""
        return self.keccak(list(message), 136, 0x01, 24, 32)

    def sha3_256(self, message):
        return self.keccak(message, 136, 0x06, 24, 32)

    def validate_order(self, input_x, pub_range, input_y, pub_c):
        """ValidateOrder (mod.rs:1459-1476) over four Word64s and a (low, high) pair of Word64s"""
        x_geq = self.greater_than_eq(input_x, pub_range[0])
        x_leq = self.less_than_eq(input_x, pub_range[1])
        in_range = self.new_and(x_geq, x_leq)
        y_geq = self.greater_than_eq(input_y, pub_c)
        hash_x_y = self.keccak256_stream(list(input_x) + list(input_y))
        return {"is_x_within_range": in_range, "is_y_greater_than_c": y_geq, "hash_x_y": hash_x_y}

    def finish(self, verify=()):
        """-> Circuit with witness order [1], the verify wires as given, the other inputs in creation order, the other wires by id"""
        v, vp = self._wires(self._flat(verify))
        p = C.c_void_p()
        self._check(self.lib.zk_builder_finish(self.ptr, vp, v.size, C.byref(p)))
        return Circuit._from_ptr(p)


def _limbs(values):
    a = ints_to_limbs(list(values)) if len(values) else np.zeros((0, 4), np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(_lib.u64p)


class Boolgen:
    """zk_boolgen_*: the witnesses of a boolean built circuit for many input sets at once, bit-sliced (csrc/boolgen.hip).  Inputs are
    packed: input i of instance j is bit i % 8 of byte i / 8 of the instance's row.  scratch_kib / group_words / expand_form: the
    options "boolgen_scratch_kib", "boolgen_group_words" and "boolgen_expand_form" for this generator (None = the context's)."""

    def __init__(self, ctx, circuit, scratch_kib=None, group_words=None, expand_form=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.n_in, self.m = circuit.n_in, circuit.m
        self.in_bytes = (self.n_in + 7) // 8
        p = C.c_void_p()
        keep = {}
        for key, val in (("boolgen_scratch_kib", scratch_kib), ("boolgen_group_words", group_words), ("boolgen_expand_form", expand_form)):
            if val is not None:
                keep[key] = ctx.get_option(key)
                ctx.set_option(key, val)
        try:
            rc = self.lib.zk_boolgen_create(ctx.ptr, circuit.ptr, C.byref(p))
        finally:
            for key, val in keep.items():
                ctx.set_option(key, val)
        ctx._check(rc)
        self.ptr = p

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_boolgen_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, d_in_ptr, count, d_out_ptr, in_stride=None, m=None):
        """d_in_ptr: count rows of in_stride bytes (default ceil(n_in / 8)); d_out_ptr: count x m x 4 words, as Witgen.run writes"""
        self.ctx._check(self.lib.zk_boolgen_run(self.ptr, C.c_void_p(d_in_ptr), self.in_bytes if in_stride is None else in_stride, count,
                                                C.c_void_p(d_out_ptr), self.m if m is None else m))

    def eval(self, d_in_ptr, count, wires, d_out_ptr, in_stride=None, out_stride=None):
        """the witness indices `wires` only, packed into count rows of out_stride bytes (default ceil(len(wires) / 8))"""
        w = np.ascontiguousarray(np.asarray(list(wires), dtype=np.uint32))
        self.ctx._check(self.lib.zk_boolgen_eval(self.ptr, C.c_void_p(d_in_ptr), self.in_bytes if in_stride is None else in_stride, count,
                                                 w.ctypes.data_as(_lib.u32p), w.size, C.c_void_p(d_out_ptr),
                                                 (w.size + 7) // 8 if out_stride is None else out_stride))

    def eval_fields(self, d_in_ptr, count, wires, d_out_ptr, in_stride=None):
        """the witness indices `wires`, bit and packed wires alike, as field elements: count x len(wires) x 4 canonical words -- with
        wires = 1..l the `inputs` of Context.verify_batch"""
        w = np.ascontiguousarray(np.asarray(list(wires), dtype=np.uint32))
        self.ctx._check(self.lib.zk_boolgen_eval_fields(self.ptr, C.c_void_p(d_in_ptr), self.in_bytes if in_stride is None else in_stride, count,
                                                        w.ctypes.data_as(_lib.u32p), w.size, C.c_void_p(d_out_ptr)))

    def _stage(self, in_bits):
        import torch
        a = np.ascontiguousarray(in_bits, dtype=np.uint8)
        a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, max(self.in_bytes, 1))
        dev = "cuda:%d" % self.ctx.device
        return torch, dev, a, torch.from_numpy(a).to(dev)

    def run_numpy(self, in_bits):
        """in_bits (count, stride) uint8 -> (count, m, 4) uint64, staged through torch tensors on the context's device"""
        torch, dev, a, d_in = self._stage(in_bits)
        d_out = torch.empty((a.shape[0], self.m, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.run(d_in.data_ptr(), a.shape[0], d_out.data_ptr(), in_stride=a.shape[1])
        return d_out.cpu().numpy().view(np.uint64)

    def eval_numpy(self, in_bits, wires):
        """in_bits (count, stride) uint8 -> (count, ceil(len(wires) / 8)) uint8"""
        torch, dev, a, d_in = self._stage(in_bits)
        wires = list(wires)
        d_out = torch.zeros((a.shape[0], max((len(wires) + 7) // 8, 1)), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.eval(d_in.data_ptr(), a.shape[0], wires, d_out.data_ptr(), in_stride=a.shape[1], out_stride=d_out.shape[1])
        return d_out.cpu().numpy()

    def eval_fields_numpy(self, in_bits, wires):
        """in_bits (count, stride) uint8 -> (count, len(wires), 4) uint64"""
        torch, dev, a, d_in = self._stage(in_bits)
        wires = list(wires)
        d_out = torch.zeros((a.shape[0], len(wires), 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.eval_fields(d_in.data_ptr(), a.shape[0], wires, d_out.data_ptr(), in_stride=a.shape[1])
        return d_out.cpu().numpy().view(np.uint64)


class Mixgen:
    """zk_mixgen_*: the witnesses of any built circuit for many input sets at once: the boolean core bit-sliced as Boolgen runs it, the
    field tail as a small field tape with one instance per lane (csrc/mixgen.hip).  Bit inputs are packed as for Boolgen (bit k = the
    k-th bit input in input order), field inputs are 4 canonical words each, n_field per instance.  scratch_kib / group_words /
    expand_form: the options "boolgen_scratch_kib" (here the cap of state plus tail scratch), "boolgen_group_words" and
    "boolgen_expand_form" for this generator (None = the context's)."""

    def __init__(self, ctx, circuit, scratch_kib=None, group_words=None, expand_form=None):
        self.ctx, self.lib = ctx, ctx.lib
        dims = circuit.mixed_dims()
        self.n_bit, self.n_field, self.m = dims["n_bit_inputs"], dims["n_field_inputs"], circuit.m
        self.in_bytes = (self.n_bit + 7) // 8
        p = C.c_void_p()
        keep = {}
        for key, val in (("boolgen_scratch_kib", scratch_kib), ("boolgen_group_words", group_words), ("boolgen_expand_form", expand_form)):
            if val is not None:
                keep[key] = ctx.get_option(key)
                ctx.set_option(key, val)
        try:
            rc = self.lib.zk_mixgen_create(ctx.ptr, circuit.ptr, C.byref(p))
        finally:
            for key, val in keep.items():
                ctx.set_option(key, val)
        ctx._check(rc)
        self.ptr = p

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_mixgen_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, d_in_ptr, d_fields_ptr, count, d_out_ptr, in_stride=None, m=None):
        """d_in_ptr: count rows of in_stride bytes (default ceil(n_bit / 8)); d_fields_ptr: count x n_field x 4 words (None or 0 where
        the circuit has no field input); d_out_ptr: count x m x 4 words, as Witgen.run writes"""
        self.ctx._check(self.lib.zk_mixgen_run(self.ptr, C.c_void_p(d_in_ptr), self.in_bytes if in_stride is None else in_stride,
                                               C.c_void_p(d_fields_ptr), count, C.c_void_p(d_out_ptr), self.m if m is None else m))

    def run_checked(self, qap, d_in_ptr, d_fields_ptr, count, d_out_ptr, in_stride=None):
        """run(), then zk_qap_check_dev on the witnesses where they lie, as Witgen.run_checked"""
        self.run(d_in_ptr, d_fields_ptr, count, d_out_ptr, in_stride=in_stride)
        return self.ctx.qap_check_dev(qap, d_out_ptr, self.m, count)

    def eval_fields(self, d_in_ptr, d_fields_ptr, count, wires, d_out_ptr, in_stride=None):
        """the witness indices `wires` of either class as field elements: count x len(wires) x 4 canonical words -- with wires = 1..l
        the `inputs` of Context.verify_batch.  Nothing is expanded."""
        w = np.ascontiguousarray(np.asarray(list(wires), dtype=np.uint32))
        self.ctx._check(self.lib.zk_mixgen_eval_fields(self.ptr, C.c_void_p(d_in_ptr), self.in_bytes if in_stride is None else in_stride,
                                                       C.c_void_p(d_fields_ptr), count, w.ctypes.data_as(_lib.u32p), w.size, C.c_void_p(d_out_ptr)))

    def _stage(self, in_bits, in_fields):
        import torch
        a = np.ascontiguousarray(in_bits, dtype=np.uint8)
        a = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, max(self.in_bytes, 1))
        dev = "cuda:%d" % self.ctx.device
        d_f = None
        if self.n_field:
            f = np.ascontiguousarray(in_fields, dtype=np.uint64).reshape(a.shape[0], self.n_field, 4)
            d_f = torch.from_numpy(f.view(np.int64)).to(dev)
        return torch, dev, a, torch.from_numpy(a).to(dev), d_f

    def run_numpy(self, in_bits, in_fields=(), fill=None):
        """in_bits (count, stride) uint8, in_fields (count, n_field, 4) uint64 -> (count, m, 4) uint64, staged through torch tensors on
        the context's device; fill: a byte the output buffer holds before the call"""
        torch, dev, a, d_in, d_f = self._stage(in_bits, in_fields)
        d_out = torch.empty((a.shape[0], self.m, 4), dtype=torch.int64, device=dev)
        if fill is not None:
            d_out.view(torch.uint8).fill_(fill)
        torch.cuda.synchronize(dev)
        self.run(d_in.data_ptr(), d_f.data_ptr() if d_f is not None else None, a.shape[0], d_out.data_ptr(), in_stride=a.shape[1])
        return d_out.cpu().numpy().view(np.uint64)

    def eval_fields_numpy(self, in_bits, in_fields, wires):
        """-> (count, len(wires), 4) uint64"""
        torch, dev, a, d_in, d_f = self._stage(in_bits, in_fields)
        wires = list(wires)
        d_out = torch.zeros((a.shape[0], len(wires), 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.eval_fields(d_in.data_ptr(), d_f.data_ptr() if d_f is not None else None, a.shape[0], wires, d_out.data_ptr(), in_stride=a.shape[1])
        return d_out.cpu().numpy().view(np.uint64)


class Witgen:
    """zk_witgen_*: circuit::weights for many input sets at once on the GPU (csrc/witgen.hip).  The circuit may be closed afterwards;
    the context must stay open.  scratch_kib: cap of the device memory held for slot values (None = the context's option
    "witgen_scratch_kib", 8 GiB by default); the instances run in chunks under it."""

    def __init__(self, ctx, circuit, scratch_kib=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.n_in, self.m = circuit.n_in, circuit.m
        p = C.c_void_p()
        if scratch_kib is None:
            rc = self.lib.zk_witgen_create(ctx.ptr, circuit.ptr, C.byref(p))
        else:
            keep = ctx.get_option("witgen_scratch_kib")
            ctx.set_option("witgen_scratch_kib", scratch_kib)
            try:
                rc = self.lib.zk_witgen_create(ctx.ptr, circuit.ptr, C.byref(p))
            finally:
                ctx.set_option("witgen_scratch_kib", keep)
        ctx._check(rc)
        self.ptr = p

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_witgen_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, d_inputs_ptr, count, d_out_ptr, n_in=None, m=None):
        """d_inputs_ptr: count x n_in x 4 words in HBM; d_out_ptr: count x m x 4 words, witness j at d_out_ptr + j * m * 32 bytes."""
        self.ctx._check(self.lib.zk_witgen_run(self.ptr, C.c_void_p(d_inputs_ptr), self.n_in if n_in is None else n_in, count,
                                               C.c_void_p(d_out_ptr), self.m if m is None else m))

    def run_checked(self, qap, d_inputs_ptr, count, d_out_ptr):
        """run(), then zk_qap_check_dev on the witnesses where they lie: the structured result array of Context.qap_check_dev, one
        entry per instance.  The witnesses never visit the host.  qap: a sparse QAP of this circuit (Circuit.qap_sparse)."""
        self.run(d_inputs_ptr, count, d_out_ptr)
        return self.ctx.qap_check_dev(qap, d_out_ptr, self.m, count)

    def run_numpy(self, inputs):
        """inputs (count, n_in, 4) uint64 -> (count, m, 4) uint64, staged through torch tensors on the context's device."""
        import torch
        a = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, self.n_in, 4)
        count = a.shape[0]
        dev = "cuda:%d" % self.ctx.device
        d_in = torch.from_numpy(a.view(np.int64)).to(dev)
        d_out = torch.empty((count, self.m, 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self.run(d_in.data_ptr(), count, d_out.data_ptr())
        return d_out.cpu().numpy().view(np.uint64)


def qap_download_dense(ctx, qap):
    u = np.zeros((qap.m, qap.n, 4), np.uint64)
    v = np.zeros_like(u)
    w = np.zeros_like(u)
    t = np.zeros((qap.n + 1, 4), np.uint64)
    ctx._check(ctx.lib.zk_qap_download_dense(ctx.ptr, qap.ptr, u.ctypes.data_as(_lib.u64p), v.ctypes.data_as(_lib.u64p),
                                             w.ctypes.data_as(_lib.u64p), t.ctypes.data_as(_lib.u64p)))
    return u, v, w, t
