"""The reference's .zk front end behind the C ABI (host code, as in the reference).

    ASTParser::try_parse      circuit/mod.rs:224-527   -> Circuit(code)
    circuit::weights          circuit/mod.rs:529-637   -> Circuit.weights(inputs), Circuit.weights_tape(inputs) (compiled tape),
                                                          Witgen(ctx, circuit).run(...) (the tape for many input sets on the GPU)
    QAP::from(root_rep)       fr.rs:140-173            -> Circuit.qap(ctx)   (Lagrange interpolation on the GPU)
"""
import ctypes as C

import numpy as np

from . import _lib, ZkError, ints_to_limbs, Qap


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
        self.ptr = p
        m, n, l, n_in = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.lib.zk_circuit_dims(p, C.byref(m), C.byref(n), C.byref(l), C.byref(n_in))
        self.m, self.n, self.input, self.n_in = m.value, n.value, l.value, n_in.value

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
