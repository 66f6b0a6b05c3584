"""Poseidon over the BN254 scalar field (csrc/poseidon.hpp, csrc/poseidon.hip): x^5, t = arity + 1 for arity 1, 2, 4, R_F = 8,
R_P = 56 / 57 / 60 -- circomlib's parameter sets, generated in code from the Grain LFSR.

    hash(ints), params(arity), zero_hashes(depth)      host code, no context (zk_poseidon_hash, zk_poseidon_params)
    Context.poseidon_hash_batch(...)                   one hash per lane on the GPU (zk_poseidon_hash_batch)
    Context.poseidon_tree(leaves, depth) -> PoseidonTree    a binary Merkle tree that stays on the device; .paths() hands out
                                                       authentication paths in the layout Mixgen.run reads; .update() and
                                                       .append() change it in place (zk_poseidon_tree_update / _append)
    circuit.Builder.poseidon / .merkle_root            the same function as sub-circuits
"""
import ctypes as C

import numpy as np

from . import _lib, ZkError, ints_to_limbs, limbs_to_int, limbs_to_ints

ARITIES = (1, 2, 4)


def hash(inputs):   # noqa: A001 -- the function's name
    """Poseidon of 1, 2 or 4 integers < r -> integer"""
    lib = _lib.load()
    xs = [int(x) for x in inputs]
    if any(x < 0 or x >> 256 for x in xs):
        raise ZkError(_lib.ZK_ERR_RANGE, "poseidon: an input is not below r")
    a = ints_to_limbs(xs) if xs else np.zeros((1, 4), np.uint64)
    out = np.zeros(4, np.uint64)
    rc = lib.zk_poseidon_hash(a.ctypes.data_as(_lib.u64p), len(xs), out.ctypes.data_as(_lib.u64p))
    if rc != 0:
        raise ZkError(rc, "poseidon: the arity must be 1, 2 or 4, got %d" % len(xs) if rc == _lib.ZK_ERR_ARG else "poseidon: an input is not below r")
    return limbs_to_int(out)


def params(arity):
    """dict(t, rf, rp, c: the (rf + rp) * t round constants, m: the t x t matrix M) as integers"""
    lib = _lib.load()
    rf, rp = C.c_uint(), C.c_uint()
    rc = lib.zk_poseidon_params(arity, C.byref(rf), C.byref(rp), None, None)
    if rc != 0:
        raise ZkError(rc, "poseidon: the arity must be 1, 2 or 4, got %d" % arity)
    t = arity + 1
    c = np.zeros(((rf.value + rp.value) * t, 4), np.uint64)
    m = np.zeros((t * t, 4), np.uint64)
    lib.zk_poseidon_params(arity, None, None, c.ctypes.data_as(_lib.u64p), m.ctypes.data_as(_lib.u64p))
    flat = limbs_to_ints(m)
    return dict(t=t, rf=rf.value, rp=rp.value, c=limbs_to_ints(c), m=[flat[i * t:(i + 1) * t] for i in range(t)])


def zero_hashes(depth):
    """[z_0 .. z_depth]: z_0 = 0, z_{k+1} = hash(z_k, z_k), the value of a subtree of height k without a leaf"""
    z = [0]
    for _ in range(depth):
        z.append(hash([z[-1], z[-1]]))
    return z


class PoseidonTree:
    """zk_poseidon_tree: a binary Merkle tree over Poseidon of arity 2, resident on the device.  Level 0 is the leaves, level k holds
    ceil(n_leaves / 2^k) nodes (at least one from level 1 up); a child that does not exist counts as zero_hashes(depth)[k].  The
    context must stay open.  update() rewrites leaves and append() adds leaves behind the last one; both rehash only the nodes above
    the changed leaves and leave the tree as zk_poseidon_tree_build over the new leaf list would make it.  n_leaves follows the
    library (zk_poseidon_tree_dims) after every accepted call; a refused call changes nothing."""

    def __init__(self, ctx, d_leaves_ptr, n_leaves, depth):
        self.ctx, self.lib = ctx, ctx.lib
        p = C.c_void_p()
        ctx._check(self.lib.zk_poseidon_tree_build(ctx.ptr, C.c_void_p(d_leaves_ptr), n_leaves, depth, C.byref(p)))
        self.ptr, self.n_leaves, self.depth = p, n_leaves, depth
        self.field_words, self.bit_bytes = 4 * (depth + 1), (depth + 7) // 8

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_poseidon_tree_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def root(self):
        out = np.zeros(4, np.uint64)
        self.ctx._check(self.lib.zk_poseidon_tree_root(self.ptr, out.ctypes.data_as(_lib.u64p)))
        return limbs_to_int(out)

    def level_size(self, level):
        return self.n_leaves if level == 0 else max(1, (self.n_leaves + (1 << level) - 1) >> level)

    def nodes(self, level):
        """the stored nodes of one level as integers"""
        if level < 0 or level > self.depth:
            raise ZkError(_lib.ZK_ERR_ARG, "poseidon tree: level %d is not in 0..%d" % (level, self.depth))
        out = np.zeros((max(self.level_size(level), 1), 4), np.uint64)
        self.ctx._check(self.lib.zk_poseidon_tree_nodes(self.ptr, level, out.ctypes.data_as(_lib.u64p)))
        return limbs_to_ints(out[:self.level_size(level)])

    def paths_dev(self, d_indices_ptr, count, d_fields_ptr, d_bits_ptr, field_stride_words=None, bits_stride_bytes=None):
        """device to device: d_indices_ptr count uint64; d_fields_ptr rows of (1 + depth) x 4 words -- leaf, siblings -- and
        d_bits_ptr rows of ceil(depth / 8) bytes -- the direction bits -- are Mixgen.run's d_fields_ptr and d_in_ptr for a circuit
        whose inputs were created in the order leaf, siblings, directions"""
        self.ctx._check(self.lib.zk_poseidon_tree_paths(
            self.ptr, C.c_void_p(d_indices_ptr), count, C.c_void_p(d_fields_ptr), self.field_words if field_stride_words is None else field_stride_words,
            C.c_void_p(d_bits_ptr), self.bit_bytes if bits_stride_bytes is None else bits_stride_bytes))

    def paths(self, indices):
        """host indices -> (fields (count, 1 + depth, 4) uint64, bits (count, ceil(depth / 8)) uint8), staged through torch tensors"""
        import torch
        idx = np.ascontiguousarray(np.asarray(list(indices), dtype=np.uint64))
        dev = "cuda:%d" % self.ctx.device
        d_idx = torch.from_numpy(idx.view(np.int64)).to(dev)
        d_fields = torch.zeros((max(idx.size, 1), self.depth + 1, 4), dtype=torch.int64, device=dev)
        d_bits = torch.zeros((max(idx.size, 1), max(self.bit_bytes, 1)), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.paths_dev(d_idx.data_ptr(), idx.size, d_fields.data_ptr(), d_bits.data_ptr(), bits_stride_bytes=max(self.bit_bytes, 1))
        return d_fields.cpu().numpy().view(np.uint64)[:idx.size], d_bits.cpu().numpy()[:idx.size, :self.bit_bytes]

    def _refresh_dims(self):
        n = C.c_size_t()
        self.ctx._check(self.lib.zk_poseidon_tree_dims(self.ptr, C.byref(n), None))
        self.n_leaves = n.value

    def update_dev(self, d_indices_ptr, d_values_ptr, count):
        """device to device: leaf indices[j] = values[j] for count uint64 indices and count x 4 canonical words.  ZkError, and the tree
        as it was: an index >= n_leaves or a value >= r (ZK_ERR_RANGE, naming the lowest instance), an index that occurs twice
        (ZK_ERR_ARG, naming the lowest such leaf)"""
        self.ctx._check(self.lib.zk_poseidon_tree_update(self.ptr, C.c_void_p(d_indices_ptr), C.c_void_p(d_values_ptr), count))
        self._refresh_dims()

    def update(self, indices, values):
        """host indices and values (integers or (count, 4) uint64), staged through torch tensors"""
        import torch
        idx = np.ascontiguousarray(np.asarray(list(indices), dtype=np.uint64))
        dev = "cuda:%d" % self.ctx.device
        d_idx = torch.from_numpy(np.append(idx, np.uint64(0)).view(np.int64)).to(dev)     # never an empty tensor
        d_val = self._stage(values, dev)
        if d_val.shape[0] - 1 != idx.size:
            raise ZkError(_lib.ZK_ERR_ARG, "poseidon tree: %d indices and %d values" % (idx.size, d_val.shape[0] - 1))
        self.update_dev(d_idx.data_ptr(), d_val.data_ptr(), idx.size)

    def append_dev(self, d_leaves_ptr, count):
        """device to device: count x 4 canonical words become leaves n_leaves .. n_leaves + count - 1.  ZkError, and the tree as it
        was: more leaves than 2^depth (ZK_ERR_ARG), a leaf >= r (ZK_ERR_RANGE, naming the lowest position)"""
        self.ctx._check(self.lib.zk_poseidon_tree_append(self.ptr, C.c_void_p(d_leaves_ptr), count))
        self._refresh_dims()

    def append(self, leaves):
        """host leaves (integers or (count, 4) uint64), staged through a torch tensor"""
        d = self._stage(leaves, "cuda:%d" % self.ctx.device)
        self.append_dev(d.data_ptr(), d.shape[0] - 1)

    @staticmethod
    def _stage(values, dev):
        """-> a device tensor of the values' limbs and one row of zeros behind them (never an empty tensor)"""
        import torch
        a = values if isinstance(values, np.ndarray) else ints_to_limbs(list(values))
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        d = torch.from_numpy(np.ascontiguousarray(np.vstack([a, np.zeros((1, 4), np.uint64)])).view(np.int64)).to(dev)
        torch.cuda.synchronize(dev)
        return d
