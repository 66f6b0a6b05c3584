"""Poseidon on the device (csrc/poseidon.hip): zk_poseidon_hash_batch at every lane, wave and workgroup edge, the device Merkle tree
level by level, its authentication paths, and a depth-3 membership circuit fed device to device from the tree's paths through
zk_mixgen_run to proofs that verify against the tree's root.  The reference is tests/poseidon_model.py (Python integers), computed
once per shape and shared."""
import functools

import numpy as np
import pytest
import torch

from zksnark_rs_amd import SplitMix64, ZkError, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuit import Builder, Mixgen, Witgen

import poseidon_model as pm

pytestmark = pytest.mark.gpu

R = pm.R
FILL = 0xA5                                                 # the byte an output buffer holds before a call
BLOCK = 256                                                 # lanes of a workgroup of k_poseidon
COUNTS = (1, 63, 64, 65, 255, 256, 257, 2 * BLOCK + 1)
TREES = [(0, 3), (1, 0), (1, 1), (2, 1), (3, 2), (5, 3), (64, 6), (65, 7), (1000, 10), (1000, 20)]


def to_dev(ctx, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:%d" % ctx.device)


@functools.lru_cache(maxsize=None)
def batch_case(arity):
    """2 * BLOCK + 1 input rows, the first ones made of 0 and r - 1, and their digests by the model"""
    rng = SplitMix64(700 + arity)
    rows = [[0] * arity, [R - 1] * arity, [0] * (arity - 1) + [R - 1], [R - 1] + [0] * (arity - 1), [1] * arity]
    rows += [[rng.fr() for _ in range(arity)] for _ in range(max(COUNTS) - len(rows))]
    return np.stack([ints_to_limbs(r) for r in rows]), [pm.hash(r) for r in rows]


@functools.lru_cache(maxsize=None)
def tree_case(n_leaves, depth):
    rng = SplitMix64(800 + 31 * n_leaves + depth)
    leaves = ([0, R - 1] + [rng.fr() for _ in range(n_leaves)])[2 if n_leaves < 3 else 0:][:n_leaves]
    return leaves, pm.tree_levels(leaves, depth)


# ---- zk_poseidon_hash_batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arity", [1, 2, 4])
def test_hash_batch_at_every_edge(ctx, arity):
    inputs, want = batch_case(arity)
    d_in = to_dev(ctx, inputs)
    for count in COUNTS:
        d_out = torch.empty((count + 3, 4), dtype=torch.int64, device=d_in.device)
        d_out.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        ctx.poseidon_hash_batch(d_in.data_ptr(), arity, count, d_out.data_ptr())
        out = d_out.cpu().numpy().view(np.uint64)
        assert limbs_to_ints(out[:count]) == want[:count], count
        assert (out[count:].view(np.uint8) == FILL).all(), count   # lanes past `count` write nothing
    assert limbs_to_ints(ctx.poseidon_hash_batch(inputs[:5])) == want[:5]      # the host form


def test_hash_batch_refusals(ctx):
    inputs, want = batch_case(2)
    bad = inputs[:100].copy()
    bad[70, 1] = ints_to_limbs([R])[0]
    bad[5, 0] = ints_to_limbs([(1 << 256) - 1])[0]
    with pytest.raises(ZkError) as e:
        ctx.poseidon_hash_batch(bad)
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 5" in str(e.value)
    bad[5] = inputs[5]
    with pytest.raises(ZkError) as e:
        ctx.poseidon_hash_batch(bad)
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 70" in str(e.value)
    assert limbs_to_ints(ctx.poseidon_hash_batch(inputs[:100])) == want[:100]  # and the context goes on working
    d = to_dev(ctx, inputs[:4])
    for arity in (0, 3, 5):
        with pytest.raises(ZkError) as e:
            ctx.poseidon_hash_batch(d.data_ptr(), arity, 1, d.data_ptr())
        assert e.value.status == _lib.ZK_ERR_ARG and "arity" in str(e.value)
    ctx.poseidon_hash_batch(0, 2, 0, 0)                      # count == 0: nothing is touched
    with pytest.raises(ZkError) as e:
        ctx.poseidon_hash_batch(0, 2, 1, d.data_ptr())
    assert e.value.status == _lib.ZK_ERR_ARG


# ---- the tree ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_leaves,depth", TREES)
def test_tree_levels_against_the_model(ctx, n_leaves, depth):
    leaves, levels = tree_case(n_leaves, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    assert tree.root == pm.tree_root(levels, depth)
    if n_leaves == 0:
        assert tree.root == pm.zero_hashes(depth)[depth]
    for k in range(depth + 1):
        assert tree.level_size(k) == len(levels[k]) == pm.level_size(n_leaves, k)
        assert tree.nodes(k) == levels[k], k
    with pytest.raises(ZkError) as e:
        tree.ctx._check(tree.lib.zk_poseidon_tree_nodes(tree.ptr, depth + 1, None))
    assert e.value.status == _lib.ZK_ERR_ARG
    tree.close()


def test_tree_known_roots_and_refusals(ctx):
    for depth, want in ((2, 0x0d9e989a60f1961e8fda683cfc3585608a47d513f9af9167c1287fa8cea0720e),
                        (3, 0x05c1e52b41a571293b30efacd2afdb7173b20cfaf1f646c4ac9f96eb75848270)):
        tree = ctx.poseidon_tree([1, 2, 3], depth)
        assert tree.root == want
        tree.close()
    for leaves, depth, word in (([1, 2, R, 4, R], 3, "leaf 2"), ([R], 0, "leaf 0"), ([5, (1 << 256) - 1], 1, "leaf 1")):
        with pytest.raises(ZkError) as e:
            ctx.poseidon_tree(leaves, depth)
        assert e.value.status == _lib.ZK_ERR_RANGE and word in str(e.value)
    for n_leaves, depth in ((9, 3), (2, 0), (1, 33)):
        with pytest.raises(ZkError) as e:
            ctx.poseidon_tree(list(range(n_leaves)), depth)
        assert e.value.status == _lib.ZK_ERR_ARG
    tree = ctx.poseidon_tree(list(range(8)), 3)             # n_leaves == 2^depth is the full tree
    assert tree.root == pm.tree_root(pm.tree_levels(list(range(8)), 3), 3)
    tree.close()


@pytest.mark.parametrize("n_leaves,depth", [(1, 0), (1, 1), (5, 3), (65, 7), (1000, 10), (1000, 20)])
def test_paths_fold_to_the_root(ctx, n_leaves, depth):
    leaves, levels = tree_case(n_leaves, depth)
    root = pm.tree_root(levels, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    rng = SplitMix64(900 + n_leaves + depth)
    edge = [0, n_leaves - 1]
    for k in range(depth):                                  # the last node of a level of odd size: its sibling is z_k
        if len(levels[k]) % 2:
            edge.append(min(((len(levels[k]) - 1) << k), n_leaves - 1))
    indices = (edge + [rng.next() % n_leaves for _ in range(65)])[:65]
    for count in (1, 64, 65):
        fields, bits = tree.paths(indices[:count])
        assert fields.shape == (count, depth + 1, 4) and bits.shape == (count, (depth + 7) // 8)
        for j in range(count):
            vals = limbs_to_ints(fields[j])
            assert int.from_bytes(bytes(bits[j]), "little") == indices[j], j
            leaf, sibs, dirs = pm.path(levels, depth, indices[j])
            assert (vals[0], vals[1:]) == (leaf, sibs), j
            if count == 65 and j < 12:
                assert pm.fold(vals[0], vals[1:], dirs) == root, j
    # wider strides: the gaps keep what they held
    count, fs, bs = 3, 4 * (depth + 1) + 3, (depth + 7) // 8 + 2
    d_idx = to_dev(ctx, np.array(indices[:count], np.uint64))
    d_f = torch.full((count, fs), -1, dtype=torch.int64, device=d_idx.device)
    d_b = torch.full((count, bs), FILL, dtype=torch.uint8, device=d_idx.device)
    torch.cuda.synchronize()
    tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr(), field_stride_words=fs, bits_stride_bytes=bs)
    wide, wide_bits = d_f.cpu().numpy().view(np.uint64), d_b.cpu().numpy()
    assert np.array_equal(wide[:, :4 * (depth + 1)].reshape(count, depth + 1, 4), tree.paths(indices[:count])[0])
    assert (wide[:, 4 * (depth + 1):] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (wide_bits[:, (depth + 7) // 8:] == FILL).all()
    # refusals
    with pytest.raises(ZkError) as e:
        tree.paths([0] * 70 + [n_leaves] + [0] * 5 + [n_leaves + 1])
    assert e.value.status == _lib.ZK_ERR_RANGE and "instance 70" in str(e.value)
    with pytest.raises(ZkError) as e:
        tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr(), field_stride_words=4 * (depth + 1) - 1, bits_stride_bytes=bs)
    assert e.value.status == _lib.ZK_ERR_ARG
    if depth:
        with pytest.raises(ZkError) as e:
            tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr(), field_stride_words=fs, bits_stride_bytes=(depth + 7) // 8 - 1)
        assert e.value.status == _lib.ZK_ERR_ARG
    tree.close()


# ---- end to end: a membership circuit fed from the tree -----------------------------------------------------------------------
def membership_circuit(depth):
    """public: the root; private: leaf, siblings, directions -- created in the order PoseidonTree.paths writes them"""
    b = Builder()
    leaf = b.new_wire()
    sibs = [b.new_wire() for _ in range(depth)]
    dirs = b.new_bits(depth)
    root = b.merkle_root(leaf, sibs, dirs)
    assert b.dims()[1] == 246 * depth
    return b.finish([root])


@pytest.fixture(scope="module")
def membership(ctx):
    depth = 3
    c = membership_circuit(depth)
    d = c.mixed_dims()
    assert (d["n_bit_inputs"], d["n_field_inputs"], d["core_ops"], c.input, c.n) == (3, 4, 0, 1, 738)
    leaves, levels = tree_case(5, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    qap = c.qap_sparse_unity(ctx)
    rng = SplitMix64(4242)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    yield c, tree, qap, crs, rng
    crs.close()
    qap.close()
    tree.close()


def run_from_paths(ctx, c, tree, mg, indices, edit=None):
    """paths -> Mixgen.run, device to device; `edit(d_fields, d_bits)` may tamper with the paths in between.  -> the device
    witnesses and the host copies of the two path arrays"""
    count = len(indices)
    d_idx = to_dev(ctx, np.array(indices, np.uint64))
    d_f = torch.zeros((count, tree.depth + 1, 4), dtype=torch.int64, device=d_idx.device)
    d_b = torch.zeros((count, tree.bit_bytes), dtype=torch.uint8, device=d_idx.device)
    d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device=d_idx.device)
    d_w.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr())
    if edit:
        edit(d_f, d_b)
        torch.cuda.synchronize()
    mg.run(d_b.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr())
    return d_w, d_f.cpu().numpy().view(np.uint64), d_b.cpu().numpy()


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_paths_feed_mixgen_device_to_device(ctx, membership, count):
    c, tree, qap, crs, rng = membership
    indices = [(3 * j + 1) % 5 for j in range(count)]
    mg = Mixgen(ctx, c)
    d_w, fields, bits = run_from_paths(ctx, c, tree, mg, indices)
    got = d_w.cpu().numpy().view(np.uint64)
    tape_in = np.zeros((count, 7, 4), np.uint64)            # the same inputs as field elements in creation order
    tape_in[:, :4] = fields
    for k in range(3):
        tape_in[:, 4 + k, 0] = (bits[:, 0] >> k) & 1
    wg = Witgen(ctx, c)
    assert np.array_equal(got, wg.run_numpy(tape_in))
    wg.close()
    for j in range(count):
        assert np.array_equal(got[j], c.weights_mixed(bytes(bits[j]), fields[j])), j
    assert limbs_to_ints(got[:, 1]) == [tree.root] * count
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert [int(x) for x in res["bad_gates"]] == [0] * count and (res["first_bad"] == _lib.QAP_CHECK_NONE).all()
    mg.close()


def test_membership_proofs_verify_against_the_tree_root(ctx, membership):
    c, tree, qap, crs, rng = membership
    count = 65
    indices = [j % 5 for j in range(count)]
    mg = Mixgen(ctx, c)
    d_w, _, _ = run_from_paths(ctx, c, tree, mg, indices)
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert not any(int(x) for x in res["bad_gates"])
    ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(count)]
    proofs = []
    for first in range(0, count, 64):                       # a batch holds at most ZK_MAX_BATCH = 64 proofs
        n = min(64, count - first)
        ticket = ctx.prove_batch_submit(crs, qap, ptrs[first:first + n], [c.m] * n, [rng.fr() for _ in range(n)], [rng.fr() for _ in range(n)])
        proofs += ctx.prove_batch_wait(ticket, n)
    public = np.tile(ints_to_limbs([tree.root]).reshape(1, 1, 4), (count, 1, 1))
    assert ctx.verify_batch(crs, public, proofs).all()
    other = ctx.poseidon_tree([7, 8, 9, 10, 11], 3)          # another tree's root: refused by the verdict
    assert other.root != tree.root
    wrong = public.copy()
    wrong[11, 0] = ints_to_limbs([other.root])[0]
    assert [j for j, ok in enumerate(ctx.verify_batch(crs, wrong, proofs)) if not ok] == [11]
    other.close()

    # a wrong sibling and a flipped direction: consistent witnesses of ANOTHER root -- every gate holds, the verdict refuses
    def tamper(d_f, d_b):
        d_f[1, 2, 0] ^= 1                                   # instance 1: the sibling of level 1
        d_b[2, 0] ^= 2                                      # instance 2: the direction of level 1
    d_t, _, _ = run_from_paths(ctx, c, tree, mg, [4, 4, 4], edit=tamper)
    res = ctx.qap_check_dev(qap, d_t.data_ptr(), c.m, 3)
    assert [int(x) for x in res["bad_gates"]] == [0, 0, 0]
    roots = limbs_to_ints(d_t.cpu().numpy().view(np.uint64)[:, 1])
    assert roots[0] == tree.root and roots[1] != tree.root and roots[2] != tree.root
    ticket = ctx.prove_batch_submit(crs, qap, [d_t.data_ptr() + j * c.m * 32 for j in range(3)], [c.m] * 3, [rng.fr() for _ in range(3)],
                                    [rng.fr() for _ in range(3)])
    forged = ctx.prove_batch_wait(ticket, 3)
    assert list(ctx.verify_batch(crs, public[:3], forged)) == [True, False, False]
    # the true root written over the wrong one: now the closing gate of the last hash fails, and qap_check says so
    d_t[1, 1] = d_t[0, 1]
    torch.cuda.synchronize()
    res = ctx.qap_check_dev(qap, d_t.data_ptr(), c.m, 3)
    assert [int(x) > 0 for x in res["bad_gates"]] == [False, True, False] and int(res["first_bad"][1]) == c.n - 1
    mg.close()
