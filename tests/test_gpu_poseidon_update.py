"""zk_poseidon_tree_update and zk_poseidon_tree_append (csrc/poseidon.hip): after every call the root, every level and the paths are
what zk_poseidon_tree_build over the new leaf list gives, word for word; a refused call leaves the tree as it was.  The reference is
tests/poseidon_model.py's tree_levels over the edited leaf list (Python integers), computed once per (leaves, depth) and shared."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from zksnark_rs_amd import SplitMix64, ZkError, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd.circuit import Builder, Mixgen

import poseidon_model as pm

pytestmark = pytest.mark.gpu

R = pm.R
TREES = [(1, 0), (1, 1), (2, 1), (5, 3), (64, 6), (65, 7), (1000, 10), (1000, 20)]
COUNTS = (1, 63, 64, 65, 255, 256, 257)                     # lanes of a wave and of a workgroup of the update kernels, and one more


@functools.lru_cache(maxsize=None)
def model(leaves, depth):
    """leaves: a tuple -> the levels of the tree over them"""
    return pm.tree_levels(list(leaves), depth)


def drawn_leaves(n_leaves, depth):
    rng = SplitMix64(800 + 31 * n_leaves + depth)
    return ([0, R - 1] + [rng.fr() for _ in range(n_leaves)])[2 if n_leaves < 3 else 0:][:n_leaves]


def shuffled(rng, items):
    items = list(items)
    for i in range(len(items) - 1, 0, -1):
        j = rng.next() % (i + 1)
        items[i], items[j] = items[j], items[i]
    return items


def dims(tree):
    n, d = C.c_size_t(), C.c_uint()
    tree.ctx._check(tree.lib.zk_poseidon_tree_dims(tree.ptr, C.byref(n), C.byref(d)))
    return n.value, d.value


def check(tree, leaves, depth, what=None):
    """the tree equals the model over `leaves` at the root, in its dims and at every level"""
    levels = model(tuple(leaves), depth)
    assert dims(tree) == (len(leaves), depth) and tree.n_leaves == len(leaves), what
    assert tree.root == pm.tree_root(levels, depth), what
    for k in range(depth + 1):
        assert tree.level_size(k) == len(levels[k]), (what, k)
        assert tree.nodes(k) == levels[k], (what, k)


def snapshot(tree):
    return tree.root, dims(tree), tree.n_leaves, [tree.nodes(k) for k in range(tree.depth + 1)]


def values_for(rng, count):
    """drawn values; 0 and r - 1 are among them"""
    if count == 1:
        return [(0, R - 1)[rng.next() & 1]]
    return [0, R - 1] + [rng.fr() for _ in range(count - 2)]


def index_sets(n_leaves, depth, rng):
    sizes = [pm.level_size(n_leaves, k) for k in range(depth + 1)]
    sets = [("leaf 0", [0]), ("the last leaf", [n_leaves - 1])]
    odd = []
    for k in range(depth):                                  # the last node of a level of odd size: its sibling is z_k
        if sizes[k] % 2:
            leaf = min((sizes[k] - 1) << k, n_leaves - 1)
            if leaf not in odd:
                odd.append(leaf)
    if odd:
        sets.append(("the last nodes of the odd levels", odd[::-1]))
    if n_leaves >= 2:
        i = n_leaves // 4
        sets.append(("both children of a parent", [2 * i + 1, 2 * i]))
    if n_leaves >= 4:
        g = n_leaves // 8
        sets.append(("the four leaves of a grandparent", [4 * g + 2, 4 * g, 4 * g + 3, 4 * g + 1]))
    sets.append(("every leaf, reversed", list(range(n_leaves))[::-1]))
    for count in COUNTS:
        if count <= n_leaves:
            sets.append(("%d drawn" % count, shuffled(rng, range(n_leaves))[:count]))
    return sets


# ---- 1. update against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_leaves,depth", TREES)
def test_update_against_the_model_at_every_level(ctx, n_leaves, depth):
    leaves = drawn_leaves(n_leaves, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    rng = SplitMix64(1300 + 31 * n_leaves + depth)
    for what, indices in index_sets(n_leaves, depth, rng):
        values = values_for(rng, len(indices))
        tree.update(indices, values)
        for i, v in zip(indices, values):
            leaves[i] = v
        check(tree, leaves, depth, what)
    tree.close()


# ---- 2. sequences -------------------------------------------------------------------------------------------------------------
def test_update_append_update_then_paths(ctx):
    """1000 leaves, two overlapping updates, 65 appended leaves, an update of two of them, 65 paths.  The depth is 11, not 10:
    1000 + 65 leaves do not fit 2^10, so at depth 10 the same append is refused (checked first, with the append of 24 that fills
    that tree); at depth 11 it crosses 1024 leaves, where level 10 gets its second node."""
    n_leaves, depth = 1000, 10
    leaves = drawn_leaves(n_leaves, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    rng = SplitMix64(76)
    before = snapshot(tree)
    with pytest.raises(ZkError) as e:
        tree.append([rng.fr() for _ in range(65)])
    assert e.value.status == _lib.ZK_ERR_ARG and snapshot(tree) == before
    more = [rng.fr() for _ in range(24)]
    tree.append(more)
    check(tree, leaves + more, depth, "filled")
    tree.close()

    depth = 11
    tree = ctx.poseidon_tree(leaves, depth)
    rng = SplitMix64(77)
    first = shuffled(rng, range(n_leaves))[:100]
    second = first[50:] + [i for i in shuffled(rng, range(n_leaves)) if i not in first][:50]   # overlaps the first call's leaves
    for what, indices in (("first", first), ("second", second)):
        values = values_for(rng, len(indices))
        tree.update(indices, values)
        for i, v in zip(indices, values):
            leaves[i] = v
        check(tree, leaves, depth, what)
    more = [rng.fr() for _ in range(65)]
    tree.append(more)
    leaves += more
    check(tree, leaves, depth, "append")
    tree.update([1063, 1001], [R - 1, 0])                   # two of the appended leaves
    leaves[1063], leaves[1001] = R - 1, 0
    check(tree, leaves, depth, "update of appended leaves")
    levels = model(tuple(leaves), depth)
    root = pm.tree_root(levels, depth)
    indices = [0, 999, 1000, 1064, 1063, 1001, first[0], second[-1]]
    indices += [rng.next() % len(leaves) for _ in range(65 - len(indices))]
    fields, bits = tree.paths(indices)
    for j, index in enumerate(indices):
        vals = limbs_to_ints(fields[j])
        assert int.from_bytes(bytes(bits[j]), "little") == index, j
        leaf, sibs, dirs = pm.path(levels, depth, index)
        assert (vals[0], vals[1:]) == (leaf, sibs), j
        if j < 12:
            assert pm.fold(vals[0], vals[1:], dirs) == root, j
    tree.close()


# ---- 3. append against the model ------------------------------------------------------------------------------------------------
def test_append_from_an_empty_tree(ctx):
    depth = 11
    rng = SplitMix64(1100)
    pool = [0, R - 1] + [rng.fr() for _ in range(998)]
    tree = ctx.poseidon_tree([], depth)
    assert tree.root == pm.zero_hashes(depth)[depth]
    leaves = []
    for count in (1, 1, 1, 62, 191, 1, 743):                # 1, 2, 3, 65, 256, 257, 1000 leaves
        new = pool[len(leaves):len(leaves) + count]
        tree.append(new)
        leaves += new
        assert dims(tree) == (len(leaves), depth) and tree.n_leaves == len(leaves)
        assert tree.root == pm.tree_root(model(tuple(leaves), depth), depth), len(leaves)
        if len(leaves) in (65, 257, 1000):
            check(tree, leaves, depth, len(leaves))
    assert len(leaves) == 1000
    tree.close()


def test_append_fills_a_tree_and_is_then_refused(ctx):
    rng = SplitMix64(1101)
    tree = ctx.poseidon_tree([], 3)
    leaves = []
    for count in (1, 2, 5):
        new = [rng.fr() for _ in range(count)]
        tree.append(new)
        leaves += new
        check(tree, leaves, 3, len(leaves))
    before = snapshot(tree)
    with pytest.raises(ZkError) as e:
        tree.append([1])
    assert e.value.status == _lib.ZK_ERR_ARG and "depth 3" in str(e.value)
    assert snapshot(tree) == before
    tree.close()

    tree = ctx.poseidon_tree([], 0)                         # depth 0: the root is the one leaf
    assert tree.root == 0
    tree.append([R - 1])
    check(tree, [R - 1], 0)
    assert tree.root == R - 1
    with pytest.raises(ZkError) as e:
        tree.append([5])
    assert e.value.status == _lib.ZK_ERR_ARG
    check(tree, [R - 1], 0)
    tree.close()


@pytest.mark.parametrize("n_leaves,depth,counts", [(5, 3, (3,)), (63, 7, (1, 1)), (1000, 20, (65,))])
def test_append_to_a_built_tree(ctx, n_leaves, depth, counts):
    leaves = drawn_leaves(n_leaves, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    rng = SplitMix64(1200 + n_leaves)
    for count in counts:
        new = values_for(rng, count)
        tree.append(new)
        leaves += new
        check(tree, leaves, depth, len(leaves))
    tree.append_dev(0, 0)                                   # no leaves, a null pointer: ZK_OK
    check(tree, leaves, depth, "after an empty append")
    tree.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tree_as_it_was(ctx):
    n_leaves, depth = 65, 7
    leaves = drawn_leaves(n_leaves, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    before = snapshot(tree)
    rng = SplitMix64(1400)

    def refused(indices, values, status, pattern):
        with pytest.raises(ZkError) as e:
            tree.update(indices, values)
        assert e.value.status == status and re.search(pattern, str(e.value)), str(e.value)
        assert snapshot(tree) == before
        good = shuffled(rng, range(n_leaves))[:3]           # and a valid update goes through, here one that rewrites what is there
        tree.update(good, [leaves[i] for i in good])
        assert snapshot(tree) == before

    distinct = shuffled(rng, range(n_leaves)) + [0] * 15    # 80 instances: the first 65 are distinct leaves
    values = [rng.fr() for _ in range(80)]

    idx = distinct[:64] + [distinct[64]] * 16               # instances 64 .. 79 repeat a leaf: the range error still wins
    idx[70], idx[75] = n_leaves, n_leaves
    refused(idx, values, _lib.ZK_ERR_RANGE, r"instance 70\b")
    idx = distinct[:65]
    idx[20] = 1 << 40                                       # far out of range, alone
    refused(idx, values[:65], _lib.ZK_ERR_RANGE, r"instance 20\b")

    bad = list(values[:65])
    bad[40], bad[7] = R, (1 << 256) - 1
    refused(distinct[:65], bad, _lib.ZK_ERR_RANGE, r"instance 7\b")
    bad[7] = values[7]
    refused(distinct[:65], bad, _lib.ZK_ERR_RANGE, r"instance 40\b")

    rest = [i for i in range(n_leaves) if i not in (9, 33)]
    idx = rest[:61]
    idx[3], idx[60], idx[5], idx[6] = 9, 9, 33, 33
    refused(idx, values[:61], _lib.ZK_ERR_ARG, r"leaf 9\b")
    same = list(values[:61])
    same[60] = same[3]                                      # equal values: refused all the same
    refused(idx, same, _lib.ZK_ERR_ARG, r"leaf 9\b")

    idx[10] = n_leaves                                      # an index out of range next to the duplicates: the range error wins
    refused(idx, values[:61], _lib.ZK_ERR_RANGE, r"instance 10\b")
    bad = list(values[:61])
    bad[50] = R                                             # a value out of range next to the duplicates, every index in range
    idx[10] = rest[61]
    refused(idx, bad, _lib.ZK_ERR_RANGE, r"instance 50\b")

    d_idx = torch.zeros(1, dtype=torch.int64, device="cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    for d_i, d_v in ((d_idx.data_ptr(), 0), (0, d_idx.data_ptr())):
        with pytest.raises(ZkError) as e:
            tree.update_dev(d_i, d_v, 1)
        assert e.value.status == _lib.ZK_ERR_ARG
        assert snapshot(tree) == before
    tree.update_dev(0, 0, 0)                                # no instance, null pointers: ZK_OK
    assert snapshot(tree) == before

    with pytest.raises(ZkError) as e:
        tree.append([1, 2, R, (1 << 256) - 1])
    assert e.value.status == _lib.ZK_ERR_RANGE and re.search(r"position 2\b", str(e.value)), str(e.value)
    assert snapshot(tree) == before
    with pytest.raises(ZkError) as e:
        tree.append([1] * ((1 << depth) - n_leaves + 1))
    assert e.value.status == _lib.ZK_ERR_ARG
    assert snapshot(tree) == before
    with pytest.raises(ZkError) as e:
        tree.append_dev(0, 1)
    assert e.value.status == _lib.ZK_ERR_ARG
    assert snapshot(tree) == before

    tree.update([64, 0], [0, R - 1])                        # and the tree still works
    leaves[64], leaves[0] = 0, R - 1
    check(tree, leaves, depth)
    tree.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------
def membership_circuit(depth):
    """public: the root; private: leaf, siblings, directions -- created in the order PoseidonTree.paths writes them"""
    b = Builder()
    leaf = b.new_wire()
    sibs = [b.new_wire() for _ in range(depth)]
    dirs = b.new_bits(depth)
    root = b.merkle_root(leaf, sibs, dirs)
    return b.finish([root])


def test_membership_proofs_follow_the_changed_tree(ctx):
    depth, count = 3, 6
    c = membership_circuit(depth)
    leaves = drawn_leaves(5, depth)
    tree = ctx.poseidon_tree(leaves, depth)
    old_root = tree.root
    rng = SplitMix64(4343)
    tree.update([2], [rng.fr()])
    tree.append([rng.fr()])
    assert dims(tree) == (6, depth) and tree.root != old_root
    qap = c.qap_sparse_unity(ctx)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    mg = Mixgen(ctx, c)
    dev = "cuda:%d" % ctx.device
    d_idx = torch.from_numpy(np.arange(count, dtype=np.int64)).to(dev)
    d_f = torch.zeros((count, depth + 1, 4), dtype=torch.int64, device=dev)
    d_b = torch.zeros((count, tree.bit_bytes), dtype=torch.uint8, device=dev)
    d_w = torch.zeros((count, c.m, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr(), d_b.data_ptr())
    mg.run(d_b.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr())
    got = d_w.cpu().numpy().view(np.uint64)
    assert limbs_to_ints(got[:, 1]) == [tree.root] * count
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert [int(x) for x in res["bad_gates"]] == [0] * count and (res["first_bad"] == _lib.QAP_CHECK_NONE).all()
    ptrs = [d_w.data_ptr() + j * c.m * 32 for j in range(count)]
    ticket = ctx.prove_batch_submit(crs, qap, ptrs, [c.m] * count, [rng.fr() for _ in range(count)], [rng.fr() for _ in range(count)])
    proofs = ctx.prove_batch_wait(ticket, count)
    public = np.tile(ints_to_limbs([tree.root]).reshape(1, 1, 4), (count, 1, 1))
    assert ctx.verify_batch(crs, public, proofs).all()
    stale = np.tile(ints_to_limbs([old_root]).reshape(1, 1, 4), (count, 1, 1))
    assert not ctx.verify_batch(crs, stale, proofs).any()
    mg.close()
    crs.close()
    qap.close()
    tree.close()
