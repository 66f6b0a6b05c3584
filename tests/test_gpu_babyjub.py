"""Baby Jubjub on the device (csrc/babyjub.hip): zk_babyjub_mul_batch, fixed and variable base, at every lane, wave and workgroup
edge, on the edge scalars and points and on every (window, digit) of the kernels' windows, with packed and strided output; its
refusals; the chain secrets -> keys -> leaves -> tree without a host step; and the identity statement "I know the secret key of a
leaf of this tree" fed device to device from mul_batch and the tree's paths through zk_mixgen_run to proofs that verify against the
tree's root.  The reference is tests/babyjub_model.py (Python integers), computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from zksnark_rs_amd import SplitMix64, ZkError, _lib, ints_to_limbs, limbs_to_ints
from zksnark_rs_amd import babyjub
from zksnark_rs_amd.circuit import Builder, Mixgen, Witgen

import babyjub_model as bm
import poseidon_model as pm

pytestmark = pytest.mark.gpu

R = bm.R
FILL = 0xA5                                                 # the byte an output buffer holds before a call
BLOCK = 256                                                 # lanes of a workgroup of the kernels
COUNTS = (1, 63, 64, 65, 255, 256, 257, 2 * BLOCK + 1)
N = max(COUNTS)
EDGE_LANES = (0, 63, 64, 255, 256, 512)                     # the first and last lane of a wave and of a workgroup


def to_dev(ctx, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:%d" % ctx.device)


def points_to_limbs(points):
    return np.stack([ints_to_limbs(list(p)) for p in points])


def draw_scalar(rng):
    return (rng.fr() << 128 ^ rng.fr()) & ((1 << 256) - 1)


@functools.lru_cache(maxsize=None)
def multiples_of_generator():
    """k -> [k] Generator for k < N + 1, by repeated addition"""
    out = [bm.IDENTITY]
    for _ in range(N):
        out.append(bm.add(out[-1], bm.GENERATOR))
    return out


@functools.lru_cache(maxsize=None)
def fixed_case():
    """N scalars: the edge scalars in front and at the lane edges, drawn ones elsewhere; their multiples of Base8 by the model"""
    rng = SplitMix64(1700)
    scalars = [draw_scalar(rng) for _ in range(N)]
    scalars[:len(bm.EDGE_SCALARS)] = bm.EDGE_SCALARS
    for lane, k in zip(EDGE_LANES, ((1 << 256) - 1, 0, bm.L, 1 << 255, bm.R - 1, 8 * bm.L)):
        scalars[lane] = k
    return scalars, [bm.pmul(k) for k in scalars]


@functools.lru_cache(maxsize=None)
def var_case():
    """N (scalar, point) pairs: the edge points against the edge scalars in front, the edge points at the lane edges, drawn multiples
    of Generator against drawn scalars elsewhere"""
    rng = SplitMix64(1800)
    edge, gen = bm.edge_points(), multiples_of_generator()
    scalars = [draw_scalar(rng) for _ in range(N)]
    points = [gen[1 + rng.next() % N] for _ in range(N)]
    at = 1
    for i, p in enumerate(edge):                            # every edge point meets edge scalars, the pairing shifted per point
        for t in range(3):
            scalars[at], points[at] = bm.EDGE_SCALARS[(i + 5 * t) % len(bm.EDGE_SCALARS)], p
            at += 1
    for lane, p, k in zip(EDGE_LANES, edge, ((1 << 256) - 1, bm.L, 0, 8 * bm.L - 1, 1 << 255, bm.R - 1)):
        scalars[lane], points[lane] = k, p
    return scalars, points, [bm.pmul(k, p) for k, p in zip(scalars, points)]


def run_batch(ctx, d_s, d_p, count, stride):
    """-> (results (count, 2, 4), everything the call must not have written)"""
    rows = count + 3
    d_out = torch.empty((rows, stride), dtype=torch.int64, device=d_s.device)
    d_out.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    ctx.babyjub_mul_batch(d_s.data_ptr(), None if d_p is None else d_p.data_ptr(), count, d_out.data_ptr(), stride)
    out = d_out.cpu().numpy().view(np.uint64)
    untouched = np.concatenate([out[:count, 8:].reshape(-1), out[count:].reshape(-1)])
    return out[:count, :8].reshape(count, 2, 4), untouched


# ---- zk_babyjub_mul_batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [8, 24])
def test_fixed_base_at_every_edge(ctx, stride):
    scalars, want = fixed_case()
    d_s = to_dev(ctx, babyjub.scalars_to_words(scalars))
    for count in COUNTS:
        got, untouched = run_batch(ctx, d_s, None, count, stride)
        assert [tuple(limbs_to_ints(p)) for p in got] == want[:count], count
        assert (untouched.view(np.uint8) == FILL).all(), count
    got = ctx.babyjub_mul_batch(scalars[:5])                # the host form, and stride 0 = packed
    assert [tuple(limbs_to_ints(p)) for p in got] == want[:5]


@pytest.mark.parametrize("stride", [8, 24])
def test_variable_base_at_every_edge(ctx, stride):
    scalars, points, want = var_case()
    d_s, d_p = to_dev(ctx, babyjub.scalars_to_words(scalars)), to_dev(ctx, points_to_limbs(points))
    for count in COUNTS:
        got, untouched = run_batch(ctx, d_s, d_p, count, stride)
        assert [tuple(limbs_to_ints(p)) for p in got] == want[:count], count
        assert (untouched.view(np.uint8) == FILL).all(), count
    got = ctx.babyjub_mul_batch(scalars[:5], points[:5])
    assert [tuple(limbs_to_ints(p)) for p in got] == want[:5]


def test_every_window_and_digit(ctx):
    """one scalar per (window, digit): digit j in window k alone, for the fixed-base kernel's 64 windows of 4 bits and the
    variable-base kernel's 128 windows of 2 bits"""
    w = babyjub.FIXED_WINDOW
    scalars = [j << (w * k) for k in range(256 // w) for j in range(1 << w)]
    base, want = bm.BASE8, []
    for k in range(256 // w):                               # j 2^(w k) Base8 by repeated addition
        acc = bm.IDENTITY
        for j in range(1 << w):
            want.append(acc)
            acc = bm.add(acc, base)
        base = acc
    got = ctx.babyjub_mul_batch(scalars)
    assert [tuple(limbs_to_ints(p)) for p in got] == want
    w = babyjub.VAR_WINDOW
    scalars = [j << (w * k) for k in range(256 // w) for j in range(1 << w)]
    p = multiples_of_generator()[3]
    base, want = p, []
    for k in range(256 // w):
        acc = bm.IDENTITY
        for j in range(1 << w):
            want.append(acc)
            acc = bm.add(acc, base)
        base = acc
    got = ctx.babyjub_mul_batch(scalars, [p] * len(scalars))
    assert [tuple(limbs_to_ints(q)) for q in got] == want


def test_refusals_leave_the_output_untouched(ctx):
    scalars, points, want = var_case()
    count = 100
    good = points_to_limbs(points[:count])
    d_s = to_dev(ctx, babyjub.scalars_to_words(scalars[:count]))

    def refused(limbs, word):
        d_p = to_dev(ctx, limbs)
        d_out = torch.empty((count, 8), dtype=torch.int64, device=d_s.device)
        d_out.view(torch.uint8).fill_(FILL)
        torch.cuda.synchronize()
        with pytest.raises(ZkError) as e:
            ctx.babyjub_mul_batch(d_s.data_ptr(), d_p.data_ptr(), count, d_out.data_ptr(), 8)
        assert e.value.status == _lib.ZK_ERR_RANGE and word in str(e.value), str(e.value)
        assert (d_out.cpu().numpy().view(np.uint8) == FILL).all()

    bad = good.copy()
    bad[70, 1] = ints_to_limbs([R])[0]                      # y = r at instance 70, x = r at instance 5, off the curve at 64
    bad[5, 0] = ints_to_limbs([R])[0]
    bad[64, 1, 0] ^= np.uint64(1)
    refused(bad, ">= r in instance 5")
    bad[5] = good[5]
    refused(bad, ">= r in instance 70")                     # range before curve, although instance 64 comes first
    bad[70] = good[70]
    refused(bad, "curve in instance 64")
    assert [tuple(limbs_to_ints(p)) for p in ctx.babyjub_mul_batch(scalars[:count], points[:count])] == want[:count]   # the context goes on working
    d_p = to_dev(ctx, good)
    ctx.babyjub_mul_batch(0, None, 0, 0)                    # count == 0: nothing is touched
    for args in ((0, None, 1, d_p.data_ptr(), 8), (d_s.data_ptr(), None, 1, 0, 8), (d_s.data_ptr(), None, 1, d_p.data_ptr(), 7),
                 (d_s.data_ptr() + 4, None, 1, d_p.data_ptr(), 8)):
        with pytest.raises(ZkError) as e:
            ctx.babyjub_mul_batch(*args)
        assert e.value.status == _lib.ZK_ERR_ARG


# ---- secrets -> keys -> leaves -> tree, device to device ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def identities(count):
    rng = SplitMix64(1900)
    secrets = [draw_scalar(rng) for _ in range(count)]
    secrets[:3] = [bm.L - 1, (1 << 256) - 1, 1]
    keys = [bm.pmul(k) for k in secrets]
    return secrets, keys, [pm.hash(list(k)) for k in keys]


def test_secrets_to_tree_without_a_host_step(ctx):
    """65 leaves need depth 7: a tree of depth 3 holds 8 and refuses them"""
    count, depth = 65, 7
    secrets, keys, leaves = identities(count)
    d_s = to_dev(ctx, babyjub.scalars_to_words(secrets))
    d_keys = torch.zeros((count, 8), dtype=torch.int64, device=d_s.device)
    d_leaves = torch.zeros((count, 4), dtype=torch.int64, device=d_s.device)
    torch.cuda.synchronize()
    ctx.babyjub_mul_batch(d_s.data_ptr(), None, count, d_keys.data_ptr(), 0)
    ctx.poseidon_hash_batch(d_keys.data_ptr(), 2, count, d_leaves.data_ptr())    # the packed keys are the hash's input as they lie
    tree = ctx.poseidon_tree(d_leaves.data_ptr(), depth, n_leaves=count)
    assert tree.root == pm.tree_root(pm.tree_levels(leaves, depth), depth)
    assert limbs_to_ints(d_leaves.cpu().numpy().view(np.uint64)) == leaves
    tree.close()
    with pytest.raises(ZkError) as e:
        ctx.poseidon_tree(d_leaves.data_ptr(), 3, n_leaves=count)
    assert e.value.status == _lib.ZK_ERR_ARG


# ---- the identity statement ---------------------------------------------------------------------------------------------------
DEPTH, LEAVES = 3, 5


def identity_circuit():
    """public: the root.  Field inputs Ax, Ay, siblings; bit inputs the 256 bits of the secret, then the directions"""
    b = Builder()
    ax, ay = b.new_wire(), b.new_wire()
    sibs = [b.new_wire() for _ in range(DEPTH)]
    bits = b.new_bits(256)
    dirs = b.new_bits(DEPTH)
    key = b.babyjub_mul_fixed(bits)
    b.babyjub_affine(key, [ax, ay])
    leaf = b.poseidon([ax, ay])
    root = b.merkle_root(leaf, sibs, dirs)
    assert b.dims()[1] == 1446 + 4 + 244 + 246 * DEPTH
    return b.finish([root])


@pytest.fixture(scope="module")
def statement(ctx):
    c = identity_circuit()
    d = c.mixed_dims()
    assert (d["n_bit_inputs"], d["n_field_inputs"], c.input) == (256 + DEPTH, 2 + DEPTH, 1)
    secrets, keys, leaves = identities(LEAVES)
    tree = ctx.poseidon_tree(leaves, DEPTH)
    assert tree.root == pm.tree_root(pm.tree_levels(leaves, DEPTH), DEPTH)
    qap = c.qap_sparse_unity(ctx)
    rng = SplitMix64(4343)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    yield c, tree, qap, crs, rng
    crs.close()
    qap.close()
    tree.close()


ROW_WORDS = 4 * (2 + DEPTH)                                 # a row of d_in_fields: Ax, Ay, siblings
ROW_BYTES = 33                                              # a row of d_in_bits: the secret's 32 bytes, then the directions


def run_statement(ctx, c, tree, mg, indices, key_of=None, edit=None):
    """secrets and leaf indices -> witnesses.  tree.paths writes leaf | siblings one element into each row, so the siblings land in
    their place and the leaf where Ay goes; mul_batch then writes (Ax, Ay) over the row's head with the row as its stride.  The
    secret's words are the bit inputs as they lie; a device copy puts them in front of the direction bytes.  key_of: the secret
    whose key instance j supplies (default: its own)."""
    count = len(indices)
    secrets, _, _ = identities(LEAVES)
    d_idx = to_dev(ctx, np.array(indices, np.uint64))
    d_s = to_dev(ctx, babyjub.scalars_to_words([secrets[i] for i in indices]))
    d_ks = d_s if key_of is None else to_dev(ctx, babyjub.scalars_to_words([secrets[i] for i in key_of]))
    d_f = torch.zeros((count * ROW_WORDS + 4,), dtype=torch.int64, device=d_idx.device)
    d_b = torch.zeros((count, ROW_BYTES), dtype=torch.uint8, device=d_idx.device)
    d_w = torch.empty((count, c.m, 4), dtype=torch.int64, device=d_idx.device)
    d_w.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    tree.paths_dev(d_idx.data_ptr(), count, d_f.data_ptr() + 32, d_b.data_ptr() + 32, field_stride_words=ROW_WORDS, bits_stride_bytes=ROW_BYTES)
    ctx.babyjub_mul_batch(d_ks.data_ptr(), None, count, d_f.data_ptr(), ROW_WORDS)
    d_b[:, :32] = d_s.view(torch.uint8).view(count, 32)
    if edit:
        edit(d_f.view(torch.int64)[:count * ROW_WORDS].view(count, 2 + DEPTH, 4), d_b)
    torch.cuda.synchronize()
    mg.run(d_b.data_ptr(), d_f.data_ptr(), count, d_w.data_ptr(), in_stride=ROW_BYTES)
    fields = d_f.cpu().numpy().view(np.uint64)[:count * ROW_WORDS].reshape(count, 2 + DEPTH, 4)
    return d_w, fields, d_b.cpu().numpy()


@pytest.mark.parametrize("count", [1, 64, 65])
def test_identity_witnesses_device_to_device(ctx, statement, count):
    c, tree, qap, crs, rng = statement
    secrets, keys, leaves = identities(LEAVES)
    indices = [(3 * j + 1) % LEAVES for j in range(count)]
    mg = Mixgen(ctx, c)
    d_w, fields, bits = run_statement(ctx, c, tree, mg, indices)
    got = d_w.cpu().numpy().view(np.uint64)
    for j in range(min(count, 7)):
        assert tuple(limbs_to_ints(fields[j, :2])) == keys[indices[j]]
        assert int.from_bytes(bytes(bits[j, :32]), "little") == secrets[indices[j]] and bits[j, 32] == indices[j]
    n_in = 2 + DEPTH + 256 + DEPTH
    tape_in = np.zeros((count, n_in, 4), np.uint64)         # the same inputs as field elements in creation order
    tape_in[:, :2 + DEPTH] = fields
    for k in range(256 + DEPTH):
        tape_in[:, 2 + DEPTH + k, 0] = (bits[:, k // 8] >> (k % 8)) & 1
    wg = Witgen(ctx, c)
    assert np.array_equal(got, wg.run_numpy(tape_in))
    wg.close()
    for j in range(min(count, 3)):
        assert np.array_equal(got[j], c.weights_mixed(bytes(bits[j]), fields[j])), j
    assert limbs_to_ints(got[:, 1]) == [tree.root] * count
    res = ctx.qap_check_dev(qap, d_w.data_ptr(), c.m, count)
    assert [int(x) for x in res["bad_gates"]] == [0] * count and (res["first_bad"] == _lib.QAP_CHECK_NONE).all()
    mg.close()


def test_identity_proofs_verify_against_the_tree_root(ctx, statement):
    c, tree, qap, crs, rng = statement
    count = 65
    indices = [j % LEAVES for j in range(count)]
    mg = Mixgen(ctx, c)
    d_w, _, _ = run_statement(ctx, c, tree, mg, indices)
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
    other = ctx.poseidon_tree([7, 8, 9, 10, 11], DEPTH)      # another tree's root: refused by the verdict
    assert other.root != tree.root
    wrong = public.copy()
    wrong[11, 0] = ints_to_limbs([other.root])[0]
    assert [j for j, ok in enumerate(ctx.verify_batch(crs, wrong, proofs)) if not ok] == [11]
    other.close()

    # instance 1 supplies the key of another leaf's secret; instance 2 supplies its own Ax off by one: the gates that pin the
    # affine coordinates fail, and the QAP check says so
    def off_by_one(d_f, d_b):
        d_f[2, 0, 0] += 1
    d_t, _, _ = run_statement(ctx, c, tree, mg, [4, 4, 4], key_of=[4, 3, 4], edit=off_by_one)
    res = ctx.qap_check_dev(qap, d_t.data_ptr(), c.m, 3)
    assert [int(x) > 0 for x in res["bad_gates"]] == [False, True, True]
    affine_x = 1446 + 1                                     # the assertion (x Z - X) * 1 = 0 behind the 1446 gates of mul_fixed
    assert int(res["first_bad"][1]) == affine_x and int(res["first_bad"][2]) == affine_x and int(res["bad_gates"][2]) == 1
    mg.close()
