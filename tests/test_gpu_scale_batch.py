"""zk_g1_scale_batch (csrc/crs_contribute.hip k_g1_scale: every point of an array times ONE scalar) word for word against two
references: zk_g1_mul_batch with the scalar repeated (independent device code: one scalar per lane through jac_mul_words) and the
oracle's g1_mul_batch.  Counts sit on every grouping constant of the kernel, scalars on the corners of the recoding, infinity
entries on every position of a lane's inversion group.  No tolerance: words only."""
import ctypes as C

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, _lib, ints_to_limbs

import crs_contribute_model as cm
from test_crs_contribute_host import drawn_scalars, fixed_scalars

pytestmark = pytest.mark.gpu
R = zk.R_MODULUS
# the grouping constants of k_g1_scale (csrc/crs_contribute.hip)
SC_BLOCK = 64                 # lanes per work-group: one wave
SC_PPL = 4                    # points a lane owns: its inversion group (the points i, i + 64, i + 128, i + 192 of a tile)
SC_TILE = SC_BLOCK * SC_PPL   # points per work-group
N_MAX = (1 << 13) + 1
COUNTS = sorted({0, 1, 63, 64, 65} | {c + e for c in (SC_PPL, SC_BLOCK, SC_TILE) for e in (-1, 0, 1)} | {N_MAX})


@pytest.fixture(scope="module")
def points(orc):
    """N_MAX distinct points: (i + 1) (k0 G), shared by every test and never written"""
    rng = SplitMix64(66000)
    g = orc.g1_mul_batch(orc.enc_base_g1().reshape(1, 8), ints_to_limbs([rng.fr()]))
    pts = orc.g1_mul_batch(np.tile(g, (N_MAX, 1)), ints_to_limbs(list(range(1, N_MAX + 1))))
    pts.setflags(write=False)
    return pts


def reference(ctx, orc, pts, k, with_oracle=True):
    ks = np.tile(ints_to_limbs([k]), (len(pts), 1))
    want = ctx.g1_mul_batch(pts, ks) if len(pts) else np.zeros((0, 8), np.uint64)
    if with_oracle and len(pts):
        assert np.array_equal(want, orc.g1_mul_batch(np.ascontiguousarray(pts), ks))
    return want


@pytest.mark.parametrize("count", COUNTS)
def test_counts_on_every_grouping_constant(ctx, orc, points, count):
    k = SplitMix64(66100 + count).fr()
    got = ctx.g1_scale_batch(points[:count], k)
    assert got.shape == (count, 8)
    assert np.array_equal(got, reference(ctx, orc, points[:count], k, with_oracle=count <= 300))


def test_scalars_on_the_corners_of_the_recoding(ctx, orc, points):
    drawn, signs = [], set()
    for k in drawn_scalars(64, 66200):
        s = tuple(h < 0 for h in cm.glv_split(k))
        if s not in signs:
            signs.add(s)
            drawn.append(k)
    assert len(signs) == 4                      # each sign combination of (k1, k2) occurs (the Python split)
    pts = points[:SC_BLOCK + 3]
    for k in fixed_scalars() + list(range(41)) + drawn:
        assert np.array_equal(ctx.g1_scale_batch(pts, k), reference(ctx, orc, pts, k, with_oracle=k > 40 or k % 8 == 0)), hex(k)
    assert not ctx.g1_scale_batch(pts, 0).any()  # k = 0: every output is infinity


def test_infinity_entries(ctx, orc, points):
    n = 2 * SC_TILE + 5
    k = SplitMix64(66300).fr()
    lane = 7
    group = [lane + j * SC_BLOCK for j in range(SC_PPL)]            # one lane's inversion group in the first tile
    holes = [[0], [n - 1], [0, n - 1]] + [[g] for g in group] + [group, group[:2], group[1:], list(range(SC_TILE, 2 * SC_TILE)), list(range(n))]
    for h in holes:
        pts = np.array(points[:n], copy=True)
        pts[h] = 0
        got = ctx.g1_scale_batch(pts, k)
        assert np.array_equal(got, reference(ctx, orc, pts, k, with_oracle=False)), h[:4]
        assert not got[h].any() and got[[i for i in range(n) if i not in set(h)]].any(axis=1).all()


def test_in_place(ctx, orc, points):
    n = SC_TILE + SC_BLOCK + 1
    k = SplitMix64(66400).fr()
    buf = np.array(points[:n], copy=True)
    want = reference(ctx, orc, buf, k)
    kk = np.ascontiguousarray(ints_to_limbs([k]).reshape(4))
    p = buf.ctypes.data_as(_lib.u64p)
    assert ctx.lib.zk_g1_scale_batch(ctx.ptr, p, kk.ctypes.data_as(_lib.u64p), p, n) == 0
    assert np.array_equal(buf, want)


def test_range_and_null_arguments(ctx, orc, points):
    pts = np.array(points[:5], copy=True)
    with pytest.raises(zk.ZkError) as e:
        ctx.g1_scale_batch(pts, R)
    assert e.value.status == _lib.ZK_ERR_RANGE
    bad = pts.copy()
    bad[3, :4] = ints_to_limbs([cm.Q]).reshape(4)
    with pytest.raises(zk.ZkError) as e:
        ctx.g1_scale_batch(bad, 3)
    assert e.value.status == _lib.ZK_ERR_RANGE
    one = np.ascontiguousarray(ints_to_limbs([1]).reshape(4)).ctypes.data_as(_lib.u64p)
    p = pts.ctypes.data_as(_lib.u64p)
    assert ctx.lib.zk_g1_scale_batch(None, p, one, p, 5) == _lib.ZK_ERR_ARG
    assert ctx.lib.zk_g1_scale_batch(ctx.ptr, None, one, p, 5) == _lib.ZK_ERR_ARG
    assert ctx.lib.zk_g1_scale_batch(ctx.ptr, p, None, p, 5) == _lib.ZK_ERR_ARG
    assert ctx.lib.zk_g1_scale_batch(ctx.ptr, p, one, None, 5) == _lib.ZK_ERR_ARG
    assert np.array_equal(ctx.g1_scale_batch(pts, 1), pts)          # the context stays usable
    assert np.array_equal(ctx.g1_scale_batch(pts, R - 1)[:, :4], pts[:, :4])   # -P: the same x
