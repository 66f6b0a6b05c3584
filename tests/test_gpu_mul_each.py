"""-m gpu: k_mul_each (csrc/powers.hip), the kernel zk_powers_contribute multiplies a transcript with -- one scalar per point, regular
signed windows, the same instruction stream in every lane -- through its diagnostic entry points zk_g1_mul_each / zk_g2_mul_each.
Everything is compared with zk_g1_mul_batch / zk_g2_mul_batch (k_point_mul: plain double-and-add, pinned against the oracle by
test_gpu_blocks.py), and the two forms of the option powers_mul_form with each other, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, ZkError, _lib, ints_to_limbs
from zksnark_rs_amd.circuits import chain_rows

from test_powers_recode_host import edge_scalars

pytestmark = pytest.mark.gpu
R, Q = zk.R_MODULUS, zk.Q_MODULUS
PPL = [0, 1, 2, 4]                           # option powers_mul_ppl: points a lane of k_mul_each owns; 0 = chosen from the length (1 at these sizes)
TILE = 256                                   # the largest tile: 64 lanes x 4 points a work-group


def lengths(ppl):
    """1, 63, 64, 65 (a wave), T - 1, T, T + 1 and 2 T + 1 for the tile T = 64 ppl of that setting"""
    t = 64 * max(ppl, 1)
    return sorted({1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1})


GROUPS = ["g1", "g2"]


@pytest.fixture(scope="module")
def gens(ctx):
    m, l, u, v, w = chain_rows(1)
    a = ctx.crs_download(ctx.setup(ctx.qap_sparse(1, m, l, u, v, w), ints_to_limbs([3, 5, 7, 11, 13])))
    return {"g1": a["xi_g1"][0].copy(), "g2": a["xi_g2"][0].copy()}


@pytest.fixture(autouse=True)
def default_form(ctx):
    ctx.set_option("powers_mul_form", 0)
    ctx.set_option("powers_mul_ppl", 0)
    yield
    ctx.set_option("powers_mul_form", 0)
    ctx.set_option("powers_mul_ppl", 0)


def each(ctx, g):
    return ctx.g1_mul_each if g == "g1" else ctx.g2_mul_each


def batch(ctx, g):
    return ctx.g1_mul_batch if g == "g1" else ctx.g2_mul_batch


def some_points(ctx, gens, g, count, seed):
    """count points of the group: drawn multiples of the generator"""
    rng = SplitMix64(seed)
    return batch(ctx, g)(np.tile(gens[g], (count, 1)), ints_to_limbs([rng.fr() for _ in range(count)]))


def test_the_library_exports_the_calls_and_the_option(ctx):
    lib = _lib.load()
    assert lib.zk_g1_mul_each is not None and lib.zk_g2_mul_each is not None
    assert ctx.get_option("powers_mul_form") == 0                       # the new kernel is the default
    ctx.set_option("powers_mul_form", 1)
    assert ctx.get_option("powers_mul_form") == 1


@pytest.mark.parametrize("g", GROUPS)
def test_edge_scalars_on_edge_points(ctx, gens, g):
    """every edge scalar times the generator, a drawn point, 2 G and infinity: 4 x 46 products in one array, so that the lanes of a
    wave hold DIFFERENT edge scalars (a zero half next to a full one, either sign, either parity)"""
    scalars = edge_scalars()
    gen = gens[g]
    pts4 = [gen, some_points(ctx, gens, g, 1, 91000)[0], batch(ctx, g)(gen.reshape(1, -1), ints_to_limbs([2]))[0], np.zeros_like(gen)]
    points = np.stack([p for p in pts4 for _ in scalars])
    ks = ints_to_limbs(scalars * 4)
    want = batch(ctx, g)(points, ks)
    for ppl in PPL:                                                     # one, two and four points a lane: a lane's points share an inversion
        ctx.set_option("powers_mul_ppl", ppl)
        got = each(ctx, g)(points, ks)
        assert np.array_equal(got, want), ppl
    n = len(scalars)
    assert not got[3 * n:].any()                                        # infinity stays infinity
    assert not got[0].any() and not got[n].any()                        # the scalar 0 gives infinity
    assert np.array_equal(got[1], gen)                                  # 1 G = G
    ctx.set_option("powers_mul_form", 1)
    assert np.array_equal(each(ctx, g)(points, ks), want)


@pytest.mark.parametrize("g", GROUPS)
def test_a_different_edge_scalar_in_every_lane_of_a_wave(ctx, gens, g):
    """64 consecutive points = the 64 lanes of one wave at one of their four points: the first 64 edge scalars rotated, so that every
    lane's scalar differs from its neighbours' in sign pattern and in which half is zero"""
    scalars = list(dict.fromkeys(edge_scalars() + [R - j for j in range(3, 40)]))[:64]   # the list names 1 and 2 twice
    assert len(set(scalars)) == 64
    points = some_points(ctx, gens, g, 64, 91100)
    for rot, ppl in ((0, 1), (17, 4)):
        ctx.set_option("powers_mul_ppl", ppl)
        ks = ints_to_limbs(scalars[rot:] + scalars[:rot])
        assert np.array_equal(each(ctx, g)(points, ks), batch(ctx, g)(points, ks)), rot


@pytest.mark.parametrize("g", GROUPS)
def test_every_length_around_the_wave_and_the_tile(ctx, gens, g):
    """1, 63, 64, 65 (a wave), T - 1, T, T + 1 (a work-group's tile: the lanes of the last group own 0 to ppl points), 2 T + 1, for
    every number of points a lane can own; one reference for the longest, its prefixes for the others"""
    longest = 2 * TILE + 1
    rng = SplitMix64(91200)
    points = some_points(ctx, gens, g, longest, 91201)
    ks = ints_to_limbs([rng.fr() for _ in range(longest)])
    want = batch(ctx, g)(points, ks)
    forms = {}
    for form in (0, 1):
        ctx.set_option("powers_mul_form", form)
        for ppl in (PPL if form == 0 else [0]):
            ctx.set_option("powers_mul_ppl", ppl)
            for n in lengths(ppl):
                got = each(ctx, g)(points[:n], ks[:n])
                assert np.array_equal(got, want[:n]), (form, ppl, n)
        forms[form] = each(ctx, g)(points, ks)
    assert forms[0].tobytes() == forms[1].tobytes()                     # the two forms, byte for byte
    assert each(ctx, g)(points[:0], ks[:0]).shape[0] == 0


@pytest.mark.parametrize("g", GROUPS)
def test_out_may_be_points(ctx, gens, g):
    lib = _lib.load()
    n = TILE + 3
    ctx.set_option("powers_mul_ppl", 4)
    rng = SplitMix64(91300)
    points = some_points(ctx, gens, g, n, 91301)
    ks = ints_to_limbs([rng.fr() for _ in range(n)])
    want = batch(ctx, g)(points, ks)
    buf = np.ascontiguousarray(points.copy())
    fn = lib.zk_g1_mul_each if g == "g1" else lib.zk_g2_mul_each
    p = buf.ctypes.data_as(_lib.u64p)
    assert fn(ctx.ptr, p, np.ascontiguousarray(ks).ctypes.data_as(_lib.u64p), p, n) == 0
    assert np.array_equal(buf, want)


@pytest.mark.parametrize("g", GROUPS)
def test_range_refusals(ctx, gens, g):
    lib = _lib.load()
    points = some_points(ctx, gens, g, 3, 91400)
    ks = ints_to_limbs([5, 6, 7])
    for bad in (R, R + 1, (1 << 256) - 1):
        with pytest.raises(ZkError) as e:
            each(ctx, g)(points, ints_to_limbs([5, bad, 7]))
        assert e.value.status == _lib.ZK_ERR_RANGE
    big = points.copy()
    big[2, :4] = ints_to_limbs([Q]).reshape(4)
    with pytest.raises(ZkError) as e:
        each(ctx, g)(big, ks)
    assert e.value.status == _lib.ZK_ERR_RANGE
    fn = lib.zk_g1_mul_each if g == "g1" else lib.zk_g2_mul_each
    p, k = np.ascontiguousarray(points).ctypes.data_as(_lib.u64p), np.ascontiguousarray(ks).ctypes.data_as(_lib.u64p)
    out = np.zeros_like(points)
    assert fn(None, p, k, out.ctypes.data_as(_lib.u64p), 3) == _lib.ZK_ERR_ARG
    assert fn(ctx.ptr, None, k, out.ctypes.data_as(_lib.u64p), 3) == _lib.ZK_ERR_ARG
    assert fn(ctx.ptr, p, None, out.ctypes.data_as(_lib.u64p), 3) == _lib.ZK_ERR_ARG
    assert fn(ctx.ptr, p, k, None, 3) == _lib.ZK_ERR_ARG
    assert np.array_equal(each(ctx, g)(points, ks), batch(ctx, g)(points, ks))      # the context is still usable
