"""zk_eddsa_sign_batch on the device: the rows (A.x, A.y, R8.x, R8.y, M), S and the bit rows word for word against the host library
(eddsa.public_key / sign / challenge, which tests/test_eddsa.py holds against the model) in every lane at the wave and block edges, and
against tests/eddsa_model.py directly at the edge lanes; every quotient of the two reductions mod l in one wave; the edge values of
the three inputs; the refusals, which leave every output byte untouched; and the chain sign -> Mixgen -> QAP check with no verify call
and no host step between."""
import functools

import numpy as np
import pytest
import torch

import zksnark_rs_amd as zk
from zksnark_rs_amd import SplitMix64, _lib, eddsa, ints_to_limbs
from zksnark_rs_amd.babyjub import scalars_to_words
from zksnark_rs_amd.circuit import Mixgen, Witgen

import babyjub_model as bm
import eddsa_cases as ec
import eddsa_model as em

pytestmark = pytest.mark.gpu

R, L = bm.R, bm.L
FILL = 0xA5
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
EDGE_LANES = (0, 63, 64, 255, 256)


def to_dev(ctx, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:%d" % ctx.device)


def sign_dev(ctx, triples, stride=None, expect=None):
    """one call over (k, n, M) triples -> rows (count, 5, 4), S (count, 4) uint64 and, with a stride, bit rows (count, stride) uint8.
    One spare row or word behind each output must keep its fill byte.  expect: a ZkError is awaited and returned, and every output
    must be untouched."""
    count = len(triples)
    dev = "cuda:%d" % ctx.device
    d_k, d_n, d_m = [to_dev(ctx, scalars_to_words([t[i] for t in triples])) for i in range(3)]
    d_p = torch.full((count + 1, 160), FILL, dtype=torch.uint8, device=dev)
    d_s = torch.full((count + 1, 32), FILL, dtype=torch.uint8, device=dev)
    d_b = torch.full((count + 1, stride), FILL, dtype=torch.uint8, device=dev) if stride else None
    torch.cuda.synchronize()
    args = (d_k.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr(), None if d_b is None else d_b.data_ptr(), stride or 64)
    if expect is not None:
        with pytest.raises(zk.ZkError) as err:
            ctx.eddsa_sign_batch(*args)
        assert err.value.status == expect
        for out in (d_p, d_s, d_b):
            assert out is None or (out.cpu().numpy() == FILL).all()
        return err.value
    ctx.eddsa_sign_batch(*args)
    p, s = d_p.cpu().numpy(), d_s.cpu().numpy()
    assert (p[count] == FILL).all() and (s[count] == FILL).all()
    rows, sv = p[:count].copy().view(np.uint64).reshape(count, 5, 4), s[:count].copy().view(np.uint64).reshape(count, 4)
    if not stride:
        return rows, sv
    b = d_b.cpu().numpy()
    assert (b[count] == FILL).all() and (b[:, 64:] == FILL).all()          # bytes of a row past the 64th are not written
    return rows, sv, b[:count]


def bit_row(s, hm):
    return np.frombuffer((s | (hm << em.S_BITS)).to_bytes(64, "little"), np.uint8)


@functools.lru_cache(maxsize=None)
def drawn():
    """1000 distinct (k, n, M) and what the host library gives for each: A, R8, S, hm"""
    rng = SplitMix64(3700)
    triples = [(rng.fr() % L or 1, rng.fr(), rng.fr()) for _ in range(max(COUNTS))]
    assert len(set(triples)) == len(triples)
    host = []
    for k, n, msg in triples:
        a = eddsa.public_key(k)
        r8, s = eddsa.sign(k, n, msg)
        host.append((a, r8, s, eddsa.challenge(r8, a, msg)))
    return tuple(triples), tuple(host)


@functools.lru_cache(maxsize=None)
def model(k, n, msg):
    """(A, R8, S, hm) from the model"""
    a = em.public_key(k)
    r8, s = em.sign(k, n, msg)
    return a, r8, s, em.challenge(r8, a, msg)


def assert_lane(rows, sv, bits, j, triple, want):
    a, r8, s, hm = want
    assert [int(x) for x in zk.limbs_to_ints(rows[j])] == [a[0], a[1], r8[0], r8[1], triple[2]], j
    assert zk.limbs_to_int(sv[j]) == s, j
    if bits is not None:
        assert np.array_equal(bits[j, :64], bit_row(s, hm)), j


# ---- a. counts at the wave and block edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_every_lane_against_the_host_library(ctx, count):
    triples, host = drawn()
    triples, host = list(triples[:count]), host[:count]
    rows, sv = sign_dev(ctx, triples)
    r64, s64, b64 = sign_dev(ctx, triples, 64)
    r72, s72, b72 = sign_dev(ctx, triples, 72)
    assert np.array_equal(rows, r64) and np.array_equal(rows, r72) and np.array_equal(sv, s64) and np.array_equal(sv, s72)
    assert np.array_equal(b64, b72[:, :64])
    want_rows = np.stack([ints_to_limbs([a[0], a[1], r8[0], r8[1], t[2]]) for t, (a, r8, s, hm) in zip(triples, host)])
    assert np.array_equal(rows, want_rows), np.argwhere((rows != want_rows).any(axis=(1, 2)))[:3]
    want_s = scalars_to_words([h[2] for h in host])
    assert np.array_equal(sv, want_s), np.argwhere((sv != want_s).any(axis=1))[:3]
    want_bits = np.stack([bit_row(s, hm) for _, _, s, hm in host])
    assert np.array_equal(b64, want_bits), np.argwhere((b64 != want_bits).any(axis=1))[:3]
    for j in sorted({j for j in EDGE_LANES + (count - 1,) if j < count}):
        assert_lane(rows, sv, b72, j, triples[j], model(*triples[j]))
    # what was signed verifies, and verification writes the same bit rows
    d_p, d_s = to_dev(ctx, rows), to_dev(ctx, sv)
    d_st = torch.full((count,), -1, dtype=torch.int32, device=d_p.device)
    d_b = torch.full((count, 72), FILL, dtype=torch.uint8, device=d_p.device)
    torch.cuda.synchronize()
    ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr(), d_b.data_ptr(), 72)
    assert (d_st.cpu().numpy() == em.VALID).all()
    assert np.array_equal(d_b.cpu().numpy(), b72)


def test_host_form(ctx):
    triples, host = drawn()
    ks, ns, ms = zip(*triples[:5])
    rows, sv, bits = ctx.eddsa_sign_batch(list(ks), list(ns), list(ms), bits=True)
    assert rows.shape == (5, 5, 4) and sv.shape == (5, 4) and bits.shape == (5, 64) and rows.dtype == np.uint64 and sv.dtype == np.uint64
    for j in range(5):
        assert_lane(rows, sv, bits, j, triples[j], host[j])
    r2, s2 = ctx.eddsa_sign_batch(scalars_to_words(ks), scalars_to_words(ns), scalars_to_words(ms))
    assert np.array_equal(r2, rows) and np.array_equal(s2, sv)
    r0, s0 = ctx.eddsa_sign_batch([], [], [])
    assert r0.shape == (0, 5, 4) and s0.shape == (0, 4)
    with pytest.raises(zk.ZkError) as err:
        ctx.eddsa_sign_batch([1, 2], [3], [4, 5])
    assert err.value.status == _lib.ZK_ERR_ARG
    with pytest.raises(zk.ZkError) as err:
        ctx.eddsa_sign_batch([1, L], [3, 4], [4, 5])
    assert err.value.status == _lib.ZK_ERR_RANGE and "instance 1" in str(err.value)


# ---- b. every quotient of the two reductions mod l in one wave ----------------------------------------------------------------------
RHO_QUOTIENT_INPUTS = (1, 10, 3, 0, 4, 18, 2, 8)            # n = i, M = i + 1: floor(H6(n, M, 0, 0, 0) / l) = 0 .. 7


def test_every_quotient_of_both_reductions_in_one_wave(ctx):
    k0 = ec.keys()[3][0]
    triples = [(k0, i, i + 1) for i in RHO_QUOTIENT_INPUTS]
    assert [em.h6(n, msg, 0, 0, 0) // L for _, n, msg in triples] == list(range(8))
    by_quotient = {}
    rng = SplitMix64(3701)
    for _ in range(400):
        if len(by_quotient) == 8:
            break
        t = (rng.fr() % L or 1, rng.fr(), rng.fr())
        by_quotient.setdefault(model(*t)[3] // L, t)
    assert sorted(by_quotient) == list(range(8))             # all eight of both before the device is looked at
    triples += [by_quotient[q] for q in range(8)]
    assert {model(*t)[3] // L for t in triples} == set(range(8))
    rows, sv, bits = sign_dev(ctx, triples, 64)
    for j, t in enumerate(triples):
        assert_lane(rows, sv, bits, j, t, model(*t))


# ---- c. edge values of the three inputs ---------------------------------------------------------------------------------------------
def test_edge_values_at_the_wave_edges(ctx):
    edges = [(k, n, msg) for k in (1, L - 1) for n in (0, R - 1) for msg in (0, R - 1, 1 << 253)]
    filler, _ = drawn()
    count = 130
    lanes = (0, 63, 64, count - 1)
    for first in range(0, len(edges), len(lanes)):
        triples = list(filler[:count])
        for lane, t in zip(lanes, edges[first:first + len(lanes)]):
            triples[lane] = t
        rows, sv, bits = sign_dev(ctx, triples, 64)
        for lane in lanes:
            assert_lane(rows, sv, bits, lane, triples[lane], model(*triples[lane]))
        assert_lane(rows, sv, bits, 1, triples[1], drawn()[1][1])     # a neighbour is what it was


# ---- d. refusals --------------------------------------------------------------------------------------------------------------------
PLANTED = (("key", 0, 0), ("key", 0, L), ("key", 0, (1 << 256) - 1), ("nonce key", 1, R), ("message", 2, R))


@pytest.mark.parametrize("lane", (0, 63, 64, 256))
def test_range_refusals_leave_the_outputs_untouched(ctx, lane):
    count = 257
    good = list(drawn()[0][:count])
    for name, which, value in PLANTED:
        triples = list(good)
        t = list(triples[lane])
        t[which] = value
        triples[lane] = tuple(t)
        err = sign_dev(ctx, triples, 72, expect=_lib.ZK_ERR_RANGE)
        assert "eddsa" in str(err) and "the %s of instance %d " % (name, lane) in str(err), (str(err), name, lane)
    # two offenders: the lowest instance is named; within one instance the key, then the nonce key, then the message
    if lane:
        triples = list(good)
        triples[lane] = (0, good[lane][1], good[lane][2])
        triples[lane - 1] = (good[lane - 1][0], good[lane - 1][1], R)
        err = sign_dev(ctx, triples, 64, expect=_lib.ZK_ERR_RANGE)
        assert "the message of instance %d " % (lane - 1) in str(err), str(err)
    triples = list(good)
    triples[lane] = (L, R, R)
    assert "the key of instance %d " % lane in str(sign_dev(ctx, triples, None, expect=_lib.ZK_ERR_RANGE))
    triples[lane] = (good[lane][0], R, R)
    assert "the nonce key of instance %d " % lane in str(sign_dev(ctx, triples, None, expect=_lib.ZK_ERR_RANGE))
    # the context signs as before after a refusal
    rows, sv = sign_dev(ctx, good[:2])
    assert_lane(rows, sv, None, 1, good[1], drawn()[1][1])


def test_argument_refusals_and_count_zero(ctx):
    triples = list(drawn()[0][:4])
    dev = "cuda:%d" % ctx.device
    d_k, d_n, d_m = [to_dev(ctx, scalars_to_words([t[i] for t in triples])) for i in range(3)]
    d_p = torch.full((5, 160), FILL, dtype=torch.uint8, device=dev)
    d_s = torch.full((5, 32), FILL, dtype=torch.uint8, device=dev)
    d_b = torch.full((5, 72), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    k, n, m, p, s, b = [t.data_ptr() for t in (d_k, d_n, d_m, d_p, d_s, d_b)]
    bad = [(0, n, m, 4, p, s, None, 64), (k, 0, m, 4, p, s, None, 64), (k, n, 0, 4, p, s, None, 64), (k, n, m, 4, 0, s, None, 64),
           (k, n, m, 4, p, 0, None, 64), (k + 4, n, m, 4, p, s, None, 64), (k, n + 4, m, 4, p, s, None, 64), (k, n, m + 4, 4, p, s, None, 64),
           (k, n, m, 4, p + 4, s, None, 64), (k, n, m, 4, p, s + 4, None, 64), (k, n, m, 4, p, s, b + 4, 64), (k, n, m, 4, p, s, b, 56),
           (k, n, m, 4, p, s, b, 68), (k, n, m, 4, p, s, b, 0)]
    for args in bad:
        with pytest.raises(zk.ZkError) as err:
            ctx.eddsa_sign_batch(*args)
        assert err.value.status == _lib.ZK_ERR_ARG and "eddsa" in str(err.value), args
    ctx.eddsa_sign_batch(0, 0, 0, 0, 0, 0, None, 64)         # count == 0 touches nothing, null pointers included
    ctx.eddsa_sign_batch(k, n, m, 0, p, s, b, 64)
    for out in (d_p, d_s, d_b):
        assert (out.cpu().numpy() == FILL).all()
    ctx.eddsa_sign_batch(k, n, m, 4, p, s, b, 72)
    assert (d_p.cpu().numpy()[4] == FILL).all() and (d_s.cpu().numpy()[4] == FILL).all() and (d_b.cpu().numpy()[4] == FILL).all()
    rows = d_p.cpu().numpy()[:4].copy().view(np.uint64).reshape(4, 5, 4)
    sv = d_s.cpu().numpy()[:4].copy().view(np.uint64).reshape(4, 4)
    for j in range(4):
        assert_lane(rows, sv, d_b.cpu().numpy(), j, triples[j], drawn()[1][j])


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    triples = list(drawn()[0][:300])
    first = sign_dev(ctx, triples, 72)
    second = sign_dev(ctx, triples, 72)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


# ---- e. the chain: sign -> Mixgen -> QAP check, nothing between ---------------------------------------------------------------------
CHAIN_COUNT = 65


def test_chain_sign_mixgen_qap_check(ctx):
    case = ec.gadget_case()
    m = case.c.m
    count = CHAIN_COUNT
    triples = list(drawn()[0][:count])
    dev = "cuda:%d" % ctx.device
    d_k, d_n, d_m = [to_dev(ctx, scalars_to_words([t[i] for t in triples])) for i in range(3)]
    d_p = torch.zeros((count, 20), dtype=torch.int64, device=dev)
    d_s = torch.zeros((count, 4), dtype=torch.int64, device=dev)
    d_bits = torch.zeros((count, 64), dtype=torch.uint8, device=dev)
    d_w = torch.empty((count + 1, m, 4), dtype=torch.int64, device=dev)
    d_w.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    ctx.eddsa_sign_batch(d_k.data_ptr(), d_n.data_ptr(), d_m.data_ptr(), count, d_p.data_ptr(), d_s.data_ptr(), d_bits.data_ptr(), 64)
    mg = Mixgen(ctx, case.c)
    mg.run(d_bits.data_ptr(), d_p.data_ptr(), count, d_w.data_ptr(), in_stride=64)
    qap = case.c.qap_sparse_unity(ctx)
    try:
        res = ctx.qap_check_dev(qap, d_w.data_ptr(), m, count)
        assert [int(x) for x in res["bad_gates"]] == [0] * count
        assert (d_w[count:].cpu().numpy().view(np.uint8) == FILL).all()
        # the same inputs as field elements through the tape
        bits = np.unpackbits(d_bits.cpu().numpy(), axis=1, bitorder="little")[:, :em.S_BITS + em.HM_BITS]
        ins = np.zeros((count, 5 + bits.shape[1], 4), np.uint64)
        ins[:, :5] = d_p.cpu().numpy().view(np.uint64).reshape(count, 5, 4)
        ins[:, 5:, 0] = bits
        wg = Witgen(ctx, case.c)
        d_t = torch.empty((count, m, 4), dtype=torch.int64, device=dev)
        d_in = to_dev(ctx, ins)
        torch.cuda.synchronize()
        wg.run(d_in.data_ptr(), count, d_t.data_ptr())
        wg.close()
        assert torch.equal(d_t, d_w[:count])
        # one message word flipped after signing: that instance, and only it, fails
        d_p[7, 16] ^= 1
        torch.cuda.synchronize()
        mg.run(d_bits.data_ptr(), d_p.data_ptr(), count, d_w.data_ptr(), in_stride=64)
        res = ctx.qap_check_dev(qap, d_w.data_ptr(), m, count)
        assert [int(x) == 0 for x in res["bad_gates"]] == [j != 7 for j in range(count)]
    finally:
        mg.close()
        qap.close()
