"""zk_eddsa_verify_batch on the device against tests/eddsa_model.py: the status array entry for entry at the wave and block edges with
every status planted among valid neighbours, the whole status set in one wave, the bit rows bit for bit at two strides, the
refusals, the keys of zk_babyjub_mul_batch fed device to device, and the chain verify -> Mixgen / Witgen -> QAP check -> proofs: the
verdict equals the circuit's satisfiability.  The valid signatures are made by the library's host signer, which tests/test_eddsa.py
holds byte for byte against the model; the planted defects and every expected status come from the model (eddsa_cases)."""
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
EDGE_LANES = (0, 63, 64, 255, 256)                          # the first lane, the last of a wave, the first of the next, the same of a block


@functools.lru_cache(maxsize=None)
def valid_pool():
    """64 distinct valid signatures (A, M, R8, S) over four keys"""
    rng = SplitMix64(3300)
    out = []
    for j in range(64):
        k, a = ec.keys()[j % 4]
        msg = rng.fr()
        r8, s = eddsa.sign(k, rng.fr(), msg)
        out.append((a, msg, r8, s))
    assert em.verify(*out[0]) == em.VALID and em.verify(*out[63]) == em.VALID
    return tuple(out)


@functools.lru_cache(maxsize=None)
def one_of_each_status():
    by = {}
    for name, a, msg, r8, s, st in ec.status_cases():
        by.setdefault(st, (a, msg, r8, s))
    return by


def arrays(sigs):
    """signatures -> ((count, 5, 4), (count, 4)) uint64"""
    points = np.stack([ints_to_limbs(em.field_row(a, msg, r8)) for a, msg, r8, _ in sigs])
    return points, scalars_to_words([s for _, _, _, s in sigs])


def to_dev(ctx, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:%d" % ctx.device)


def run(ctx, sigs, stride=None):
    """-> statuses, or (statuses, bit rows (count, stride) uint8 with one spare row) where a stride is given"""
    count = len(sigs)
    points, s = arrays(sigs)
    d_p, d_s = to_dev(ctx, points), to_dev(ctx, s)
    d_st = torch.full((count + 1,), -1, dtype=torch.int32, device=d_p.device)
    d_bits = None
    if stride:
        d_bits = torch.full((count + 1, stride), FILL, dtype=torch.uint8, device=d_p.device)
    torch.cuda.synchronize()
    ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr(), None if d_bits is None else d_bits.data_ptr(), stride or 64)
    st = d_st.cpu().numpy()
    assert st[count] == -1                                  # nothing behind the last status
    return (st[:count], d_bits.cpu().numpy()) if stride else st[:count]


# ---- a. counts, and every status at the edges of a wave and of a block ---------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_statuses_at_wave_and_block_edges(ctx, count):
    pool = valid_pool()
    lanes = sorted({j for j in EDGE_LANES + (count - 1,) if j < count})
    for st in range(1, 6):
        sigs = [pool[j % 64] for j in range(count)]
        want = [em.VALID] * count
        for j in lanes:
            sigs[j] = one_of_each_status()[st]
            want[j] = st
        got = run(ctx, sigs)
        assert [int(x) for x in got] == want, (count, st)   # a planted lane changes no neighbour's verdict


def test_the_whole_status_set_in_one_wave(ctx):
    cases = ec.status_cases()
    assert len(cases) <= 64
    pool = valid_pool()
    sigs = [c[1:5] for c in cases] + [pool[j] for j in range(64 - len(cases))]
    want = [c[5] for c in cases] + [em.VALID] * (64 - len(cases))
    assert set(want) == set(range(6))
    got = run(ctx, sigs)
    assert [int(x) for x in got] == want, [(c[0], int(g)) for c, g in zip(cases, got) if int(g) != c[5]]
    host = run_host_form(ctx, sigs)
    assert [int(x) for x in host] == want


def run_host_form(ctx, sigs):
    return ctx.eddsa_verify_batch([em.field_row(a, msg, r8) for a, msg, r8, _ in sigs], [s for _, _, _, s in sigs])


# ---- b. the bit rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [64, 72])
def test_bit_rows_against_the_model(ctx, stride):
    cases = ec.status_cases()
    sigs = [c[1:5] for c in cases] + list(valid_pool()[:70 - len(cases)])
    plain = run(ctx, sigs)
    st, bits = run(ctx, sigs, stride)
    assert np.array_equal(st, plain)                        # the call with NULL gives the same statuses
    for j, (a, msg, r8, s) in enumerate(sigs):
        want = np.frombuffer(em.bit_row(a, msg, r8, s), np.uint8)
        assert np.array_equal(bits[j, :64], want), j        # 251 bits of S, 254 of hm, 7 pad bits of zero; all zero for RANGE
        assert (bits[j, 64:] == FILL).all(), j              # bytes of a row past the 64th are not written
    assert (bits[len(sigs)] == FILL).all()
    assert any(int(x) == em.RANGE for x in st) and not bits[[j for j, x in enumerate(st) if int(x) == em.RANGE], :64].any()


# ---- c. refusals ---------------------------------------------------------------------------------------------------------------
def test_argument_refusals_and_count_zero(ctx):
    points, s = arrays(valid_pool()[:4])
    d_p, d_s = to_dev(ctx, points), to_dev(ctx, s)
    d_st = torch.full((8,), -1, dtype=torch.int32, device=d_p.device)
    d_bits = torch.full((8, 72), FILL, dtype=torch.uint8, device=d_p.device)
    torch.cuda.synchronize()
    p, sp, st, b = d_p.data_ptr(), d_s.data_ptr(), d_st.data_ptr(), d_bits.data_ptr()
    bad = [(0, sp, 4, st, None, 64), (p, 0, 4, st, None, 64), (p, sp, 4, 0, None, 64), (p + 4, sp, 4, st, None, 64), (p, sp + 4, 4, st, None, 64),
           (p, sp, 4, st + 2, None, 64), (p, sp, 4, st, b + 4, 64), (p, sp, 4, st, b, 56), (p, sp, 4, st, b, 68), (p, sp, 4, st, b, 0)]
    for args in bad:
        with pytest.raises(zk.ZkError) as err:
            ctx.eddsa_verify_batch(*args)
        assert err.value.status == _lib.ZK_ERR_ARG and "eddsa" in str(err.value), args
    ctx.eddsa_verify_batch(0, 0, 0, 0, None, 64)            # count == 0 touches nothing, null pointers included
    ctx.eddsa_verify_batch(p, sp, 0, st, b, 64)
    assert (d_st.cpu().numpy() == -1).all() and (d_bits.cpu().numpy() == FILL).all()
    ctx.eddsa_verify_batch(p, sp, 4, st, b, 72)
    assert (d_st.cpu().numpy()[:4] == 0).all() and (d_st.cpu().numpy()[4:] == -1).all()
    assert ctx.eddsa_verify_batch([], []).shape == (0,)


# ---- d. keys from the fixed-base kernel, device to device --------------------------------------------------------------------------
def test_keys_from_the_scalar_multiplication_kernel(ctx):
    rng = SplitMix64(3400)
    count = 65
    secrets = [rng.fr() % L or 1 for _ in range(count)]
    messages = [rng.fr() for _ in range(count)]
    signed = [eddsa.sign(k, rng.fr(), msg) for k, msg in zip(secrets, messages)]
    rows = np.zeros((count, 5, 4), np.uint64)               # A is left to the kernel
    rows[:, 2:4] = np.stack([ints_to_limbs(list(r8)) for r8, _ in signed])
    rows[:, 4] = ints_to_limbs(messages)
    d_rows, d_k = to_dev(ctx, rows), to_dev(ctx, scalars_to_words(secrets))
    d_s = to_dev(ctx, scalars_to_words([s for _, s in signed]))
    d_st = torch.full((count,), -1, dtype=torch.int32, device=d_rows.device)
    torch.cuda.synchronize()
    ctx.babyjub_mul_batch(d_k.data_ptr(), None, count, d_rows.data_ptr(), 20)
    ctx.eddsa_verify_batch(d_rows.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr())
    assert (d_st.cpu().numpy() == em.VALID).all()
    keys = d_rows.cpu().numpy().view(np.uint64)[:, 0:2]
    assert [tuple(zk.limbs_to_ints(k)) for k in keys[[0, 64]]] == [em.public_key(secrets[0]), em.public_key(secrets[64])]
    d_rows[7, 4, 0] ^= 1                                    # another message under signature 7
    torch.cuda.synchronize()
    ctx.eddsa_verify_batch(d_rows.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr())
    assert [int(x) for x in d_st.cpu().numpy()] == [em.MISMATCH if j == 7 else em.VALID for j in range(count)]


# ---- e. the verdict equals the circuit's satisfiability ------------------------------------------------------------------------------
CHAIN_COUNT = 65
CHAIN_EDGE_LANES = (0, 63, 64, 1, 31, 62, 2, 33)            # the eight named instances of the case, at the wave's edges first


def signature_of_row(row):
    a, r8, msg = (row[0], row[1]), (row[2], row[3]), row[4]
    s = sum(b << i for i, b in enumerate(row[5:5 + em.S_BITS]))
    return a, msg, r8, s


@pytest.fixture(scope="module")
def chain(ctx):
    """the circuit's eight named instances at the edge lanes among copies of the valid one; statuses, bits and fields from the kernel;
    the alias lane's hm bits replaced by those of hm + r; then the witnesses of Mixgen.run over what lies on the device"""
    case = ec.gadget_case()
    names = case.info["names"]
    lane_row = [names.index("valid")] * CHAIN_COUNT
    for lane, k in zip(CHAIN_EDGE_LANES, range(len(names))):
        lane_row[lane] = k
    sigs = []
    for k in lane_row:
        sigs.append(signature_of_row(case.rows[k]))         # the S + l of its row fits 251 bits
    count = CHAIN_COUNT
    points, s = arrays(sigs)
    d_p, d_s = to_dev(ctx, points), to_dev(ctx, s)
    d_st = torch.full((count,), -1, dtype=torch.int32, device=d_p.device)
    d_bits = torch.zeros((count, 64), dtype=torch.uint8, device=d_p.device)
    torch.cuda.synchronize()
    ctx.eddsa_verify_batch(d_p.data_ptr(), d_s.data_ptr(), count, d_st.data_ptr(), d_bits.data_ptr(), 64)
    status = d_st.cpu().numpy()
    canonical = d_bits.cpu().numpy().copy()
    alias_lane = CHAIN_EDGE_LANES[names.index("alias")]
    a, msg, r8, sv = sigs[alias_lane]
    row = (sv | ((em.challenge(r8, a, msg) + R) << em.S_BITS)).to_bytes(64, "little")
    d_bits[alias_lane] = torch.from_numpy(np.frombuffer(row, np.uint8).copy()).to(d_bits.device)
    torch.cuda.synchronize()
    m = case.c.m
    mg = Mixgen(ctx, case.c)
    d_w = torch.empty((count + 1, m, 4), dtype=torch.int64, device=d_p.device)
    d_w.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()
    mg.run(d_bits.data_ptr(), d_p.data_ptr(), count, d_w.data_ptr(), in_stride=64)
    mg.close()
    qap = case.c.qap_sparse_unity(ctx)
    yield dict(case=case, names=names, lane_row=lane_row, sigs=sigs, status=status, canonical=canonical, d_p=d_p, d_bits=d_bits, d_w=d_w, qap=qap,
               alias_lane=alias_lane)
    qap.close()


def test_chain_statuses_and_bits(ctx, chain):
    by_name = {"valid": em.VALID, "tampered": em.MISMATCH, "s_plus_l": em.S_RANGE, "alias_canonical": em.VALID, "alias": em.VALID,
               "order8_key": em.VALID, "identity_key": em.VALID, "r_off_curve": em.R_OFF_CURVE}
    want = [by_name[chain["names"][k]] for k in chain["lane_row"]]
    for lane in CHAIN_EDGE_LANES:
        assert em.verify(*chain["sigs"][lane]) == want[lane], lane
    assert [int(x) for x in chain["status"]] == want
    for lane in CHAIN_EDGE_LANES:
        assert bytes(chain["canonical"][lane]) == em.bit_row(*chain["sigs"][lane]), lane


def test_chain_witnesses_word_for_word_and_the_qap_check(ctx, chain):
    case, count, m = chain["case"], CHAIN_COUNT, chain["case"].c.m
    want = np.stack([ints_to_limbs(case.want(k)) for k in range(len(case.rows))])[chain["lane_row"]]
    d_w = chain["d_w"]
    got = d_w.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:count], want), np.argwhere((got[:count] != want).any(axis=2))[:3]
    assert (got[count:].view(np.uint8) == FILL).all()
    # the same inputs as field elements through the tape
    bits = np.unpackbits(chain["d_bits"].cpu().numpy(), axis=1, bitorder="little")[:, :em.S_BITS + em.HM_BITS]
    ins = np.zeros((count, 5 + bits.shape[1], 4), np.uint64)
    ins[:, :5] = chain["d_p"].cpu().numpy().view(np.uint64)
    ins[:, 5:, 0] = bits
    wg = Witgen(ctx, case.c)
    d_t = torch.empty((count, m, 4), dtype=torch.int64, device=chain["d_p"].device)
    d_in = to_dev(ctx, ins)
    torch.cuda.synchronize()
    wg.run(d_in.data_ptr(), count, d_t.data_ptr())
    wg.close()
    assert torch.equal(d_t, d_w[:count])
    # zero failing gates exactly where the status is VALID and the bits are the canonical ones
    res = ctx.qap_check_dev(chain["qap"], d_w.data_ptr(), m, count)
    satisfied = [int(x) == 0 for x in res["bad_gates"]]
    assert satisfied == [int(chain["status"][j]) == em.VALID and j != chain["alias_lane"] for j in range(count)]
    for lane, k in zip(CHAIN_EDGE_LANES, range(len(case.rows))):
        bad = case.failing[k]
        assert int(res["bad_gates"][lane]) == len(bad) and int(res["first_bad"][lane]) == (bad[0] if bad else _lib.QAP_CHECK_NONE), chain["names"][k]


def test_three_proofs_of_the_batch_verify(ctx, chain):
    case, m = chain["case"], chain["case"].c.m
    rng = SplitMix64(3500)
    crs = ctx.setup(chain["qap"], ints_to_limbs([rng.fr() for _ in range(5)]))
    names = chain["names"]
    lanes = [CHAIN_EDGE_LANES[names.index("valid")], CHAIN_EDGE_LANES[names.index("order8_key")], 40]
    assert all(int(chain["status"][j]) == em.VALID for j in lanes)
    d_w = chain["d_w"]
    rs, ss = [rng.fr() for _ in lanes], [rng.fr() for _ in lanes]
    ticket = ctx.prove_batch_submit(crs, chain["qap"], [d_w.data_ptr() + j * m * 32 for j in lanes], [m] * 3, rs, ss)
    proofs = ctx.prove_batch_wait(ticket, 3)
    public = np.stack([ints_to_limbs([chain["sigs"][j][0][0], chain["sigs"][j][0][1], chain["sigs"][j][1]]) for j in lanes])
    assert ctx.verify_batch(crs, public, proofs).all()
    other = public.copy()
    other[0, 2, 0] ^= np.uint64(1)                          # another message
    assert not ctx.verify_batch(crs, other, proofs)[0]
    crs.close()
