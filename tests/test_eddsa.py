"""-m "not gpu": EdDSA-Poseidon on the host (csrc/eddsa.hpp through zksnark_rs_amd.eddsa, the gadget of csrc/builder.hpp through
Builder.eddsa_verify) against tests/eddsa_model.py: the published H6 digest, sign byte for byte over the key, nonce and message edges,
every status on constructed inputs, the refusals, and the gadget circuit's rows, three host evaluators and failing gates."""
import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib, eddsa, poseidon
from zksnark_rs_amd.circuit import BuildErr, Builder

import babyjub_model as bm
import eddsa_cases as ec
import eddsa_model as em
import gadget_cases as gc
import poseidon_model as pm

R, L = bm.R, bm.L


def test_model_rests_on_the_published_digest_and_the_sign_verify_identity():
    assert em.h6(1, 2, 3, 4, 5) == em.H6_12345
    c, m = em.params6()
    assert len(c) == 408 and len(m) == 6 and all(len(row) == 6 for row in m)
    for k, a in ec.keys():
        r8, s = em.sign(k, 11, 12)
        assert s < L and bm.on_curve(r8) and em.verify(a, 12, r8, s) == em.VALID
        assert em.verify(a, 13, r8, s) == em.MISMATCH
    assert [n for n in em.STATUS_NAMES] == list(eddsa.STATUS_NAMES)
    assert (eddsa.VALID, eddsa.RANGE, eddsa.KEY_OFF_CURVE, eddsa.R_OFF_CURVE, eddsa.S_RANGE, eddsa.MISMATCH) == tuple(range(6))


def test_challenge_is_the_published_digest():
    assert eddsa.challenge((1, 2), (3, 4), 5) == em.H6_12345 == 0x0dab9449e4a1398a15224c0b15a49d598b2174d305a316c918125f8feeb123c0


def test_challenge_matches_the_model_and_checks_range_only():
    rng = zk.SplitMix64(3000)
    rows = [(0,) * 5, (R - 1,) * 5, (R - 1, 0, R - 1, 0, R - 1)] + [tuple(rng.fr() for _ in range(5)) for _ in range(8)]
    for a, b, c, d, e in rows:
        assert eddsa.challenge((a, b), (c, d), e) == em.h6(a, b, c, d, e)       # no point here is on the curve
    for bad in range(5):
        v = [1, 2, 3, 4, 5]
        v[bad] = R
        with pytest.raises(zk.ZkError) as err:
            eddsa.challenge(v[0:2], v[2:4], v[4])
        assert err.value.status == _lib.ZK_ERR_RANGE


def test_public_poseidon_calls_still_refuse_arity_five():
    for arity in (3, 5):
        with pytest.raises(zk.ZkError) as err:
            poseidon.hash([1] * arity)
        assert err.value.status == _lib.ZK_ERR_ARG
        with pytest.raises(zk.ZkError) as err:
            poseidon.params(arity)
        assert err.value.status == _lib.ZK_ERR_ARG
        b = Builder()
        with pytest.raises(BuildErr):
            b.poseidon([b.new_wire() for _ in range(arity)])
        assert b.dims()[1] == 0
    assert poseidon.hash([1, 2, 3, 4]) == pm.hash([1, 2, 3, 4])


def test_public_key_and_sign_are_the_models_byte_for_byte():
    rng = zk.SplitMix64(3001)
    messages = [0, 1, R - 1, rng.fr()]
    for k, a in ec.keys():
        assert eddsa.public_key(k) == a
        for msg in messages:
            for nonce_key in (0, R - 1):
                assert eddsa.sign(k, nonce_key, msg) == em.sign(k, nonce_key, msg), (k, msg, nonce_key)
    k, a = ec.keys()[3]
    r8, s = eddsa.sign(k, 5, 6)
    assert eddsa.sign(k, 5, 6) == (r8, s)                                       # deterministic
    assert eddsa.verify(a, 6, r8, s) == eddsa.VALID


def test_sign_and_public_key_refusals():
    for k in (0, L, L + 1, R, (1 << 256) - 1):
        with pytest.raises(zk.ZkError) as err:
            eddsa.sign(k, 1, 1)
        assert err.value.status == _lib.ZK_ERR_RANGE
        with pytest.raises(zk.ZkError) as err:
            eddsa.public_key(k)
        assert err.value.status == _lib.ZK_ERR_RANGE
    for nonce_key, msg in ((R, 1), (1, R), ((1 << 256) - 1, 1)):
        with pytest.raises(zk.ZkError) as err:
            eddsa.sign(1, nonce_key, msg)
        assert err.value.status == _lib.ZK_ERR_RANGE
    lib = _lib.load()
    one = zk.ints_to_limbs([1]).ctypes.data_as(_lib.u64p)
    out = np.zeros(8, np.uint64)
    assert lib.zk_eddsa_sign(one, one, one, None, out.ctypes.data_as(_lib.u64p)) == _lib.ZK_ERR_ARG
    assert lib.zk_eddsa_public_key(None, out.ctypes.data_as(_lib.u64p)) == _lib.ZK_ERR_ARG
    assert lib.zk_eddsa_verify(one, one, one, one, None) == _lib.ZK_ERR_ARG
    assert lib.zk_eddsa_challenge(one, one, None, out.ctypes.data_as(_lib.u64p)) == _lib.ZK_ERR_ARG


@pytest.mark.parametrize("index", range(len(ec.status_cases())), ids=[c[0] for c in ec.status_cases()])
def test_verify_status(index):
    name, a, msg, r8, s, want = ec.status_cases()[index]
    assert eddsa.verify(a, msg, r8, s) == want, name


def test_status_cases_cover_what_they_claim():
    by_name = {c[0]: c for c in ec.status_cases()}
    a, msg, r8, s = ec.base()
    assert s + L < R and by_name["s_plus_l"][5] == em.S_RANGE
    assert bm.mul(s + L) == bm.mul(s)                                           # S + L satisfies the equation and is refused all the same
    assert by_name["identity_key_0"][5] == by_name["identity_key_1"][5] == em.VALID
    for n in ("order2", "order4", "order8"):
        assert by_name[n + "_valid"][5] == em.VALID and by_name[n + "_mismatch"][5] == em.MISMATCH
    flips = [c for c in ec.status_cases() if c[0].startswith("flip_")]
    assert len(flips) == 18 and all(c[5] != em.VALID for c in flips) and any(c[5] == em.MISMATCH for c in flips)


# ---- the gadget ---------------------------------------------------------------------------------------
def test_gadget_rows_and_split():
    case = ec.gadget_case()
    gc.check_rows(case.c, case.f)
    assert case.info["gates"] == em.eddsa_gates() == 73384
    d = case.c.mixed_dims()
    assert d["n_bit_inputs"] == em.S_BITS + em.HM_BITS and d["n_field_inputs"] == 5
    # both comparators run in the boolean core: every gate of theirs but the two pinning assertions, which compute nothing
    assert d["core_ops"] == em.compare_less_gates(em.S_BITS) + em.compare_less_gates(em.HM_BITS)


@pytest.mark.parametrize("index", range(8))
def test_gadget_witness_and_failing_gates(index):
    case = ec.gadget_case()
    assert len(case.rows) == 8
    gc.check_witness(case.c, case.f, case.rows[index], want=case.want(index), failing=case.failing[index])


def test_gadget_refusals_emit_nothing():
    b = Builder()
    f = [b.new_wire() for _ in range(5)]
    s_bits, hm_bits = b.new_bits(em.S_BITS), b.new_bits(em.HM_BITS)
    with pytest.raises(BuildErr):
        b.eddsa_verify(f[0:2], f[2:4], f[4], s_bits[:-1], hm_bits)
    with pytest.raises(BuildErr):
        b.eddsa_verify(f[0:2], f[2:4], f[4], s_bits, hm_bits[:-1] + [1 << 30])
    with pytest.raises(BuildErr):
        b.eddsa_verify(f[0:2], f[2:4], 1 << 30, s_bits, hm_bits)
    assert b.dims()[1] == 0
