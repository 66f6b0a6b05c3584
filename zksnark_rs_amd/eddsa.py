"""EdDSA-Poseidon on Baby Jubjub (csrc/eddsa.hpp, csrc/eddsa.hip; include/zkgpu.h states the scheme).  A secret key is an integer
0 < k < l, a public key the point A = [k] Base8, a signature the pair (R8, S): R8 a point, S an integer below l.

    challenge(r8, a, msg)                       H6(R8.x, R8.y, A.x, A.y, M), Poseidon of width 6 (zk_eddsa_challenge); no curve check
    public_key(k), sign(k, nonce_key, msg)      host code, no context (zk_eddsa_public_key / _sign); signing is deterministic
    verify(a, msg, r8, s)                       -> a status, VALID .. MISMATCH (zk_eddsa_verify); a malformed signature is a verdict
    Context.eddsa_verify_batch(...)             one verdict per lane on the GPU, and the bit rows of the circuit (zk_eddsa_verify_batch)
    Context.eddsa_sign_batch(...)               one signature per lane on the GPU: the inputs of verify_batch and its bit rows (zk_eddsa_sign_batch)
    circuit.Builder.eddsa_verify(...)           the statement as sub-circuits (zk_builder_eddsa_verify)
"""
import ctypes as C

import numpy as np

from . import _lib, ZkError, ints_to_limbs, limbs_to_int, limbs_to_ints

VALID, RANGE, KEY_OFF_CURVE, R_OFF_CURVE, S_RANGE, MISMATCH = range(6)      # ZK_EDDSA_*
STATUS_NAMES = ("VALID", "RANGE", "KEY_OFF_CURVE", "R_OFF_CURVE", "S_RANGE", "MISMATCH")
S_BITS, HM_BITS = 251, 254


def _words(values, what):
    xs = [int(x) for x in values]
    if any(x < 0 or x >> 256 for x in xs):
        raise ZkError(_lib.ZK_ERR_RANGE, "eddsa: %s is not below 2^256" % what)
    return ints_to_limbs(xs)


def _ptr(a):
    return a.ctypes.data_as(_lib.u64p)


def _raise(rc, what):
    raise ZkError(rc, "eddsa: %s" % (what if rc == _lib.ZK_ERR_RANGE else "bad argument"))


def challenge(r8, a, msg):
    """H6(R8.x, R8.y, A.x, A.y, M) for any five field elements; ZkError(ZK_ERR_RANGE) for one >= r"""
    out = np.zeros(4, np.uint64)
    rc = _lib.load().zk_eddsa_challenge(_ptr(_words(r8, "a coordinate")), _ptr(_words(a, "a coordinate")), _ptr(_words([msg], "the message")), _ptr(out))
    if rc != 0:
        _raise(rc, "an element is not below r")
    return limbs_to_int(out)


def public_key(k):
    out = np.zeros((2, 4), np.uint64)
    rc = _lib.load().zk_eddsa_public_key(_ptr(_words([k], "the key")), _ptr(out))
    if rc != 0:
        _raise(rc, "the key is 0 or not below l")
    return tuple(limbs_to_ints(out))


def sign(k, nonce_key, msg):
    """-> ((R8.x, R8.y), S); ZkError(ZK_ERR_RANGE): k == 0, k >= l, nonce_key >= r or msg >= r"""
    r8, s = np.zeros((2, 4), np.uint64), np.zeros(4, np.uint64)
    rc = _lib.load().zk_eddsa_sign(_ptr(_words([k], "the key")), _ptr(_words([nonce_key], "the nonce key")), _ptr(_words([msg], "the message")),
                                   _ptr(r8), _ptr(s))
    if rc != 0:
        _raise(rc, "the key is 0 or not below l, or the nonce key or the message is not below r")
    return tuple(limbs_to_ints(r8)), limbs_to_int(s)


def verify(a, msg, r8, s):
    """-> VALID, RANGE, KEY_OFF_CURVE, R_OFF_CURVE, S_RANGE or MISMATCH, the lowest that applies, over any integers below 2^256"""
    status = C.c_int(-1)
    rc = _lib.load().zk_eddsa_verify(_ptr(_words(a, "a coordinate")), _ptr(_words([msg], "the message")), _ptr(_words(r8, "a coordinate")),
                                     _ptr(_words([s], "S")), C.byref(status))
    if rc != 0:
        _raise(rc, "bad argument")
    return status.value
