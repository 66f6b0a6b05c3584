"""Baby Jubjub (csrc/babyjub.hpp, csrc/babyjub.hip): the twisted Edwards curve a x^2 + y^2 = 1 + d x^2 y^2 over the BN254 scalar field,
a = 168700, d = 168696 -- circomlib's, iden3's and Semaphore's curve.  A point is a pair of integers (x, y); the identity is (0, 1).

    params(), on_curve(p), add(p, q), mul(k, p=None)   host code, no context (zk_babyjub_params / _on_curve / _add / _mul)
    Context.babyjub_mul_batch(...)                     one scalar multiplication per lane on the GPU (zk_babyjub_mul_batch)
    circuit.Builder.babyjub_*                          the curve as sub-circuits: assert_on_curve, add, mul_fixed, mul, affine
"""
import numpy as np

from . import _lib, ZkError, ints_to_limbs, limbs_to_int, limbs_to_ints

FIXED_WINDOW = 4          # ZK_BABYJUB_FIXED_WINDOW: bits a window of the fixed-base kernel's table
VAR_WINDOW = 2            # ZK_BABYJUB_VAR_WINDOW: bits a window of the variable-base kernel


def _point(p):
    xs = [int(p[0]), int(p[1])]
    if any(x < 0 or x >> 256 for x in xs):
        raise ZkError(_lib.ZK_ERR_RANGE, "babyjub: a coordinate is not below r")
    return ints_to_limbs(xs)


def _raise(rc):
    raise ZkError(rc, "babyjub: a coordinate is not below r, or the point is not on the curve" if rc == _lib.ZK_ERR_RANGE else "babyjub: bad argument")


def params():
    """dict(a, d, order: l, base8: (x, y), generator: (x, y)) as integers"""
    lib = _lib.load()
    a, d, order = (np.zeros(4, np.uint64) for _ in range(3))
    b8, g = np.zeros((2, 4), np.uint64), np.zeros((2, 4), np.uint64)
    lib.zk_babyjub_params(*(x.ctypes.data_as(_lib.u64p) for x in (a, d, order, b8, g)))
    return dict(a=limbs_to_int(a), d=limbs_to_int(d), order=limbs_to_int(order), base8=tuple(limbs_to_ints(b8)), generator=tuple(limbs_to_ints(g)))


def on_curve(p):
    """True / False; ZkError(ZK_ERR_RANGE) for a coordinate >= r"""
    rc = _lib.load().zk_babyjub_on_curve(_point(p).ctypes.data_as(_lib.u64p))
    if rc < 0:
        _raise(rc)
    return bool(rc)


def add(p, q):
    a, b, out = _point(p), _point(q), np.zeros((2, 4), np.uint64)
    rc = _lib.load().zk_babyjub_add(a.ctypes.data_as(_lib.u64p), b.ctypes.data_as(_lib.u64p), out.ctypes.data_as(_lib.u64p))
    if rc != 0:
        _raise(rc)
    return tuple(limbs_to_ints(out))


def mul(k, p=None):
    """[k] p for an integer 0 <= k < 2^256, taken as an integer and not reduced; p None: Base8"""
    k = int(k)
    if k < 0 or k >> 256:
        raise ZkError(_lib.ZK_ERR_RANGE, "babyjub: the scalar is not below 2^256")
    s = np.array([(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)
    a = None if p is None else _point(p)
    out = np.zeros((2, 4), np.uint64)
    rc = _lib.load().zk_babyjub_mul(s.ctypes.data_as(_lib.u64p), None if a is None else a.ctypes.data_as(_lib.u64p), out.ctypes.data_as(_lib.u64p))
    if rc != 0:
        _raise(rc)
    return tuple(limbs_to_ints(out))


def scalars_to_words(scalars):
    """integers below 2^256 -> (count, 4) uint64, the layout of zk_babyjub_mul_batch's d_scalars"""
    return np.array([[(int(k) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for k in scalars], np.uint64).reshape(-1, 4)
