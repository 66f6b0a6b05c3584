"""zksnark_rs_amd -- MI355X-native Groth16 prover (hot path of republicprotocol/zksnark-rs).

Python host-side binding over the C ABI (include/zkgpu.h -> libzkgpu.so).  All compute is in the
HIP kernels; this package only marshals numpy buffers / device pointers.  Element conventions are
those of the C ABI: Fr/Fq = 4 little-endian uint64 limbs (canonical integers), G1 affine = 8
limbs, G2 affine = 16 limbs, infinity = all zero.

  ctx  = Context()                                   # one HIP device
  qap  = ctx.qap_sparse(log_n, m, l, u, v, w)        # QAP::from(root_rep) on roots w^j
  crs  = ctx.setup(qap, trapdoor)                    # groth16::setup      (mod.rs:134)
  pf   = ctx.prove(crs, qap, weights, r, s)          # groth16::prove      (mod.rs:213) -> 259 bytes

`zksnark_rs_amd.groth16` mirrors the reference's function names and argument order.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import PROOF_BYTES, PROOF_COMPRESSED_BYTES, PARTIAL_BYTES, MAX_IN_FLIGHT, MAX_BATCH

R_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q_MODULUS = 21888242871839275222246405745257275088696311157297823662689037894645226208583

__all__ = ["Context", "ZkError", "fr_to_limbs", "limbs_to_int", "ints_to_limbs", "limbs_to_ints",
           "PROOF_BYTES", "PARTIAL_BYTES", "MAX_IN_FLIGHT", "MAX_BATCH", "R_MODULUS", "Q_MODULUS", "SplitMix64", "pairing", "proof_save", "proof_load",
           "PROOF_COMPRESSED_BYTES", "proof_compress", "proof_decompress", "VerifyingKey", "CrsCheck",
           "Powers", "PowersCheck", "PowersContribution", "PowersContributionCheck", "powers_contribution_prove", "powers_role_tag"]


class ZkError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _lib.load().zk_strerror(status).decode()
        super().__init__("zkgpu status %d (%s)%s" % (status, msg, ": " + detail if detail else ""))


# ---- limb helpers ---------------------------------------------------------------------------
def fr_to_limbs(x):
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def ints_to_limbs(xs, words=4):
    """list of ints (or nested tuples flattened by the caller) -> (len, words) uint64 array"""
    out = np.empty((len(xs), words), dtype=np.uint64)
    mask = 0xFFFFFFFFFFFFFFFF
    for i, x in enumerate(xs):
        for k in range(words):
            out[i, k] = (x >> (64 * k)) & mask
    return out


def limbs_to_int(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1)
    return sum(int(v) << (64 * i) for i, v in enumerate(a))


def limbs_to_ints(a, words=4):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, words)
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in a]


class SplitMix64:
    """Deterministic stream shared by tests, bench and the oracle (seeded synthetic inputs)."""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def fr(self):
        while True:
            l = [self.next() for _ in range(4)]
            l[3] &= (1 << 62) - 1
            v = l[0] | (l[1] << 64) | (l[2] << 128) | (l[3] << 192)
            if 0 < v < R_MODULUS:
                return v


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(_lib.u64p)


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(_lib.u32p)


def pairing(g1, g2):
    """EllipticEncryptable::pairing (fr.rs:120-122) on the host: (8,) and (16,) limb arrays -> 12 Fq ints."""
    lib = _lib.load()
    a, ap = _u64(np.asarray(g1).reshape(8))
    b, bp = _u64(np.asarray(g2).reshape(16))
    out = np.zeros(48, dtype=np.uint64)
    rc = lib.zk_pairing(ap, bp, out.ctypes.data_as(_lib.u64p))
    if rc != 0:
        raise ZkError(rc)
    return limbs_to_ints(out)


def proof_save(proof, path):
    """zk_proof_save: versioned proof file ("ZKPRFv1" | 259 canonical bytes | checksum)."""
    buf = (C.c_uint8 * PROOF_BYTES).from_buffer_copy(proof)
    rc = _lib.load().zk_proof_save(buf, str(path).encode())
    if rc != 0:
        raise ZkError(rc)


def proof_load(path):
    buf = (C.c_uint8 * PROOF_BYTES)()
    rc = _lib.load().zk_proof_load(str(path).encode(), buf)
    if rc != 0:
        raise ZkError(rc)
    return bytes(buf)


def proof_compress(proof):
    """zk_proof_compress (host code): the 259-byte proof -> its 128-byte compressed form.  ZkError(ZK_ERR_RANGE) unless every
    block has a legal tag, coordinates < q and lies on its curve (the subgroup of B is not tested here)."""
    if len(proof) != PROOF_BYTES:
        raise ValueError("proof_compress: a proof is %d bytes" % PROOF_BYTES)
    src = (C.c_uint8 * PROOF_BYTES).from_buffer_copy(bytes(proof))
    dst = (C.c_uint8 * PROOF_COMPRESSED_BYTES)()
    rc = _lib.load().zk_proof_compress(src, dst)
    if rc != 0:
        raise ZkError(rc, "proof_compress: not a canonical proof encoding")
    return bytes(dst)


def proof_decompress(compressed):
    """zk_proof_decompress (host code): 128 bytes -> the 259-byte proof.  ZkError(ZK_ERR_RANGE) unless all three blocks are
    valid encodings of points on their curves."""
    if len(compressed) != PROOF_COMPRESSED_BYTES:
        raise ValueError("proof_decompress: a compressed proof is %d bytes" % PROOF_COMPRESSED_BYTES)
    src = (C.c_uint8 * PROOF_COMPRESSED_BYTES).from_buffer_copy(bytes(compressed))
    dst = (C.c_uint8 * PROOF_BYTES)()
    rc = _lib.load().zk_proof_decompress(src, dst)
    if rc != 0:
        raise ZkError(rc, "proof_decompress: not a valid compressed proof")
    return bytes(dst)


class _Handle:
    def __init__(self, ctx, ptr, free):
        self.ctx, self.ptr, self._free = ctx, ptr, free

    def close(self):
        if self.ptr:
            self._free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Qap(_Handle):
    """Device-resident QAP<CoefficientPoly<FrLocal>> (groth16/mod.rs:60-67)."""
    n = m = input = 0
    dense = False


class Crs(_Handle):
    """Device-resident (SigmaG1, SigmaG2) (groth16/mod.rs:105-121)."""
    n = m = input = 0


class CrsCheck:
    """What zk_crs_check found: `failed` = the ZK_CRS_CHECK_* bits of the relations that do not hold, `flags` = T_ZERO |
    LAGRANGE_PRESENT.  The bit values are class attributes (CrsCheck.WIRES, ...); `names` lists the failed ones; `ok` is "the CRS is
    good": no relation fails and x is not a root of t."""
    T_ZERO = _lib.CRS_CHECK_T_ZERO
    LAGRANGE_PRESENT = _lib.CRS_CHECK_LAGRANGE_PRESENT

    def __init__(self, failed, flags):
        self.failed, self.flags = int(failed), int(flags)

    @property
    def ok(self):
        return self.failed == 0 and not (self.flags & self.T_ZERO)

    @property
    def t_zero(self):
        return bool(self.flags & self.T_ZERO)

    @property
    def lagrange_present(self):
        return bool(self.flags & self.LAGRANGE_PRESENT)

    @property
    def names(self):
        return [n for k, n in enumerate(_lib.CRS_CHECK_BITS) if self.failed >> k & 1]

    def __repr__(self):
        return "CrsCheck(failed=%s, t_zero=%s, lagrange_present=%s)" % ("|".join(self.names) or "0", self.t_zero, self.lagrange_present)


for _k, _n in enumerate(_lib.CRS_CHECK_BITS):
    setattr(CrsCheck, _n, 1 << _k)


def _tag_arg(tag):
    """a 32-byte tag as the u8 pointer the ABI takes (None = 32 zero bytes inside the library)"""
    if tag is None:
        return None, None
    t = np.frombuffer(bytes(tag), dtype=np.uint8).copy()
    if t.size != 32:
        raise ValueError("the tag is 32 bytes")
    return t, t.ctypes.data_as(_lib.u8p)


def _fr_arg(x):
    """None, an int or (4,) limbs -> (array kept alive, u64 pointer or None)"""
    if x is None:
        return None, None
    return _u64(fr_to_limbs(x) if isinstance(x, int) else np.asarray(x).reshape(4))


class Contribution:
    """The record of a delta contribution (zk_crs_contribution): delta_g1 before and after, and a Schnorr proof of knowledge of the
    factor bound to a 32-byte tag.  to_bytes / from_bytes: its 224-byte memory image (little-endian words)."""

    def __init__(self, raw=None):
        self.raw = raw if raw is not None else _lib.CrsContribution()

    def to_bytes(self):
        return bytes(bytearray(self.raw))

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if len(data) != _lib.CONTRIBUTION_BYTES:
            raise ValueError("a contribution record is %d bytes" % _lib.CONTRIBUTION_BYTES)
        return cls(_lib.CrsContribution.from_buffer_copy(data))

    def _words(self, name):
        return np.array(list(getattr(self.raw, name)), dtype=np.uint64)

    delta_before_g1 = property(lambda self: self._words("delta_before_g1"))
    delta_after_g1 = property(lambda self: self._words("delta_after_g1"))
    commit_g1 = property(lambda self: self._words("commit_g1"))
    response = property(lambda self: limbs_to_int(self._words("response")))

    def verify(self, tag=None):
        """zk_crs_contribution_verify (host code): does the record prove knowledge of d with delta_after = d delta_before for `tag`?"""
        t, tp = _tag_arg(tag)
        ok = C.c_int(0)
        rc = _lib.load().zk_crs_contribution_verify(C.byref(self.raw), tp, C.byref(ok))
        if rc != 0:
            raise ZkError(rc)
        return bool(ok.value)

    def __eq__(self, other):
        return isinstance(other, Contribution) and self.to_bytes() == other.to_bytes()


def contribution_prove(delta_before_g1, d, nonce=None, tag=None):
    """zk_crs_contribution_prove (host code, no Context): the record for delta_after = d delta_before.  nonce: None = drawn from the
    OS; a fixed one is for tests only."""
    b, bp = _u64(np.asarray(delta_before_g1).reshape(8))
    d_, dp = _fr_arg(d)
    k_, kp = _fr_arg(nonce)
    t, tp = _tag_arg(tag)
    out = Contribution()
    rc = _lib.load().zk_crs_contribution_prove(bp, dp, kp, tp, C.byref(out.raw))
    if rc != 0:
        raise ZkError(rc)
    return out


class ContributionCheck:
    """What zk_crs_contribution_check found: `failed` = the ZK_CONTRIB_* bits of the relations that do not hold (class attributes
    ContributionCheck.SUM_DELTA, ...); `names` lists them; `ok`: `after` is a valid successor of `before`."""

    def __init__(self, failed, flags=0):
        self.failed, self.flags = int(failed), int(flags)

    @property
    def ok(self):
        return self.failed == 0

    @property
    def names(self):
        return [n for k, n in enumerate(_lib.CONTRIB_BITS) if self.failed >> k & 1]

    def __repr__(self):
        return "ContributionCheck(failed=%s)" % ("|".join(self.names) or "0")


for _k, _n in enumerate(_lib.CONTRIB_BITS):
    setattr(ContributionCheck, _n, 1 << _k)


class Powers(_Handle):
    """Device-resident powers-of-tau transcript (zk_powers): tau_g1 (n_tau_g1 points), tau_g2, alpha_tau_g1, beta_tau_g1 (n_rest points
    each) and beta_g2.  Context.powers_download(handle) gives the arrays as a dict of canonical affine limbs."""
    n_tau_g1 = n_rest = 0


class PowersCheck:
    """What zk_powers_check / zk_powers_contribution_check found: `failed` = the ZK_POWERS_CHECK_* bits of the relations that do not
    hold (class attributes PowersCheck.POWERS_G1, ...); `names` lists them; `ok`: none."""

    def __init__(self, failed, flags=0):
        self.failed, self.flags = int(failed), int(flags)

    @property
    def ok(self):
        return self.failed == 0

    @property
    def names(self):
        return [n for k, n in enumerate(_lib.POWERS_CHECK_BITS) if n and self.failed >> k & 1]

    def __repr__(self):
        return "%s(failed=%s)" % (type(self).__name__, "|".join(self.names) or "0")


class PowersContributionCheck(PowersCheck):
    """zk_powers_contribution_check's answer: PowersCheck's bits for `after`, and RECORD / KNOWLEDGE for the record."""


for _k, _n in enumerate(_lib.POWERS_CHECK_BITS):
    if _n:
        setattr(PowersCheck, _n, 1 << _k)


def _secrets_arg(values, what):
    """None or three scalars (ints or (4,) limbs) -> (array kept alive, u64 pointer or None)"""
    if values is None:
        return None, None
    if len(values) != 3:
        raise ValueError("%s: three scalars" % what)
    return _u64(np.stack([fr_to_limbs(v) if isinstance(v, int) else np.asarray(v, np.uint64).reshape(4) for v in values]))


class PowersContribution:
    """The record of a powers-of-tau contribution (zk_powers_contribution): three Contribution records -- .tau (knowledge of s on
    tau_g1[1]), .alpha (a on alpha_tau_g1[0]), .beta (b on beta_tau_g1[0]) -- each bound to its role and the caller's tag.
    to_bytes / from_bytes: the 672-byte memory image."""

    def __init__(self, raw=None):
        self.raw = raw if raw is not None else _lib.PowersContribution()

    def to_bytes(self):
        return bytes(bytearray(self.raw))

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if len(data) != 3 * _lib.CONTRIBUTION_BYTES:
            raise ValueError("a powers contribution record is %d bytes" % (3 * _lib.CONTRIBUTION_BYTES))
        return cls(_lib.PowersContribution.from_buffer_copy(data))

    tau = property(lambda self: Contribution.from_bytes(bytes(bytearray(self.raw.tau))))
    alpha = property(lambda self: Contribution.from_bytes(bytes(bytearray(self.raw.alpha))))
    beta = property(lambda self: Contribution.from_bytes(bytes(bytearray(self.raw.beta))))

    def verify(self, tag=None):
        """zk_powers_contribution_verify (host code): do all three parts verify under their role tags for `tag`?"""
        t, tp = _tag_arg(tag)
        ok = C.c_int(0)
        rc = _lib.load().zk_powers_contribution_verify(C.byref(self.raw), tp, C.byref(ok))
        if rc != 0:
            raise ZkError(rc)
        return bool(ok.value)

    def __eq__(self, other):
        return isinstance(other, PowersContribution) and self.to_bytes() == other.to_bytes()


def powers_role_tag(role, tag=None):
    """SHA-256("ZKPOWv1\\0" | role byte | tag): the tag a part of a PowersContribution is bound to (role 1 tau, 2 alpha, 3 beta)"""
    import hashlib
    return hashlib.sha256(b"ZKPOWv1\0" + bytes([role]) + (bytes(tag) if tag is not None else bytes(32))).digest()


def powers_contribution_prove(before, secrets, nonces=None, tag=None):
    """zk_powers_contribution_prove (host code, no Context).  before: the three before-points tau_g1[1], alpha_tau_g1[0],
    beta_tau_g1[0] as (3, 8) limbs; secrets: (s, a, b); nonces: None = drawn from the OS, three fixed ones are for tests only."""
    b, bp = _u64(np.asarray(before).reshape(24))
    s_, sp = _secrets_arg(secrets, "secrets")
    k_, kp = _secrets_arg(nonces, "nonces")
    t, tp = _tag_arg(tag)
    out = PowersContribution()
    rc = _lib.load().zk_powers_contribution_prove(bp, sp, kp, tp, C.byref(out.raw))
    if rc != 0:
        raise ZkError(rc)
    return out


class Context:
    def __init__(self, device=0):
        self.lib = _lib.load()
        p = C.c_void_p()
        rc = self.lib.zk_ctx_create(device, C.byref(p))
        if rc != 0:
            raise ZkError(rc)
        self.ptr = p
        self.device = device

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_ctx_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZkError(rc, self.lib.zk_last_error(self.ptr).decode())

    def set_option(self, key, value):
        self._check(self.lib.zk_set_option(self.ptr, key.encode(), int(value)))

    def get_option(self, key):
        """Value of an option, -1 for a key this build does not know ("measure_build": 1 in a ZK_MEASURE build of the library)."""
        return int(self.lib.zk_get_option(self.ptr, key.encode()))

    # ---- building blocks ----
    def ntt_fr(self, data, inverse=False, coset=False):
        """field::dft / field::idft (field/mod.rs:508-537) on a (2^k, 4) uint64 array; returns a new array."""
        a = np.array(data, dtype=np.uint64, order="C").reshape(-1, 4)
        n = a.shape[0]
        log_n = n.bit_length() - 1
        if n == 0 or (1 << log_n) != n:
            raise ValueError("length must be a power of two")
        self._check(self.lib.zk_ntt_fr(self.ptr, a.ctypes.data_as(_lib.u64p), log_n, int(inverse), int(coset)))
        return a

    def interpolate_fr(self, roots, values):
        """coefficients of the polynomial of degree < n through (roots[k], values[k]) -- zk_interpolate_fr"""
        r = np.ascontiguousarray(np.asarray(roots, dtype=np.uint64).reshape(-1, 4))
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, 4))
        if r.shape != v.shape:
            raise ValueError("roots and values differ in length")
        out = np.zeros_like(r)
        self._check(self.lib.zk_interpolate_fr(self.ptr, r.ctypes.data_as(_lib.u64p), v.ctypes.data_as(_lib.u64p), r.shape[0], out.ctypes.data_as(_lib.u64p)))
        return out

    def _msm(self, fn, words, points, scalars, window_bits):
        p, pp = _u64(np.asarray(points).reshape(-1, words))
        s, sp = _u64(np.asarray(scalars).reshape(-1, 4))
        if p.shape[0] != s.shape[0]:
            raise ValueError("points / scalars length mismatch")
        out = np.zeros(words, dtype=np.uint64)
        self._check(fn(self.ptr, pp, sp, p.shape[0], int(window_bits), out.ctypes.data_as(_lib.u64p)))
        return out

    def msm_g1(self, points, scalars, window_bits=0):
        return self._msm(self.lib.zk_msm_g1, 8, points, scalars, window_bits)

    def msm_g2(self, points, scalars, window_bits=0):
        return self._msm(self.lib.zk_msm_g2, 16, points, scalars, window_bits)

    def _batch(self, fn, op, a, b):
        a, ap = _u64(np.asarray(a).reshape(-1, 4))
        if b is None:
            b, bp = a, ap
        else:
            b, bp = _u64(np.asarray(b).reshape(-1, 4))
        out = np.zeros_like(a)
        self._check(fn(self.ptr, op, ap, bp, out.ctypes.data_as(_lib.u64p), a.shape[0]))
        return out

    def fr_batch(self, op, a, b=None):
        return self._batch(self.lib.zk_fr_batch, {"add": 0, "sub": 1, "mul": 2, "inv": 3, "inv_euclid": 4, "inv_divsteps": 5}[op], a, b)

    def fq_batch(self, op, a, b=None):
        return self._batch(self.lib.zk_fq_batch, {"add": 0, "sub": 1, "mul": 2, "inv": 3, "inv_euclid": 4, "inv_divsteps": 5}[op], a, b)

    def _pt2(self, fn, words, a, b, bwords):
        a, ap = _u64(np.asarray(a).reshape(-1, words))
        b, bp = _u64(np.asarray(b).reshape(-1, bwords))
        out = np.zeros_like(a)
        self._check(fn(self.ptr, ap, bp, out.ctypes.data_as(_lib.u64p), a.shape[0]))
        return out

    def g1_mul_batch(self, points, scalars):
        return self._pt2(self.lib.zk_g1_mul_batch, 8, points, scalars, 4)

    def g2_mul_batch(self, points, scalars):
        return self._pt2(self.lib.zk_g2_mul_batch, 16, points, scalars, 4)

    def g1_mul_each(self, points, scalars):
        """zk_g1_mul_each: out[i] = scalars[i] points[i] through k_mul_each, the kernel of powers_contribute (option "powers_mul_form")"""
        return self._pt2(self.lib.zk_g1_mul_each, 8, points, scalars, 4)

    def g2_mul_each(self, points, scalars):
        return self._pt2(self.lib.zk_g2_mul_each, 16, points, scalars, 4)

    def g1_scale_batch(self, points, scalar):
        """zk_g1_scale_batch: every point times ONE scalar (an int or (4,) limbs) -> (n, 8) array."""
        a, ap = _u64(np.asarray(points).reshape(-1, 8))
        k_, kp = _fr_arg(scalar)
        out = np.zeros_like(a)
        self._check(self.lib.zk_g1_scale_batch(self.ptr, ap, kp, out.ctypes.data_as(_lib.u64p), a.shape[0]))
        return out

    def g1_add_batch(self, a, b):
        return self._pt2(self.lib.zk_g1_add_batch, 8, a, b, 8)

    def g2_add_batch(self, a, b):
        return self._pt2(self.lib.zk_g2_add_batch, 16, a, b, 16)

    # ---- QAP ----
    @staticmethod
    def _rows(rows, keep):
        ptr, gate, val = rows
        ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        gate = np.ascontiguousarray(gate, dtype=np.uint32)
        val = np.ascontiguousarray(np.asarray(val, dtype=np.uint64).reshape(-1, 4))
        keep += [ptr, gate, val]
        return _lib.SparseRows(ptr.ctypes.data_as(_lib.u64p), gate.ctypes.data_as(_lib.u32p), val.ctypes.data_as(_lib.u64p))

    @staticmethod
    def sparse_desc(log_n, m, input, u, v, w):
        keep = []
        d = _lib.QapSparseDesc(log_n, m, input, Context._rows(u, keep), Context._rows(v, keep), Context._rows(w, keep))
        d._keep = keep
        return d

    def qap_sparse(self, log_n, m, input, u, v, w):
        """u, v, w: (ptr[m+1], gate[nnz], val[nnz,4]) rows by wire (RootRepresentation, circuit/mod.rs:201)."""
        d = self.sparse_desc(log_n, m, input, u, v, w)
        p = C.c_void_p()
        self._check(self.lib.zk_qap_upload_sparse(self.ptr, C.byref(d), C.byref(p)))
        q = Qap(self, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense, q.log_n = 1 << log_n, m, input, False, log_n
        return q

    def qap_sparse_integers(self, n, m, input, u, v, w):
        """Rows as in qap_sparse, over the roots 1..n that ASTParser emits (circuit/mod.rs:517); any n <= 2^21."""
        d = self.sparse_desc(0, m, input, u, v, w)
        p = C.c_void_p()
        self._check(self.lib.zk_qap_upload_sparse_integers(self.ptr, C.byref(d), n, C.byref(p)))
        q = Qap(self, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense, q.roots = n, m, input, False, "integers"
        return q

    def qap_sparse_roots(self, roots, m, input, u, v, w):
        """Rows as in qap_sparse over ANY distinct roots (RootRepresentation::roots(), circuit/mod.rs:201-214): gate j = roots[j] ((n, 4) limbs)."""
        r = np.ascontiguousarray(np.asarray(roots, dtype=np.uint64).reshape(-1, 4))
        n = r.shape[0]
        d = self.sparse_desc(0, m, input, u, v, w)
        p = C.c_void_p()
        self._check(self.lib.zk_qap_upload_sparse_roots(self.ptr, C.byref(d), r.ctypes.data_as(_lib.u64p), n, C.byref(p)))
        q = Qap(self, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense, q.roots = n, m, input, False, "arbitrary"
        return q

    def qap_dense(self, u, v, w, t, input):
        """u, v, w: (m, n, 4) coefficient matrices, t: (n+1, 4)."""
        u, up = _u64(u); v, vp = _u64(v); w, wp = _u64(w); t, tp = _u64(t)
        m, n = u.shape[0], u.shape[1]
        p = C.c_void_p()
        self._check(self.lib.zk_qap_upload_dense(self.ptr, up, vp, wp, tp, m, n, input, C.byref(p)))
        q = Qap(self, p, self.lib.zk_qap_free)
        q.n, q.m, q.input, q.dense = n, m, input, True
        return q

    # ---- CRS ----
    def setup(self, qap, trapdoor):
        """groth16::setup (mod.rs:134-197) with (alpha, beta, gamma, delta, x) injected: (5,4) limbs or 5 ints."""
        if not isinstance(trapdoor, np.ndarray):
            trapdoor = ints_to_limbs(list(trapdoor))
        td, tp = _u64(trapdoor.reshape(5, 4))
        p = C.c_void_p()
        self._check(self.lib.zk_setup(self.ptr, qap.ptr, tp, C.byref(p)))
        c = Crs(self, p, self.lib.zk_crs_free)
        c.n, c.m, c.input = qap.n, qap.m, qap.input
        return c

    @staticmethod
    def crs_arrays(n, m, input):
        return dict(alpha_g1=np.zeros(8, np.uint64), beta_g1=np.zeros(8, np.uint64), delta_g1=np.zeros(8, np.uint64),
                    xi_g1=np.zeros((n, 8), np.uint64), sum_gamma_g1=np.zeros((input + 1, 8), np.uint64),
                    sum_delta_g1=np.zeros((max(m - input - 1, 0), 8), np.uint64), xi_t_g1=np.zeros((max(n - 1, 0), 8), np.uint64),
                    beta_g2=np.zeros(16, np.uint64), gamma_g2=np.zeros(16, np.uint64), delta_g2=np.zeros(16, np.uint64),
                    xi_g2=np.zeros((n, 16), np.uint64))

    def crs_download(self, crs):
        arrs = self.crs_arrays(crs.n, crs.m, crs.input)
        out = _lib.CrsOut(**{k: v.ctypes.data_as(_lib.u64p) for k, v in arrs.items()})
        self._check(self.lib.zk_crs_download(self.ptr, crs.ptr, C.byref(out)))
        return arrs

    @staticmethod
    def crs_desc(n, m, input, arrs):
        keep = {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in arrs.items()}
        d = _lib.CrsDesc(n, m, input, **{k: v.ctypes.data_as(_lib.u64p) for k, v in keep.items()})
        d._keep = keep
        return d

    def crs_upload(self, n, m, input, arrs):
        d = self.crs_desc(n, m, input, arrs)
        p = C.c_void_p()
        self._check(self.lib.zk_crs_upload(self.ptr, C.byref(d), C.byref(p)))
        c = Crs(self, p, self.lib.zk_crs_free)
        c.n, c.m, c.input = n, m, input
        return c

    def crs_check(self, crs, qap, challenge=None):
        """zk_crs_check: is `crs` a Groth16 CRS of some trapdoor for `qap`?  -> CrsCheck (.ok, .failed, .flags, .names).  challenge:
        None draws it from the OS inside the library (the only sound choice: whoever made the CRS must not be able to predict it); an
        int in [1, r) or (4,) limbs fixes it, for tests."""
        if challenge is None:
            sp = None
        else:
            s_, sp = _u64(fr_to_limbs(challenge) if isinstance(challenge, int) else np.asarray(challenge).reshape(4))
        out = _lib.CrsCheckResult(0xFFFFFFFF, 0xFFFFFFFF)
        self._check(self.lib.zk_crs_check(self.ptr, crs.ptr, qap.ptr, sp, C.byref(out)))
        return CrsCheck(out.failed, out.flags)

    def crs_contribute(self, crs, d=None, tag=None):
        """zk_crs_contribute: a new CRS whose delta is d times `crs`'s -- byte-equal to setup's for (alpha, beta, gamma, delta d, x) --
        and the record that proves knowledge of d for `tag` (32 bytes, None = zeros).  d: None draws it from the OS inside the library
        (it is wiped and never returned); an int in [1, r) or (4,) limbs fixes it.  -> (Crs, Contribution)"""
        d_, dp = _fr_arg(d)
        t, tp = _tag_arg(tag)
        p = C.c_void_p()
        rec = Contribution()
        self._check(self.lib.zk_crs_contribute(self.ptr, crs.ptr, dp, tp, C.byref(p), C.byref(rec.raw)))
        c = Crs(self, p, self.lib.zk_crs_free)
        c.n, c.m, c.input = crs.n, crs.m, crs.input
        return c, rec

    def crs_contribution_check(self, before, after, contribution, tag=None, challenge=None):
        """zk_crs_contribution_check: is `after` the CRS `before` with only delta re-keyed by whoever made `contribution` for `tag`?
        -> ContributionCheck (.ok, .failed, .names).  challenge: None draws it from the OS (the only sound choice); an int in [1, r)
        or (4,) limbs fixes it, for tests."""
        s_, sp = _fr_arg(challenge)
        t, tp = _tag_arg(tag)
        out = _lib.CrsContributionResult(0xFFFFFFFF, 0xFFFFFFFF)
        self._check(self.lib.zk_crs_contribution_check(self.ptr, before.ptr, after.ptr, C.byref(contribution.raw), tp, sp, C.byref(out)))
        return ContributionCheck(out.failed, out.flags)

    # ---- powers of tau (phase 1) ----
    def _powers(self, p):
        h = Powers(self, p, self.lib.zk_powers_free)
        n1, n2 = C.c_size_t(), C.c_size_t()
        self._check(self.lib.zk_powers_dims(p, C.byref(n1), C.byref(n2)))
        h.n_tau_g1, h.n_rest = n1.value, n2.value
        return h

    def powers_upload(self, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2):
        """zk_powers_upload: a resident transcript from canonical affine limbs (range, curve and G2-subgroup checked; whether it IS a
        transcript is powers_check's question).  -> Powers"""
        t1, t1p = _u64(np.asarray(tau_g1).reshape(-1, 8))
        t2, t2p = _u64(np.asarray(tau_g2).reshape(-1, 16))
        a1, a1p = _u64(np.asarray(alpha_tau_g1).reshape(-1, 8))
        b1, b1p = _u64(np.asarray(beta_tau_g1).reshape(-1, 8))
        b2, b2p = _u64(np.asarray(beta_g2).reshape(16))
        if not (t2.shape[0] == a1.shape[0] == b1.shape[0]):
            raise ValueError("tau_g2, alpha_tau_g1 and beta_tau_g1 differ in length")
        d = _lib.PowersDesc(t1.shape[0], t2.shape[0], t1p, t2p, a1p, b1p, b2p)
        p = C.c_void_p()
        self._check(self.lib.zk_powers_upload(self.ptr, C.byref(d), C.byref(p)))
        return self._powers(p)

    def powers_initial(self, n_tau_g1, n_rest):
        """zk_powers_initial: the head of a ceremony (x = alpha = beta = 1: every entry a generator).  -> Powers"""
        p = C.c_void_p()
        self._check(self.lib.zk_powers_initial(self.ptr, n_tau_g1, n_rest, C.byref(p)))
        return self._powers(p)

    def powers_download(self, powers):
        """zk_powers_download -> dict(tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2) of canonical affine limbs"""
        n1, n2 = powers.n_tau_g1, powers.n_rest
        arrs = dict(tau_g1=np.zeros((n1, 8), np.uint64), tau_g2=np.zeros((n2, 16), np.uint64), alpha_tau_g1=np.zeros((n2, 8), np.uint64),
                    beta_tau_g1=np.zeros((n2, 8), np.uint64), beta_g2=np.zeros(16, np.uint64))
        out = _lib.PowersOut(*[arrs[k].ctypes.data_as(_lib.u64p) for k in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")])
        self._check(self.lib.zk_powers_download(self.ptr, powers.ptr, C.byref(out)))
        return arrs

    def powers_check(self, powers, challenge=None):
        """zk_powers_check: is `powers` a powers-of-tau transcript over the library's generators?  -> PowersCheck.  challenge: None
        draws it from the OS (the only sound choice); an int in [1, r) or (4,) limbs fixes it, for tests."""
        s_, sp = _fr_arg(challenge)
        out = _lib.PowersCheckResult(0xFFFFFFFF, 0xFFFFFFFF)
        self._check(self.lib.zk_powers_check(self.ptr, powers.ptr, sp, C.byref(out)))
        return PowersCheck(out.failed, out.flags)

    def powers_contribute(self, powers, secrets=None, tag=None):
        """zk_powers_contribute: the transcript of (alpha a, beta b, x s) and the record proving knowledge of the three factors for
        `tag`.  secrets: None draws (s, a, b) from the OS inside the library (wiped, never returned); three ints in [1, r) fix them,
        for tests.  -> (Powers, PowersContribution)"""
        s_, sp = _secrets_arg(secrets, "secrets")
        t, tp = _tag_arg(tag)
        p = C.c_void_p()
        rec = PowersContribution()
        self._check(self.lib.zk_powers_contribute(self.ptr, powers.ptr, sp, tp, C.byref(p), C.byref(rec.raw)))
        return self._powers(p), rec

    def powers_contribution_check(self, before, after, contribution, tag=None, challenge=None):
        """zk_powers_contribution_check: is `after` a transcript, and `before` re-keyed by whoever made `contribution` for `tag`?
        -> PowersContributionCheck.  `before` is not checked again.  Leave `challenge` None outside tests."""
        s_, sp = _fr_arg(challenge)
        t, tp = _tag_arg(tag)
        out = _lib.PowersCheckResult(0xFFFFFFFF, 0xFFFFFFFF)
        self._check(self.lib.zk_powers_contribution_check(self.ptr, before.ptr, after.ptr, C.byref(contribution.raw), tp, sp, C.byref(out)))
        return PowersContributionCheck(out.failed, out.flags)

    def crs_from_powers(self, qap, tau_g1, tau_g2=None, alpha_tau_g1=None, beta_tau_g1=None, beta_g2=None):
        """zk_crs_from_powers: the CRS of `qap` (roots-of-unity or integer-roots form) from a powers-of-tau transcript, by group
        operations only -- byte-equal to setup(qap, (alpha, beta, 1, 1, x)) for the transcript's (alpha, beta, x).  tau_g1: (>= 2n-1, 8)
        points [x^k]_1; tau_g2 (>= n, 16), alpha_tau_g1, beta_tau_g1 (>= n, 8) of one common length; beta_g2: (16,).  The transcript is
        NOT checked to be a sequence of powers: run crs_check(result, qap), or powers_check on the transcript.  A Powers handle may be
        given in place of the five arrays: it is downloaded.  -> Crs"""
        if isinstance(tau_g1, Powers):
            a = self.powers_download(tau_g1)
            tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2 = (a[k] for k in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"))
        t1, t1p = _u64(np.asarray(tau_g1).reshape(-1, 8))
        t2, t2p = _u64(np.asarray(tau_g2).reshape(-1, 16))
        a1, a1p = _u64(np.asarray(alpha_tau_g1).reshape(-1, 8))
        b1, b1p = _u64(np.asarray(beta_tau_g1).reshape(-1, 8))
        b2, b2p = _u64(np.asarray(beta_g2).reshape(16))
        if not (t2.shape[0] == a1.shape[0] == b1.shape[0]):
            raise ValueError("tau_g2, alpha_tau_g1 and beta_tau_g1 differ in length")
        d = _lib.PowersDesc(t1.shape[0], t2.shape[0], t1p, t2p, a1p, b1p, b2p)
        p = C.c_void_p()
        self._check(self.lib.zk_crs_from_powers(self.ptr, qap.ptr, C.byref(d), C.byref(p)))
        c = Crs(self, p, self.lib.zk_crs_free)
        c.n, c.m, c.input = qap.n, qap.m, qap.input
        return c

    def qap_weighted_sum(self, qap, weights, which):
        """sum_i weights[i] * u_i / v_i / w_i (which = 0 / 1 / 2; mod.rs:233-253): coefficients (dense QAP) or values on the domain
        (sparse QAP, u and v only) as an (n, 4) uint64 array."""
        w, wp = _u64(np.asarray(weights).reshape(-1, 4))
        out = np.zeros((qap.n, 4), dtype=np.uint64)
        self._check(self.lib.zk_qap_weighted_sum(self.ptr, qap.ptr, wp, w.shape[0], which, out.ctypes.data_as(_lib.u64p)))
        return out

    QAP_CHECK_DTYPE = np.dtype([("bad_gates", np.uint32), ("first_bad", np.uint32), ("flags", np.uint32)])

    def qap_check(self, qap, weights):
        """zk_qap_check: does the witness satisfy the (sparse) QAP?  -> (bad_gates, first_bad or None, wire0_ok): the number of gates
        with U_j V_j != W_j, the lowest such gate (0-based), and whether weights[0] == 1.  Satisfied = (0, None, True).  Only the
        first min(len(weights), m_qap) weights are read, as by prove."""
        w, wp = _u64(np.asarray(weights, dtype=np.uint64).reshape(-1, 4))
        out = _lib.QapCheckResult()
        self._check(self.lib.zk_qap_check(self.ptr, qap.ptr, wp if w.shape[0] else None, w.shape[0], C.byref(out)))
        return int(out.bad_gates), (None if out.first_bad == _lib.QAP_CHECK_NONE else int(out.first_bad)), not (out.flags & _lib.QAP_CHECK_WIRE0)

    def qap_check_dev(self, qap, d_ptr, m, count, stride=None):
        """zk_qap_check_dev: `count` witnesses of m elements in device memory, witness j at d_ptr + j * stride * 32 bytes (stride = m
        when None: Witgen.run's layout) -> structured array (QAP_CHECK_DTYPE) of `count` results; first_bad is QAP_CHECK_NONE
        (0xFFFFFFFF) where every gate holds."""
        out = np.zeros(count, dtype=self.QAP_CHECK_DTYPE)
        self._check(self.lib.zk_qap_check_dev(self.ptr, qap.ptr, C.c_void_p(d_ptr), m, m if stride is None else stride, count,
                                              out.ctypes.data_as(C.POINTER(_lib.QapCheckResult))))
        return out

    def qap_save(self, qap, path):
        """Write the QAP container (zk_qap_save): sparse rows or dense matrices."""
        self._check(self.lib.zk_qap_save(self.ptr, qap.ptr, str(path).encode()))

    def qap_load(self, path):
        p = C.c_void_p()
        self._check(self.lib.zk_qap_load(self.ptr, str(path).encode(), C.byref(p)))
        q = Qap(self, p, self.lib.zk_qap_free)
        n, m, l, dense = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
        self._check(self.lib.zk_qap_dims(p, C.byref(n), C.byref(m), C.byref(l), C.byref(dense)))
        q.n, q.m, q.input, q.dense = n.value, m.value, l.value, bool(dense.value)
        kind = self.lib.zk_qap_kind(p)
        q.roots = {0: "unity", 2: "integers", 3: "arbitrary"}.get(kind)
        if kind == 0:
            q.log_n = q.n.bit_length() - 1      # roots of unity: n = 2^log_n
        return q

    def crs_save(self, crs, path):
        """Write the CRS container (zk_crs_save)."""
        self._check(self.lib.zk_crs_save(self.ptr, crs.ptr, str(path).encode()))

    def crs_load(self, path):
        p = C.c_void_p()
        self._check(self.lib.zk_crs_load(self.ptr, str(path).encode(), C.byref(p)))
        c = Crs(self, p, self.lib.zk_crs_free)
        n, m, l = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.zk_crs_dims(p, C.byref(n), C.byref(m), C.byref(l)))
        c.n, c.m, c.input = n.value, m.value, l.value
        return c

    # ---- prove ----
    def prove(self, crs, qap, weights, r, s):
        """groth16::prove (mod.rs:213-296) with (r, s) injected; returns the 259-byte canonical proof."""
        w, wp = _u64(np.asarray(weights).reshape(-1, 4))
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        self._check(self.lib.zk_prove(self.ptr, crs.ptr, qap.ptr, wp, w.shape[0], rp, sp, out.ctypes.data_as(_lib.u8p)))
        return out.tobytes()

    def prove_dev(self, crs, qap, d_weights_ptr, m, r, s):
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        self._check(self.lib.zk_prove_dev(self.ptr, crs.ptr, qap.ptr, C.c_void_p(d_weights_ptr), m, rp, sp, out.ctypes.data_as(_lib.u8p)))
        return out.tobytes()

    def prove_submit(self, crs, qap, d_weights_ptr, m, r, s):
        """Enqueue one proof without waiting (at most two in flight); returns the ticket for prove_wait."""
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_submit(self.ptr, crs.ptr, qap.ptr, C.c_void_p(d_weights_ptr), m, rp, sp, C.byref(t)))
        return t.value

    def prove_submit_host(self, crs, qap, weights_host_ptr, m, r, s):
        """zk_prove_submit_host: the witness (m x 4 words) is in host memory at `weights_host_ptr` (page-locked memory from
        host_alloc makes the transfer asynchronous); it must stay valid until prove_wait."""
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_submit_host(self.ptr, crs.ptr, qap.ptr, C.c_void_p(weights_host_ptr), m, rp, sp, C.byref(t)))
        return t.value

    def host_alloc(self, shape, dtype=np.uint64):
        """Page-locked host array (zk_host_alloc); free with host_free(arr) when no transfer from it is pending."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        if self.lib.zk_host_alloc(nbytes, C.byref(p)) != 0:
            raise ZkError(-3)
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p is not None:
            self.lib.zk_host_free(C.c_void_p(p))

    def prove_wait(self, ticket, partial=False):
        if partial:
            self._check(self.lib.zk_prove_wait(self.ptr, ticket, None))
            return None
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        self._check(self.lib.zk_prove_wait(self.ptr, ticket, out.ctypes.data_as(_lib.u8p)))
        return out.tobytes()

    def prove_partial_submit(self, crs, qap, d_weights_ptr, m, r, s, rank, world, d_partial_ptr):
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_partial_submit(self.ptr, crs.ptr, qap.ptr, C.c_void_p(d_weights_ptr), m, rp, sp, rank, world,
                                                     C.c_void_p(d_partial_ptr), C.byref(t)))
        return t.value

    def prove_partial(self, crs, qap, d_weights_ptr, m, r, s, rank, world, d_partial_ptr):
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        self._check(self.lib.zk_prove_partial(self.ptr, crs.ptr, qap.ptr, C.c_void_p(d_weights_ptr), m, rp, sp, rank, world, C.c_void_p(d_partial_ptr)))

    # ---- batches (zkgpu.h: zk_prove_batch_submit / zk_prove_batch_wait) ----
    def prove_batch_submit(self, crs, qap, d_weight_ptrs, ms, rs, ss):
        """Enqueue len(rs) proofs over one CRS / QAP as a batch (own witness pointer, length and (r, s) each)."""
        count = len(rs)
        ptrs = (C.c_void_p * count)(*[C.c_void_p(p) for p in d_weight_ptrs])
        lens = (C.c_size_t * count)(*ms)
        r_ = np.ascontiguousarray(np.stack([fr_to_limbs(x) if isinstance(x, int) else np.asarray(x, dtype=np.uint64) for x in rs]).reshape(-1), dtype=np.uint64)
        s_ = np.ascontiguousarray(np.stack([fr_to_limbs(x) if isinstance(x, int) else np.asarray(x, dtype=np.uint64) for x in ss]).reshape(-1), dtype=np.uint64)
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_batch_submit(self.ptr, crs.ptr, qap.ptr, count, ptrs, lens, r_.ctypes.data_as(_lib.u64p),
                                                   s_.ctypes.data_as(_lib.u64p), C.byref(t)))
        return t.value

    def prove_batch_wait(self, ticket, count):
        out = np.zeros(count * PROOF_BYTES, dtype=np.uint8)
        self._check(self.lib.zk_prove_batch_wait(self.ptr, ticket, count, out.ctypes.data_as(_lib.u8p)))
        raw = out.tobytes()
        return [raw[k * PROOF_BYTES:(k + 1) * PROOF_BYTES] for k in range(count)]

    # ---- multi-GPU scalar exchange (zkgpu.h: zk_prove_scalars_submit / zk_prove_msm_submit) ----
    def prove_exchange_elems(self, qap, world):
        """Element counts (32-byte Fr) of the four exchange arrays L, V, U, H for `world` ranks."""
        out = (C.c_size_t * 4)()
        self._check(self.lib.zk_prove_exchange_elems(qap.ptr, world, out))
        return [int(x) for x in out]

    def prove_scalars_submit(self, crs, qap, d_weights_ptr, m, r, s, world, d_ptrs):
        """SpMV / NTT stage of one proof; the scalars of the four inner products go to d_ptrs = (L, V, U, H)."""
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_scalars_submit(self.ptr, crs.ptr, qap.ptr, C.c_void_p(d_weights_ptr), m, rp, sp, world,
                                                     *[C.c_void_p(p) for p in d_ptrs], C.byref(t)))
        return t.value

    def prove_msm_submit(self, crs, qap, sets, rank, world, d_ptrs, d_partials_ptr):
        """Inner products of `sets` proofs over this rank's points from the exchanged chunks d_ptrs = (L, V, U, H)."""
        t = C.c_int(-1)
        self._check(self.lib.zk_prove_msm_submit(self.ptr, crs.ptr, qap.ptr, sets, rank, world, *[C.c_void_p(p) for p in d_ptrs],
                                                 C.c_void_p(d_partials_ptr), C.byref(t)))
        return t.value

    def prove_combine(self, crs, d_partials_ptr, world, r, s):
        r_, rp = _u64(fr_to_limbs(r) if isinstance(r, int) else r)
        s_, sp = _u64(fr_to_limbs(s) if isinstance(s, int) else s)
        out = np.zeros(PROOF_BYTES, dtype=np.uint8)
        self._check(self.lib.zk_prove_combine(self.ptr, crs.ptr, C.c_void_p(d_partials_ptr), world, rp, sp, out.ctypes.data_as(_lib.u8p)))
        return out.tobytes()

    # ---- verify ----
    def verify(self, crs, inputs, proof):
        """groth16::verify (mod.rs:299-320): inputs = the `verify` wires (ints or (k,4) limbs), proof = 259 bytes."""
        a = ints_to_limbs(list(inputs)) if not isinstance(inputs, np.ndarray) else np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, 4)
        pb = np.frombuffer(bytes(proof), dtype=np.uint8).copy()
        ok = C.c_int(0)
        self._check(self.lib.zk_verify(self.ptr, crs.ptr, a.ctypes.data_as(_lib.u64p), a.shape[0], pb.ctypes.data_as(_lib.u8p), C.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def _batch_args(inputs, proofs, name, proof_bytes=PROOF_BYTES):
        """(inputs as (N, k, 4) uint64, proofs as (N, proof_bytes) uint8) for the batch verify calls"""
        if isinstance(proofs, np.ndarray):
            pb = np.ascontiguousarray(proofs, dtype=np.uint8).reshape(-1, proof_bytes)
        else:
            pb = np.frombuffer(b"".join(bytes(p) for p in proofs), dtype=np.uint8).reshape(-1, proof_bytes).copy()
        n = pb.shape[0]
        if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
            a = np.ascontiguousarray(inputs, dtype=np.uint64)
        else:
            rows = [[int(x) for x in r] for r in inputs]
            k = len(rows[0]) if rows else 0
            if any(len(r) != k for r in rows):
                raise ValueError("%s: every proof needs the same number of inputs" % name)
            a = ints_to_limbs([x for r in rows for x in r]).reshape(len(rows), k, 4)
        if a.shape[0] != n or a.shape[2:] != (4,):
            raise ValueError("%s: inputs must hold one row per proof" % name)
        return a, pb

    def verify_batch(self, crs, inputs, proofs):
        """zk_verify_batch: verify on the GPU for every proof j -> (N,) bool array, entry j == verify(crs, inputs[j], proofs[j]).
        inputs: (N, k) ints or (N, k, 4) limbs, the same k for every proof; proofs: a list of 259-byte strings or an (N, 259)
        uint8 array."""
        a, pb = self._batch_args(inputs, proofs, "verify_batch")
        n = pb.shape[0]
        ok = np.zeros(n, dtype=np.int32)
        self._check(self.lib.zk_verify_batch(self.ptr, crs.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1],
                                             pb.ctypes.data_as(_lib.u8p), n, ok.ctypes.data_as(C.POINTER(C.c_int))))
        return ok.astype(bool)

    @staticmethod
    def _proof_rows(proofs, width, name):
        """a list of byte strings or an (N, width) uint8 array -> a contiguous (N, width) uint8 array"""
        if isinstance(proofs, np.ndarray):
            a = np.ascontiguousarray(proofs, dtype=np.uint8)
            return a.reshape(a.size // width, width)
        rows = [bytes(p) for p in proofs]
        if any(len(r) != width for r in rows):
            raise ValueError("%s: every entry is %d bytes" % (name, width))
        return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()

    def verify_batch_compressed(self, crs, inputs, proofs):
        """zk_verify_batch_compressed: verify_batch over 128-byte proofs (a list of strings or an (N, 128) uint8 array), decompressed
        on the GPU -> (N,) bool array, entry j true iff proofs[j] decompresses and verify accepts the result."""
        a, pb = self._batch_args(inputs, proofs, "verify_batch_compressed", PROOF_COMPRESSED_BYTES)
        n = pb.shape[0]
        ok = np.zeros(n, dtype=np.int32)
        self._check(self.lib.zk_verify_batch_compressed(self.ptr, crs.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1],
                                                        pb.ctypes.data_as(_lib.u8p), n, ok.ctypes.data_as(C.POINTER(C.c_int))))
        return ok.astype(bool)

    # ---- the compressed proof form ----
    proof_compress = staticmethod(proof_compress)        # host code, no device work: the module functions
    proof_decompress = staticmethod(proof_decompress)

    def _codec_batch(self, fn, entries, width_in, width_out, name):
        src = self._proof_rows(entries, width_in, name)
        n = src.shape[0]
        out = np.zeros((n, width_out), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.int32)
        self._check(fn(self.ptr, src.ctypes.data_as(_lib.u8p), n, out.ctypes.data_as(_lib.u8p), ok.ctypes.data_as(C.POINTER(C.c_int))))
        return out, ok.astype(bool)

    def proof_compress_batch(self, proofs):
        """zk_proof_compress_batch on the GPU: N 259-byte proofs -> ((N, 128) uint8 array, (N,) bool array); an entry that is no
        canonical proof encoding gives ok = False and 128 zero bytes."""
        return self._codec_batch(self.lib.zk_proof_compress_batch, proofs, PROOF_BYTES, PROOF_COMPRESSED_BYTES, "proof_compress_batch")

    def proof_decompress_batch(self, compressed):
        """zk_proof_decompress_batch on the GPU: N 128-byte strings -> ((N, 259) uint8 array, (N,) bool array); an entry that is no
        valid encoding gives ok = False and 259 bytes of 0xFF."""
        return self._codec_batch(self.lib.zk_proof_decompress_batch, compressed, PROOF_COMPRESSED_BYTES, PROOF_BYTES, "proof_decompress_batch")

    @staticmethod
    def _z_words(z, n):
        """the multipliers of verify_batch_all as an (n, 2) uint64 array; None draws them from os.urandom"""
        if z is None:
            zw = np.frombuffer(os.urandom(16 * n), dtype=np.uint64).reshape(n, 2).copy()
            for j in np.flatnonzero((zw == 0).all(axis=1)):
                while not zw[j].any():
                    zw[j] = np.frombuffer(os.urandom(16), dtype=np.uint64)
        elif isinstance(z, np.ndarray) and z.ndim == 2:
            zw = np.ascontiguousarray(z, dtype=np.uint64)
        else:
            zs = [int(v) for v in z]
            if any(v < 0 or v >> 128 for v in zs):
                raise ValueError("verify_batch_all: every z_j is a 128-bit integer")
            zw = np.array([[v & (2**64 - 1), v >> 64] for v in zs], dtype=np.uint64).reshape(-1, 2)
        if zw.shape[0] != n:
            raise ValueError("verify_batch_all: z must hold one multiplier per proof")
        return zw

    def verify_batch_all(self, crs, inputs, proofs, z=None):
        """zk_verify_batch_all: one verdict for the whole batch -> True iff every proof decodes and the random linear combination
        of their pairing equations with multipliers z holds (inputs and proofs as in verify_batch).  z: N non-zero 128-bit
        multipliers (ints, or an (N, 2) uint64 array of little-endian words); None draws them from os.urandom.  A batch with
        a bad proof passes only for z in a set of density <= 1 / (2^128 - 1), so z must be secret to whoever made the proofs."""
        a, pb = self._batch_args(inputs, proofs, "verify_batch_all")
        n = pb.shape[0]
        zw = self._z_words(z, n)
        ok = C.c_int(0)
        self._check(self.lib.zk_verify_batch_all(self.ptr, crs.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1],
                                                 pb.ctypes.data_as(_lib.u8p), n, zw.ctypes.data_as(_lib.u64p), C.byref(ok)))
        return bool(ok.value)

    def verifying_key(self, crs):
        """zk_vk_from_crs: the VerifyingKey of a device CRS (the points are copied on the verify stream)."""
        p = C.c_void_p()
        self._check(self.lib.zk_vk_from_crs(self.ptr, crs.ptr, C.byref(p)))
        return VerifyingKey(p, self)

    # ---- Poseidon (zksnark_rs_amd.poseidon) ----
    def poseidon_hash_batch(self, inputs, arity=None, count=None, d_out_ptr=None):
        """zk_poseidon_hash_batch.  Device form: inputs = a device pointer to count x arity x 4 canonical words, d_out_ptr = count x 4
        words.  Host form (arity, count, d_out_ptr left out): inputs (count, arity, 4) uint64 or rows of integers -> (count, 4)
        uint64, staged through torch tensors on the context's device."""
        if d_out_ptr is not None:
            self._check(self.lib.zk_poseidon_hash_batch(self.ptr, C.c_void_p(inputs), arity, count, C.c_void_p(d_out_ptr)))
            return None
        import torch
        a = inputs if isinstance(inputs, np.ndarray) else np.stack([ints_to_limbs(list(row)) for row in inputs])
        a = np.ascontiguousarray(a, dtype=np.uint64)
        dev = "cuda:%d" % self.device
        d_in = torch.from_numpy(a.view(np.int64)).to(dev)
        d_out = torch.zeros((a.shape[0], 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.zk_poseidon_hash_batch(self.ptr, C.c_void_p(d_in.data_ptr()), a.shape[1], a.shape[0], C.c_void_p(d_out.data_ptr())))
        return d_out.cpu().numpy().view(np.uint64)

    def poseidon_tree(self, leaves, depth, n_leaves=None):
        """zk_poseidon_tree_build -> poseidon.PoseidonTree.  leaves: a device pointer to n_leaves x 4 canonical words, or (n_leaves left
        out) host data, integers or (n, 4) uint64, staged through a torch tensor."""
        from .poseidon import PoseidonTree
        if n_leaves is not None:
            return PoseidonTree(self, leaves, n_leaves, depth)
        import torch
        a = leaves if isinstance(leaves, np.ndarray) else ints_to_limbs(list(leaves))
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        dev = "cuda:%d" % self.device
        d = torch.from_numpy(np.ascontiguousarray(np.vstack([a, np.zeros((1, 4), np.uint64)])).view(np.int64)).to(dev)   # never an empty tensor
        torch.cuda.synchronize(dev)
        return PoseidonTree(self, d.data_ptr(), a.shape[0], depth)

    # ---- Baby Jubjub (zksnark_rs_amd.babyjub) ----
    def babyjub_mul_batch(self, scalars, points=None, count=None, d_out_ptr=None, out_stride_words=0):
        """zk_babyjub_mul_batch: [scalars[j]] points[j], or [scalars[j]] Base8 where points is None.  Device form (count and d_out_ptr
        given): scalars and points are device pointers to count x 4 words and count x 8 canonical words (points may be None); the
        affine results go to the 8 words at d_out_ptr + j * out_stride_words words (0 or 8: packed, the input of poseidon_hash_batch
        of arity 2).  Host form: scalars = integers below 2^256 or (count, 4) uint64, points = pairs of integers or (count, 2, 4)
        uint64 -> (count, 2, 4) uint64, staged through torch tensors on the context's device."""
        if d_out_ptr is not None:
            self._check(self.lib.zk_babyjub_mul_batch(self.ptr, C.c_void_p(scalars), C.c_void_p(points) if points is not None else None, count,
                                                      C.c_void_p(d_out_ptr), out_stride_words))
            return None
        import torch
        from .babyjub import scalars_to_words
        s = scalars if isinstance(scalars, np.ndarray) else scalars_to_words(scalars)
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        n = s.shape[0]
        dev = "cuda:%d" % self.device
        pad = lambda a, width: np.ascontiguousarray(np.vstack([a.reshape(-1, width), np.zeros((1, width), np.uint64)]))   # noqa: E731 -- never an empty tensor
        d_s = torch.from_numpy(pad(s, 4).view(np.int64)).to(dev)
        d_p = None
        if points is not None:
            p = points if isinstance(points, np.ndarray) else np.stack([ints_to_limbs([int(x), int(y)]) for x, y in points]) if n else np.zeros((0, 2, 4), np.uint64)
            p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 8)
            if p.shape[0] != n:
                raise ZkError(_lib.ZK_ERR_ARG, "babyjub: %d scalars and %d points" % (n, p.shape[0]))
            d_p = torch.from_numpy(pad(p, 8).view(np.int64)).to(dev)
        d_out = torch.zeros((n + 1, 8), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.zk_babyjub_mul_batch(self.ptr, C.c_void_p(d_s.data_ptr()), C.c_void_p(d_p.data_ptr()) if d_p is not None else None, n,
                                                  C.c_void_p(d_out.data_ptr()), 0))
        return d_out.cpu().numpy().view(np.uint64)[:n].reshape(n, 2, 4)

    # ---- EdDSA-Poseidon (zksnark_rs_amd.eddsa) ----
    def eddsa_verify_batch(self, points_msg, s, count=None, d_status_ptr=None, d_bits_ptr=None, bits_stride_bytes=64, bits=False):
        """zk_eddsa_verify_batch: one verdict (eddsa.VALID .. eddsa.MISMATCH) per signature.  Device form (count and d_status_ptr given):
        points_msg and s are device pointers to count x 20 words (A.x, A.y, R8.x, R8.y, M) and count x 4 words; the statuses go to
        count uint32 at d_status_ptr and, where d_bits_ptr is given, the 251 bits of S and 254 bits of hm to rows bits_stride_bytes
        apart (zk_mixgen_run's d_in_bits).  Host form: points_msg = rows of five integers or (count, 5, 4) uint64, s = integers or
        (count, 4) uint64 -> (count,) uint32, or (statuses, (count, bits_stride_bytes) uint8) with bits=True, staged through torch
        tensors on the context's device."""
        if d_status_ptr is not None:
            self._check(self.lib.zk_eddsa_verify_batch(self.ptr, C.c_void_p(points_msg), C.c_void_p(s), count, C.c_void_p(d_status_ptr),
                                                       C.c_void_p(d_bits_ptr) if d_bits_ptr is not None else None, bits_stride_bytes))
            return None
        import torch
        from .babyjub import scalars_to_words
        p = points_msg if isinstance(points_msg, np.ndarray) else (np.stack([ints_to_limbs([int(x) for x in row]) for row in points_msg])
                                                                   if len(points_msg) else np.zeros((0, 5, 4), np.uint64))
        p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 20)
        sw = np.ascontiguousarray(s if isinstance(s, np.ndarray) else scalars_to_words(s), dtype=np.uint64).reshape(-1, 4)
        n = p.shape[0]
        if sw.shape[0] != n:
            raise ZkError(_lib.ZK_ERR_ARG, "eddsa: %d points and %d signatures" % (n, sw.shape[0]))
        dev = "cuda:%d" % self.device
        pad = lambda a, width: np.ascontiguousarray(np.vstack([a.reshape(-1, width), np.zeros((1, width), np.uint64)]))   # noqa: E731 -- never an empty tensor
        d_p = torch.from_numpy(pad(p, 20).view(np.int64)).to(dev)
        d_s = torch.from_numpy(pad(sw, 4).view(np.int64)).to(dev)
        d_status = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        d_bits = torch.zeros((n + 1, bits_stride_bytes), dtype=torch.uint8, device=dev) if bits else None
        torch.cuda.synchronize(dev)
        self._check(self.lib.zk_eddsa_verify_batch(self.ptr, C.c_void_p(d_p.data_ptr()), C.c_void_p(d_s.data_ptr()), n, C.c_void_p(d_status.data_ptr()),
                                                   C.c_void_p(d_bits.data_ptr()) if bits else None, bits_stride_bytes))
        status = d_status.cpu().numpy().view(np.uint32)[:n]
        return (status, d_bits.cpu().numpy()[:n]) if bits else status

    def eddsa_sign_batch(self, keys, nonce_keys, msgs, count=None, d_points_msg_ptr=None, d_s_ptr=None, d_bits_ptr=None, bits_stride_bytes=64,
                         bits=False):
        """zk_eddsa_sign_batch: instance j is signed as eddsa.sign(keys[j], nonce_keys[j], msgs[j]).  Device form (count, d_points_msg_ptr
        and d_s_ptr given): keys, nonce_keys and msgs are device pointers to count x 4 words each; the rows (A.x, A.y, R8.x, R8.y, M), with
        A = [k] Base8 computed in the call, go to count x 20 words at d_points_msg_ptr, S to count x 4 words at d_s_ptr -- the inputs of
        eddsa_verify_batch -- and, where d_bits_ptr is given, the bit rows eddsa_verify_batch writes to rows bits_stride_bytes apart.
        Host form: keys, nonce_keys, msgs = integers or (count, 4) uint64 -> ((count, 5, 4), (count, 4)) uint64, plus
        (count, bits_stride_bytes) uint8 with bits=True, staged through torch tensors on the context's device.  An input out of range
        raises ZkError (ZK_ERR_RANGE, the text naming the lowest instance and the input) before anything is written."""
        if d_points_msg_ptr is not None:
            self._check(self.lib.zk_eddsa_sign_batch(self.ptr, C.c_void_p(keys), C.c_void_p(nonce_keys), C.c_void_p(msgs), count,
                                                     C.c_void_p(d_points_msg_ptr), C.c_void_p(d_s_ptr),
                                                     C.c_void_p(d_bits_ptr) if d_bits_ptr is not None else None, bits_stride_bytes))
            return None
        import torch
        from .babyjub import scalars_to_words
        words = [np.ascontiguousarray(a if isinstance(a, np.ndarray) else scalars_to_words(a), dtype=np.uint64).reshape(-1, 4)
                 for a in (keys, nonce_keys, msgs)]
        n = words[0].shape[0]
        if words[1].shape[0] != n or words[2].shape[0] != n:
            raise ZkError(_lib.ZK_ERR_ARG, "eddsa: %d keys, %d nonce keys and %d messages" % tuple(w.shape[0] for w in words))
        dev = "cuda:%d" % self.device
        d_k, d_n, d_m = [torch.from_numpy(np.ascontiguousarray(np.vstack([w, np.zeros((1, 4), np.uint64)])).view(np.int64)).to(dev)
                         for w in words]                     # never an empty tensor
        d_p = torch.zeros((n + 1, 20), dtype=torch.int64, device=dev)
        d_s = torch.zeros((n + 1, 4), dtype=torch.int64, device=dev)
        d_bits = torch.zeros((n + 1, bits_stride_bytes), dtype=torch.uint8, device=dev) if bits else None
        torch.cuda.synchronize(dev)
        try:
            self._check(self.lib.zk_eddsa_sign_batch(self.ptr, C.c_void_p(d_k.data_ptr()), C.c_void_p(d_n.data_ptr()), C.c_void_p(d_m.data_ptr()), n,
                                                     C.c_void_p(d_p.data_ptr()), C.c_void_p(d_s.data_ptr()),
                                                     C.c_void_p(d_bits.data_ptr()) if bits else None, bits_stride_bytes))
        finally:
            d_k.zero_()                                     # the staged copy of the keys
            torch.cuda.synchronize(dev)
        out = (d_p.cpu().numpy().view(np.uint64)[:n].reshape(n, 5, 4), d_s.cpu().numpy().view(np.uint64)[:n])
        return out + (d_bits.cpu().numpy()[:n],) if bits else out

    # ---- profiling ----
    def profile_reset(self):
        self._check(self.lib.zk_profile_reset(self.ptr))

    def profile(self):
        out = {}
        for i in range(self.lib.zk_profile_count(self.ptr)):
            name, ms, cnt, by = C.c_char_p(), C.c_double(), C.c_uint64(), C.c_double()
            self.lib.zk_profile_entry(self.ptr, i, C.byref(name), C.byref(ms), C.byref(cnt), C.byref(by))
            out[name.value.decode()] = dict(total_ms=ms.value, launches=cnt.value, algo_bytes=by.value)
        return out

    # ---- the plan record (zkgpu_measure.h: the "msm_plan" option keys) ----
    MSM_PLAN_FIELDS = ("n_used", "g2", "groups", "c", "windows_owned", "buckets", "run_len", "run_branch", "quad_tail", "unchained", "cu_count")

    def msm_plan_reset(self):
        self.set_option("msm_plan_reset", 0)

    def msm_plans(self):
        """What every inner product since the last msm_plan_reset decided from its size: a list of dicts with the fields
        zkgpu_measure.h lists, in the order the host enqueued the products."""
        return [{f: self.get_option("msm_plan.%d.%s" % (i, f)) for f in self.MSM_PLAN_FIELDS} for i in range(self.get_option("msm_plan_count"))]


class VerifyingKey:
    """zk_vk: what groth16::verify reads of the CRS (alpha, beta, gamma, delta, sum_gamma[0..l]) as an object of its own.  The
    object is host data: from_points / from_bytes / load / to_bytes / save / verify need neither a Context nor a GPU.  The batch
    calls take a Context; the first one binds the key to it (constants and input-sum tables stay resident on that device)."""

    def __init__(self, ptr, ctx=None):
        """ptr: a zk_vk*; ctx: the Context this key's batch calls are meant for (see the `ctx` attribute)"""
        self.lib = _lib.load()
        self.ptr = ptr
        #: the Context that groth16.verify_batch* run this key on, or None.  Context.verifying_key and groth16.verifying_key set
        #: it; from_points / from_bytes / load take it as an argument, and it may be assigned later.  The methods of this class
        #: take their Context explicitly and do not read it.
        self.ctx = ctx

    @staticmethod
    def _new(rc, p, what, ctx=None):
        if rc != 0:
            raise ZkError(rc, what)
        return VerifyingKey(p, ctx)

    @classmethod
    def from_points(cls, alpha_g1, beta_g2, gamma_g2, delta_g2, sum_gamma_g1, ctx=None):
        """zk_vk_create: limb arrays as everywhere in the ABI -- (8,), (16,) x 3 and (l + 1, 8).  ZkError(ZK_ERR_RANGE) for a
        point out of range, off its curve or (G2) outside the order-r subgroup."""
        a, ap = _u64(np.asarray(alpha_g1).reshape(8))
        b, bp = _u64(np.asarray(beta_g2).reshape(16))
        g, gp = _u64(np.asarray(gamma_g2).reshape(16))
        d, dp = _u64(np.asarray(delta_g2).reshape(16))
        sg, sgp = _u64(np.asarray(sum_gamma_g1).reshape(-1, 8))
        if sg.shape[0] < 1:
            raise ValueError("VerifyingKey.from_points: sum_gamma holds l + 1 >= 1 points")
        desc = _lib.VkDesc(sg.shape[0] - 1, ap, bp, gp, dp, sgp)
        p = C.c_void_p()
        return cls._new(_lib.load().zk_vk_create(C.byref(desc), C.byref(p)), p, "VerifyingKey.from_points", ctx)

    @classmethod
    def from_bytes(cls, data, ctx=None):
        """zk_vk_from_bytes: ZkError(ZK_ERR_IO) for a wrong length, magic or checksum, ZK_ERR_RANGE for a bad point."""
        data = bytes(data)
        buf = np.frombuffer(data or b"\0", dtype=np.uint8).copy()      # an empty string still needs a pointer
        p = C.c_void_p()
        return cls._new(_lib.load().zk_vk_from_bytes(buf.ctypes.data_as(_lib.u8p), len(data), C.byref(p)), p, "VerifyingKey.from_bytes", ctx)

    @classmethod
    def load(cls, path, ctx=None):
        p = C.c_void_p()
        return cls._new(_lib.load().zk_vk_load(str(path).encode(), C.byref(p)), p, "VerifyingKey.load", ctx)

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.zk_vk_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def input(self):
        l = C.c_size_t(0)
        rc = self.lib.zk_vk_dims(self.ptr, C.byref(l))
        if rc != 0:
            raise ZkError(rc)
        return int(l.value)

    def to_bytes(self):
        out = np.zeros(int(self.lib.zk_vk_bytes(self.input)), dtype=np.uint8)
        rc = self.lib.zk_vk_to_bytes(self.ptr, out.ctypes.data_as(_lib.u8p), out.size)
        if rc != 0:
            raise ZkError(rc)
        return out.tobytes()

    def save(self, path):
        rc = self.lib.zk_vk_save(self.ptr, str(path).encode())
        if rc != 0:
            raise ZkError(rc, "VerifyingKey.save")

    def verify(self, inputs, proof):
        """zk_vk_verify: groth16::verify on the host, no Context: the verdict Context.verify gives over the CRS."""
        a = ints_to_limbs(list(inputs)) if not isinstance(inputs, np.ndarray) else np.ascontiguousarray(inputs, dtype=np.uint64).reshape(-1, 4)
        pb = np.frombuffer(bytes(proof), dtype=np.uint8).copy()
        if pb.size != PROOF_BYTES:
            raise ValueError("VerifyingKey.verify: a proof is %d bytes" % PROOF_BYTES)
        ok = C.c_int(0)
        rc = self.lib.zk_vk_verify(self.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[0], pb.ctypes.data_as(_lib.u8p), C.byref(ok))
        if rc != 0:
            raise ZkError(rc, "VerifyingKey.verify")
        return bool(ok.value)

    # ---- on a Context ----
    def _batch(self, fn, ctx, inputs, proofs, name, width):
        a, pb = Context._batch_args(inputs, proofs, name, width)
        n = pb.shape[0]
        ok = np.zeros(n, dtype=np.int32)
        ctx._check(fn(ctx.ptr, self.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1], pb.ctypes.data_as(_lib.u8p), n,
                      ok.ctypes.data_as(C.POINTER(C.c_int))))
        return ok.astype(bool)

    def verify_batch(self, ctx, inputs, proofs):
        """zk_vk_verify_batch: Context.verify_batch with the key in the place of the CRS -> (N,) bool array."""
        return self._batch(self.lib.zk_vk_verify_batch, ctx, inputs, proofs, "verify_batch", PROOF_BYTES)

    def verify_batch_compressed(self, ctx, inputs, proofs):
        """zk_vk_verify_batch_compressed: the same over 128-byte proofs."""
        return self._batch(self.lib.zk_vk_verify_batch_compressed, ctx, inputs, proofs, "verify_batch_compressed", PROOF_COMPRESSED_BYTES)

    def verify_batch_all(self, ctx, inputs, proofs, z=None):
        """zk_vk_verify_batch_all: Context.verify_batch_all with the key in the place of the CRS -> one bool."""
        a, pb = Context._batch_args(inputs, proofs, "verify_batch_all")
        n = pb.shape[0]
        zw = Context._z_words(z, n)
        ok = C.c_int(0)
        ctx._check(self.lib.zk_vk_verify_batch_all(ctx.ptr, self.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1],
                                                   pb.ctypes.data_as(_lib.u8p), n, zw.ctypes.data_as(_lib.u64p), C.byref(ok)))
        return bool(ok.value)

    def input_sums(self, ctx, inputs, tables=True):
        """zk_vk_input_sums: S_j = sum_gamma_0 + sum_i x_ji sum_gamma_i for every row of `inputs` ((N, k) ints or (N, k, 4)
        limbs) -> (N, 8) uint64 array of affine points (infinity = zeros).  tables=False runs verify_batch's bit-serial kernel,
        tables=True the key's window tables; the words are the same."""
        if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
            a = np.ascontiguousarray(inputs, dtype=np.uint64)
        else:
            rows = [[int(x) for x in r] for r in inputs]
            k = len(rows[0]) if rows else 0
            if any(len(r) != k for r in rows):
                raise ValueError("input_sums: every row needs the same number of inputs")
            a = ints_to_limbs([x for r in rows for x in r]).reshape(len(rows), k, 4)
        n = a.shape[0]
        out = np.zeros((n, 8), dtype=np.uint64)
        ctx._check(self.lib.zk_vk_input_sums(ctx.ptr, self.ptr, a.ctypes.data_as(_lib.u64p) if a.size else None, a.shape[1], n,
                                             1 if tables else 0, out.ctypes.data_as(_lib.u64p)))
        return out
