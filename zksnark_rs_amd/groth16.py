"""groth16::{setup, prove, verify} with the reference's names and argument order (groth16/mod.rs).

    qap              = QAP.from_zk(ctx, code)            # QAP::from(ASTParser::try_parse(code))  (fr.rs:140-173)
    sigmag1, sigmag2 = setup(qap)                         # mod.rs:134   (trapdoor from os.urandom unless given)
    proof            = prove(qap, (sigmag1, sigmag2), weights)           # mod.rs:213
    ok               = verify((sigmag1, sigmag2), inputs, proof)         # mod.rs:299

`sigmag1` / `sigmag2` are two views of one device-resident CRS handle (SigmaG1, SigmaG2).
"""
import os

from . import R_MODULUS, VerifyingKey, ints_to_limbs
from . import proof_compress as _proof_compress, proof_decompress as _proof_decompress
from .circuit import Circuit


def random_elem():
    """Random for FrLocal (fr.rs:90-99): uniform, never zero."""
    while True:
        v = int.from_bytes(os.urandom(40), "little") % R_MODULUS
        if v:
            return v


class QAP:
    """QAP<CoefficientPoly<FrLocal>> (mod.rs:60-67), device resident."""

    def __init__(self, ctx, handle, circuit=None):
        self.ctx, self.handle, self.circuit = ctx, handle, circuit

    @classmethod
    def from_zk(cls, ctx, code, sparse=False):
        """sparse: keep the root representation's rows over the roots 1..n instead of interpolating them (any size)"""
        c = Circuit(code)
        return cls(ctx, c.qap_sparse(ctx) if sparse else c.qap(ctx), c)


class _Sigma:
    """One half of the CRS.  The points live on the device; the reference's fields (mod.rs:105-121) are fetched on first
    access as affine coordinates in canonical little-endian 64-bit limbs: (8,) per G1 point, (16,) per G2 point."""
    _fields = ()

    def __init__(self, ctx, crs, shared):
        self.ctx, self.crs, self._shared = ctx, crs, shared

    def __getattr__(self, name):
        if name in type(self)._fields:
            if "arrays" not in self._shared:
                self._shared["arrays"] = self.ctx.crs_download(self.crs)
            return self._shared["arrays"][name + type(self)._suffix]
        raise AttributeError(name)


class SigmaG1(_Sigma):
    _fields = ("alpha", "beta", "delta", "xi", "sum_gamma", "sum_delta", "xi_t")
    _suffix = "_g1"


class SigmaG2(_Sigma):
    _fields = ("beta", "gamma", "delta", "xi")
    _suffix = "_g2"


def setup(qap, trapdoor=None):
    td = trapdoor if trapdoor is not None else [random_elem() for _ in range(5)]
    crs = qap.ctx.setup(qap.handle, ints_to_limbs(list(td)))
    shared = {}
    return SigmaG1(qap.ctx, crs, shared), SigmaG2(qap.ctx, crs, shared)


def setup_from_powers(qap, powers):
    """The CRS of `qap` from a powers-of-tau transcript, with gamma = delta = 1 and no trapdoor (zk_crs_from_powers): what a ceremony
    starts from instead of setup().  powers: a mapping with tau_g1 (>= 2n-1 points), tau_g2, alpha_tau_g1, beta_tau_g1 (>= n points
    each) and beta_g2, canonical affine limbs, or a resident Powers handle (check_powers / contribute_powers: it is downloaded).  Then
    check_setup(qap, sigma) -- the transcript itself is not checked here, that is check_powers -- and one
    contribute() per party, each verified with check_contribution()."""
    if hasattr(powers, "ptr"):   # a resident Powers handle: downloaded by crs_from_powers
        crs = qap.ctx.crs_from_powers(qap.handle, powers)
    else:
        crs = qap.ctx.crs_from_powers(qap.handle, powers["tau_g1"], powers["tau_g2"], powers["alpha_tau_g1"], powers["beta_tau_g1"],
                                      powers["beta_g2"])
    shared = {}
    return SigmaG1(qap.ctx, crs, shared), SigmaG2(qap.ctx, crs, shared)


def check_powers(powers, challenge=None):
    """Is the resident transcript `powers` a powers-of-tau sequence over the library's generators (zk_powers_check)?  Once per
    transcript, whatever the circuit.  -> PowersCheck: .ok, .failed, .names.  Leave `challenge` None outside tests."""
    return powers.ctx.powers_check(powers, challenge)


def contribute_powers(powers, secrets=None, tag=None):
    """Add one's own randomness to a transcript: the transcript of (alpha a, beta b, x s) and the PowersContribution that proves
    knowledge of (s, a, b) for `tag` (zk_powers_contribute).  Leave `secrets` None (drawn inside the library, wiped, never
    returned) outside tests."""
    return powers.ctx.powers_contribute(powers, secrets, tag)


def check_powers_contribution(before, after, contribution, tag=None, challenge=None):
    """Is `after` a transcript, and `before` re-keyed by whoever made `contribution` for `tag` (zk_powers_contribution_check)?  The
    head of a chain is Context.powers_initial or one check_powers.  -> PowersContributionCheck."""
    return before.ctx.powers_contribution_check(before, after, contribution, tag, challenge)


def prove(qap, sigma, weights, rs=None):
    sigmag1, sigmag2 = sigma
    assert sigmag1.crs is sigmag2.crs, "SigmaG1 / SigmaG2 come from different setups"
    r, s = rs if rs is not None else (random_elem(), random_elem())
    return qap.ctx.prove(sigmag1.crs, qap.handle, weights, r, s)


def is_satisfied(qap, weights):
    """Would prove(qap, sigma, weights) yield a proof that verifies?  True iff every gate holds (U_j V_j == W_j) and weights[0] == 1,
    decided on the GPU before anything is proved (zk_qap_check; sparse QAP forms: QAP.from_zk(..., sparse=True))."""
    bad, _, wire0_ok = qap.ctx.qap_check(qap.handle, weights)
    return bad == 0 and wire0_ok


def first_unsatisfied(qap, weights):
    """The lowest gate (0-based row of the root representation) with U_j V_j != W_j, None when every gate holds."""
    return qap.ctx.qap_check(qap.handle, weights)[1]


def check_setup(qap, sigma, challenge=None):
    """Is `sigma` a CRS of SOME trapdoor for `qap` (zk_crs_check)?  What a prover who did not run setup() asks once about the CRS it
    was handed.  -> CrsCheck: .ok, .failed, .names, .flags.  Leave `challenge` None (drawn from the OS) outside tests."""
    sigmag1, sigmag2 = sigma
    assert sigmag1.crs is sigmag2.crs, "SigmaG1 / SigmaG2 come from different setups"
    return qap.ctx.crs_check(sigmag1.crs, qap.handle, challenge)


def contribute(sigma, d=None, tag=None):
    """Re-key delta: a new (SigmaG1, SigmaG2) whose delta is d times `sigma`'s, and the Contribution that proves knowledge of d for
    `tag` (zk_crs_contribute).  Leave d None (drawn from the OS inside the library, wiped, never returned) outside tests.  What a
    party does to a CRS it was handed so that whoever ran setup() no longer knows its trapdoor."""
    sigmag1, sigmag2 = sigma
    assert sigmag1.crs is sigmag2.crs, "SigmaG1 / SigmaG2 come from different setups"
    crs, record = sigmag1.ctx.crs_contribute(sigmag1.crs, d, tag)
    shared = {}
    return (SigmaG1(sigmag1.ctx, crs, shared), SigmaG2(sigmag1.ctx, crs, shared)), record


def check_contribution(before, after, contribution, tag=None, challenge=None):
    """Is `after` the CRS `before` with only delta re-keyed, by whoever made `contribution` for `tag` (zk_crs_contribution_check)?
    -> ContributionCheck: .ok, .failed, .names.  `after` is then as good a CRS as `before` (check_setup, once, for the first CRS of
    a chain).  Leave `challenge` None outside tests."""
    assert before[0].crs is before[1].crs and after[0].crs is after[1].crs, "SigmaG1 / SigmaG2 come from different setups"
    return before[0].ctx.crs_contribution_check(before[0].crs, after[0].crs, contribution, tag, challenge)


def verifying_key(sigma):
    """The VerifyingKey of a CRS: alpha, beta, gamma, delta and sum_gamma, all verify reads.  It serialises (to_bytes / save) and
    verifies single proofs on the host with no GPU; verify* below take it where they take `sigma`.  The batch calls run on the
    key's `ctx` (VerifyingKey.ctx), here the CRS's context; restore a key with VerifyingKey.from_bytes(data, ctx=...) / load(path,
    ctx=...) to use it with them."""
    sigmag1, sigmag2 = sigma
    return sigmag1.ctx.verifying_key(sigmag1.crs)


def _key_ctx(vk):
    if vk.ctx is None:
        raise ValueError("groth16: this VerifyingKey has no Context (VerifyingKey.from_bytes(data, ctx=...), or assign key.ctx)")
    return vk.ctx


def verify(sigma, inputs, proof):
    if isinstance(sigma, VerifyingKey):
        return sigma.verify(inputs, proof)
    sigmag1, sigmag2 = sigma
    return sigmag1.ctx.verify(sigmag1.crs, inputs, proof)


def verify_batch(sigma, inputs, proofs):
    """verify for many proofs over one CRS on the GPU: inputs[j] (the same count for every j) against proofs[j] -> bool array"""
    if isinstance(sigma, VerifyingKey):
        return sigma.verify_batch(_key_ctx(sigma), inputs, proofs)
    sigmag1, sigmag2 = sigma
    return sigmag1.ctx.verify_batch(sigmag1.crs, inputs, proofs)


def verify_batch_compressed(sigma, inputs, proofs):
    """verify_batch over compressed 128-byte proofs (compress), decompressed on the GPU -> bool array"""
    if isinstance(sigma, VerifyingKey):
        return sigma.verify_batch_compressed(_key_ctx(sigma), inputs, proofs)
    sigmag1, sigmag2 = sigma
    return sigmag1.ctx.verify_batch_compressed(sigmag1.crs, inputs, proofs)


def compress(proof):
    """the 259-byte proof -> the usual 128-byte form: x coordinates with the sign of y in a flag (include/zkgpu.h)"""
    return _proof_compress(proof)


def decompress(compressed):
    """128 bytes -> the 259-byte proof verify takes; raises unless every point decodes onto its curve"""
    return _proof_decompress(compressed)


def verify_batch_all(sigma, inputs, proofs):
    """one verdict for many proofs over one CRS on the GPU: True iff verify would accept every proof (random linear
    combination with secret multipliers drawn from os.urandom; a false pass has probability <= 1 / (2^128 - 1))"""
    if isinstance(sigma, VerifyingKey):
        return sigma.verify_batch_all(_key_ctx(sigma), inputs, proofs)
    sigmag1, sigmag2 = sigma
    return sigmag1.ctx.verify_batch_all(sigmag1.crs, inputs, proofs)


def weights(code, inputs):
    """circuit::weights (circuit/mod.rs:529-637)."""
    return Circuit(code).weights(inputs)
