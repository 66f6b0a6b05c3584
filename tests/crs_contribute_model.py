"""A Python model of the delta contribution (include/zkgpu.h: zk_crs_contribution_prove / _verify / zk_crs_contribution_check): the
record restated with hashlib.sha256, Python integers and the oracle's group operations, the check restated with the oracle's inner
products and the host pairing the way tests/crs_check_model.py restates zk_crs_check (every relation: two Gt values compared).  It
shares no code with csrc/crs_contribution.hip or csrc/crs_contribute.hip.  tests/test_crs_contribute_host.py ties it to the oracle's
setup; tests/test_gpu_crs_contribute.py compares the device's verdict bits with it for the same challenge.  Also here: the GLV split
in Python integers (the constants of tools/glv_constants.py) and the list of alterations both test files walk."""
import hashlib

import numpy as np

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib, ints_to_limbs, limbs_to_int

from crs_check_model import INF1, INF2, is_inf

R = zk.R_MODULUS
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BIT = {name: 1 << k for k, name in enumerate(_lib.CONTRIB_BITS)}
UNCHANGED_KEYS = ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "xi_g1", "xi_g2", "sum_gamma_g1")
ZERO_TAG = bytes(32)

# ---- k = k1 + k2 lambda (tools/glv_constants.py prints these) ----------------------------------------------------------------------
LAMBDA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
A1, B1 = 0x6f4d8248eeb859fc8211bbeb7d4f1128, -0x89d3256894d213e3
A2, B2 = 0x89d3256894d213e3, 0x6f4d8248eeb859fd0be4e1541221250b
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0 and (A1 + B1 * LAMBDA) % R == 0 and (A2 + B2 * LAMBDA) % R == 0 and A1 * B2 - A2 * B1 == R


def glv_split(k):
    """(k1, k2) as signed integers, by the library's roundings c_i = floor(k g_i / 2^256 + 1 / 2), g1 = floor(2^256 b2 / r),
    g2 = floor(2^256 (-b1) / r)"""
    g1, g2 = (B2 << 256) // R, ((-B1) << 256) // R
    c1, c2 = (k * g1 + (1 << 255)) >> 256, (k * g2 + (1 << 255)) >> 256
    return k - c1 * A1 - c2 * A2, -c1 * B1 - c2 * B2


# ---- the record ----------------------------------------------------------------------------------------------------------------------
def words(p):
    return np.asarray(p, dtype=np.uint64).reshape(-1)


def challenge(tag, before, after, commit):
    h = hashlib.sha256(b"ZKCONTRv1\0" + bytes(tag if tag is not None else ZERO_TAG) + words(before).astype("<u8").tobytes()
                       + words(after).astype("<u8").tobytes() + words(commit).astype("<u8").tobytes()).digest()
    return int.from_bytes(h, "big") % R


def record(grp, delta_before, d, nonce, tag):
    """(delta_before, delta_after, T, z) of the record zk_crs_contribution_prove makes"""
    after, commit = grp.mul1(delta_before, d), grp.mul1(delta_before, nonce)
    z = (nonce + challenge(tag, delta_before, after, commit) * d) % R
    return words(delta_before), after, commit, z


def record_bytes(grp, delta_before, d, nonce, tag):
    b, a, t, z = record(grp, delta_before, d, nonce, tag)
    return b.astype("<u8").tobytes() + a.astype("<u8").tobytes() + t.astype("<u8").tobytes() + ints_to_limbs([z]).astype("<u8").tobytes()


def on_curve(p):
    x, y = limbs_to_int(words(p)[:4]), limbs_to_int(words(p)[4:])
    if x >= Q or y >= Q:
        return False
    return (x == 0 and y == 0) or (y * y - x * x * x - 3) % Q == 0


def verify(grp, rec, tag):
    """zk_crs_contribution_verify for a zk.Contribution"""
    b, a, t, z = rec.delta_before_g1, rec.delta_after_g1, rec.commit_g1, rec.response
    if not (on_curve(b) and on_curve(a) and on_curve(t)) or is_inf(b) or is_inf(a) or z >= R:
        return False
    c = challenge(tag, b, a, t)
    return np.array_equal(grp.mul1(b, z), grp.add1(t, grp.mul1(a, c)))


# ---- the check -----------------------------------------------------------------------------------------------------------------------
def check(grp, before, after, rec, tag, s):
    """`failed` of zk_crs_contribution_check for two CRSs as arrays (Context.crs_arrays layout), a zk.Contribution, the tag, the challenge"""
    assert 1 <= s < R
    n, nl = before["xi_g1"].shape[0], before["sum_delta_g1"].shape[0]
    failed = 0
    if not all(np.array_equal(before[k], after[k]) for k in UNCHANGED_KEYS):
        failed |= BIT["UNCHANGED"]
    if not (np.array_equal(rec.delta_before_g1, before["delta_g1"]) and np.array_equal(rec.delta_after_g1, after["delta_g1"])):
        failed |= BIT["RECORD"]
    if not verify(grp, rec, tag):
        failed |= BIT["KNOWLEDGE"]
    if is_inf(after["delta_g1"]) or is_inf(after["delta_g2"]):
        failed |= BIT["DEGENERATE"]
    G, H = after["xi_g1"][0], after["xi_g2"][0]
    if grp.e(after["delta_g1"], H) != grp.e(G, after["delta_g2"]):
        failed |= BIT["DELTA_TWINS"]
    rho = [pow(s, k, R) for k in range(max(n, nl))]
    if grp.e(grp.msm1(after["sum_delta_g1"], rho[:nl]), after["delta_g2"]) != grp.e(grp.msm1(before["sum_delta_g1"], rho[:nl]), before["delta_g2"]):
        failed |= BIT["SUM_DELTA"]
    if n >= 2 and grp.e(grp.msm1(after["xi_t_g1"], rho[:n - 1]), after["delta_g2"]) != grp.e(grp.msm1(before["xi_t_g1"], rho[:n - 1]), before["delta_g2"]):
        failed |= BIT["XI_T"]
    return failed


# ---- an honest successor from the arrays alone, and the alterations -------------------------------------------------------------------
def scaled(grp, pts, k):
    pts = np.asarray(pts, np.uint64).reshape(-1, 8)
    return grp.orc.g1_mul_batch(pts, np.tile(ints_to_limbs([k % R]), (len(pts), 1))) if len(pts) else pts.copy()


def successor(grp, before, d):
    """the arrays of `before` with delta -> d delta (what setup gives for the trapdoor with delta d)"""
    out = {k: np.array(v, copy=True) for k, v in before.items()}
    di = pow(d, -1, R)
    out["delta_g1"], out["delta_g2"] = grp.mul1(before["delta_g1"], d), grp.mul2(before["delta_g2"], d)
    out["sum_delta_g1"], out["xi_t_g1"] = scaled(grp, before["sum_delta_g1"], di), scaled(grp, before["xi_t_g1"], di)
    return out


def copy_arrs(a):
    return {k: np.array(v, copy=True) for k, v in a.items()}


def alterations(grp, before, after, rec, tag, d):
    """[(name, before, after, record, tag, expected `failed`)]: every way the issue lists in which (before, after, record) is not an
    honest contribution, with the bits the header's relations give for it.  `after` = successor(before, d), `rec` its record."""
    n, nl = before["xi_g1"].shape[0], before["sum_delta_g1"].shape[0]
    G = after["xi_g1"][0]
    sd_live = nl > 0 and before["sum_delta_g1"].any()
    xt_live = n >= 2 and before["xi_t_g1"].any()
    out = []

    def alt(name, bits, b=None, a=None, r=None, t=tag):
        out.append((name, b if b is not None else before, a if a is not None else after, r if r is not None else rec, t, bits))

    for pos in sorted({0, nl - 1}) if nl else []:
        a = copy_arrs(after)
        a["sum_delta_g1"][pos] = grp.add1(a["sum_delta_g1"][pos], G)
        alt("sum_delta'[%d] + G" % pos, BIT["SUM_DELTA"], a=a)
    if n >= 2:
        for pos in sorted({0, n - 2}):
            a = copy_arrs(after)
            a["xi_t_g1"][pos] = grp.add1(a["xi_t_g1"][pos], G)
            alt("xi_t'[%d] + G" % pos, BIT["XI_T"], a=a)
    if xt_live:
        a = copy_arrs(after)
        a["xi_t_g1"] = scaled(grp, after["xi_t_g1"], 2)
        alt("xi_t' by another factor", BIT["XI_T"], a=a)
    a = copy_arrs(after)
    a["delta_g2"] = grp.mul2(before["delta_g2"], d + 1)
    alt("delta_g2' of another d", BIT["DELTA_TWINS"] | (BIT["SUM_DELTA"] if sd_live else 0) | (BIT["XI_T"] if xt_live else 0), a=a)
    for key, pos in [("alpha_g1", None), ("gamma_g2", None), ("sum_gamma_g1", len(before["sum_gamma_g1"]) - 1)] + \
                    ([("xi_g1", n - 1), ("xi_g2", n - 1)] if n >= 2 else []):
        a = copy_arrs(after)
        two = (lambda p: grp.add1(p, p)) if a[key].shape[-1] == 8 else (lambda p: grp.add2(p, p))
        if pos is None:
            a[key] = two(a[key])
        else:
            a[key][pos] = two(a[key][pos])
        alt("%s altered" % key, BIT["UNCHANGED"], a=a)
    alt("a record for another tag", BIT["KNOWLEDGE"], t=bytes([1]) + bytes(31))
    raw = bytearray(rec.to_bytes())
    raw[192] ^= 1
    alt("a wrong response", BIT["KNOWLEDGE"], r=zk.Contribution.from_bytes(bytes(raw)))
    alt("a record of another pair", BIT["RECORD"], r=zk.contribution_prove(after["delta_g1"], d, nonce=12345, tag=tag))
    a = copy_arrs(after)
    a["delta_g1"], a["delta_g2"] = INF1.copy(), INF2.copy()
    alt("infinity deltas", BIT["DEGENERATE"] | BIT["RECORD"] | (BIT["SUM_DELTA"] if sd_live else 0) | (BIT["XI_T"] if xt_live else 0), a=a)
    return out
