"""A Python model of zk_powers_check / zk_powers_contribution_check (include/zkgpu.h) over EXPONENTS: a transcript is the dict of the
discrete logarithms of its points (tau_g1[k] = e G etc., G and H the library's generators; infinity = 0), e(a G, b H) = gt^(a b), so
every relation is an identity of Python integers mod r.  It shares no code with csrc/powers.hip (no MSM, no pairing).
tests/test_powers_check_model.py pins the bits every alteration must set by reasoning; tests/test_gpu_powers.py builds the same
alterations as points and compares the device's verdict with the model's for the same challenge."""
import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib

R = zk.R_MODULUS
BIT = {name: 1 << k for k, name in enumerate(_lib.POWERS_CHECK_BITS) if name}
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")


def exponents(alpha, beta, x, n1, n2):
    """the transcript of (alpha, beta, x): x^k (k < n1), x^k, alpha x^k, beta x^k (k < n2), beta"""
    xs = [1] * n1
    for k in range(1, n1):
        xs[k] = xs[k - 1] * x % R
    return dict(tau_g1=xs, tau_g2=xs[:n2], alpha_tau_g1=[alpha * v % R for v in xs[:n2]], beta_tau_g1=[beta * v % R for v in xs[:n2]],
                beta_g2=beta % R)


def contributed(t, s, a, b):
    """what zk_powers_contribute makes of t for the secrets (s, a, b)"""
    n1, n2 = len(t["tau_g1"]), len(t["tau_g2"])
    sk = [pow(s, k, R) for k in range(n1)]
    return dict(tau_g1=[v * sk[k] % R for k, v in enumerate(t["tau_g1"])], tau_g2=[v * sk[k] % R for k, v in enumerate(t["tau_g2"])],
                alpha_tau_g1=[v * a * sk[k] % R for k, v in enumerate(t["alpha_tau_g1"])],
                beta_tau_g1=[v * b * sk[k] % R for k, v in enumerate(t["beta_tau_g1"])], beta_g2=t["beta_g2"] * b % R), n2


def check(t, c):
    """the ZK_POWERS_CHECK_* bits of zk_powers_check(t) for the challenge c"""
    tau1, tau2, al, be, b2 = t["tau_g1"], t["tau_g2"], t["alpha_tau_g1"], t["beta_tau_g1"], t["beta_g2"]
    n1, n2 = len(tau1), len(tau2)
    rho = [pow(c, k, R) for k in range(n1)]
    dot = lambda arr, count, off=0: sum(rho[k] * arr[k + off] for k in range(count)) % R   # noqa: E731
    G, H = tau1[0], tau2[0]
    bits = 0
    if G != 1 or H != 1:
        bits |= BIT["GENERATORS"]
    if (dot(tau1, n1 - 1) * tau2[1] - dot(tau1, n1 - 1, 1) * H) % R:
        bits |= BIT["POWERS_G1"]
    s2 = dot(tau2, n2)
    if (dot(tau1, n2) * H - G * s2) % R:
        bits |= BIT["POWERS_G2"]
    if (dot(al, n2) * H - al[0] * s2) % R:
        bits |= BIT["ALPHA"]
    if (dot(be, n2) * H - be[0] * s2) % R:
        bits |= BIT["BETA"]
    if (be[0] * H - G * b2) % R:
        bits |= BIT["BETA_TWINS"]
    if not (tau1[1] and tau2[1] and al[0] and be[0] and b2):
        bits |= BIT["DEGENERATE"]
    return bits


def record_points(t):
    """the exponents of the three points a contribution record names"""
    return (t["tau_g1"][1], t["alpha_tau_g1"][0], t["beta_tau_g1"][0])


def check_contribution(before, after, rec_before, rec_after, knowledge_ok, c):
    """zk_powers_contribution_check: check(after), RECORD when the record's points (as exponents) are not the transcripts', KNOWLEDGE
    when a proof does not verify (the caller knows: a Schnorr proof is not a statement about exponents), DEGENERATE for an infinity
    after-point of the record"""
    bits = check(after, c)
    if tuple(rec_before) != record_points(before) or tuple(rec_after) != record_points(after):
        bits |= BIT["RECORD"]
    if not knowledge_ok:
        bits |= BIT["KNOWLEDGE"]
    if not all(rec_after):
        bits |= BIT["DEGENERATE"]
    return bits


def _with(t, name, index, value):
    out = {k: (list(v) if isinstance(v, list) else v) for k, v in t.items()}
    if name == "beta_g2":
        out[name] = value % R
    else:
        out[name][index] = value % R
    return out


def alterations(t, other=0x1234567):
    """[(name, altered transcript, the bits it must set)] for a GOOD transcript t of a generic (alpha, beta, x): the expected bits are
    stated from the relations, not computed.  n_rest >= 3 and n_tau_g1 > n_rest are assumed for the index cases named after them."""
    n1, n2 = len(t["tau_g1"]), len(t["tau_g2"])
    B = BIT
    out = []
    # tau_g1: every entry but G sits in POWERS_G1 (P, Q or both); the first n2 also in POWERS_G2
    for label, k in (("first", 1), ("middle", n2 // 2 if n2 // 2 >= 1 else 1), ("N2-1", n2 - 1), ("N2", n2), ("last", n1 - 1)):
        if k < n1:
            out.append(("tau_g1[%s=%d] replaced" % (label, k), _with(t, "tau_g1", k, t["tau_g1"][k] + other),
                        B["POWERS_G1"] | (B["POWERS_G2"] if k < n2 else 0)))
    # tau_g2[k], k >= 1, moves the one G2 sum: POWERS_G2, ALPHA, BETA; tau_g2[1] is also POWERS_G1's right-hand point
    for label, k in (("first", 1), ("middle", max(n2 // 2, 2)), ("last", n2 - 1)):
        if 1 <= k < n2:
            out.append(("tau_g2[%s=%d] replaced" % (label, k), _with(t, "tau_g2", k, t["tau_g2"][k] + other),
                        B["POWERS_G2"] | B["ALPHA"] | B["BETA"] | (B["POWERS_G1"] if k == 1 else 0)))
    for label, k in (("first", 0), ("middle", n2 // 2), ("last", n2 - 1)):
        out.append(("alpha_tau_g1[%s=%d] replaced" % (label, k), _with(t, "alpha_tau_g1", k, t["alpha_tau_g1"][k] + other), B["ALPHA"]))
        out.append(("beta_tau_g1[%s=%d] replaced" % (label, k), _with(t, "beta_tau_g1", k, t["beta_tau_g1"][k] + other),
                    B["BETA"] | (B["BETA_TWINS"] if k == 0 else 0)))
    if n2 >= 3:
        sw = _with(_with(t, "tau_g1", 1, t["tau_g1"][2]), "tau_g1", 2, t["tau_g1"][1])
        out.append(("tau_g1[1] and [2] swapped", sw, B["POWERS_G1"] | B["POWERS_G2"]))
        sw = _with(_with(t, "alpha_tau_g1", 0, t["alpha_tau_g1"][n2 - 1]), "alpha_tau_g1", n2 - 1, t["alpha_tau_g1"][0])
        out.append(("alpha_tau_g1 ends swapped", sw, B["ALPHA"]))
    # an array shifted by one power: tau_g1 = x^(k+1) is still a geometric sequence of ratio x -- POWERS_G1 and POWERS_G2 hold -- but
    # G = x is not the generator and e(beta, H) != e(x G, beta H); the same for tau_g2 with H = x (ALPHA, BETA hold: both sides gain x)
    x = t["tau_g1"][1]
    sh = dict(t, tau_g1=[v * x % R for v in t["tau_g1"]])
    out.append(("tau_g1 shifted by one power", sh, B["GENERATORS"] | B["BETA_TWINS"]))
    sh = dict(t, tau_g2=[v * x % R for v in t["tau_g2"]])
    out.append(("tau_g2 shifted by one power", sh, B["GENERATORS"] | B["BETA_TWINS"]))
    # alpha x^(k+1) is the transcript of alpha' = alpha x: nothing to find
    out.append(("alpha_tau_g1 shifted by one power", dict(t, alpha_tau_g1=[v * x % R for v in t["alpha_tau_g1"]]), 0))
    out.append(("beta_g2 of another beta", _with(t, "beta_g2", 0, t["beta_g2"] + other), B["BETA_TWINS"]))
    # G sits in POWERS_G1's P, on both sides of POWERS_G2 (weights 1 and S2) and in BETA_TWINS
    out.append(("G replaced by 2 G", _with(t, "tau_g1", 0, 2), B["GENERATORS"] | B["POWERS_G1"] | B["POWERS_G2"] | B["BETA_TWINS"]))
    return out
