"""EdDSA-Poseidon test cases shared by tests/test_eddsa.py (host) and tests/test_gpu_eddsa.py (device): signatures of every status,
built from tests/eddsa_model.py, and the gadget circuit built twice (gadget_cases.Pair over eddsa_model.Gadget) with its edge
instances.  Everything is computed once and handed out read-only.  Nothing here needs a device or torch."""
import functools

from zksnark_rs_amd import SplitMix64

import babyjub_model as bm
import eddsa_model as em
import gadget_cases as gc

R, L = bm.R, bm.L
WORD = 1 << 64


@functools.lru_cache(maxsize=None)
def keys():
    """(k, A) for k in 1, 2, L - 1 and a drawn one"""
    rng = SplitMix64(3100)
    return tuple((k, em.public_key(k)) for k in (1, 2, L - 1, rng.fr() % L or 1))


@functools.lru_cache(maxsize=None)
def base():
    """one valid signature (A, M, R8, S) whose S + L is still below 2^251, so that the bits of S + L can be supplied to the circuit"""
    rng = SplitMix64(3101)
    k = rng.fr() % L or 1
    a = em.public_key(k)
    while True:
        msg = rng.fr()
        r8, s = em.sign(k, 7, msg)
        if s + L < 1 << em.S_BITS:
            return a, msg, r8, s


@functools.lru_cache(maxsize=None)
def alias():
    """a valid signature whose challenge hm is below 2^254 - r (about one drawn message in four): hm + r fits the 254 bit wires"""
    rng = SplitMix64(3102)
    k = rng.fr() % L or 1
    a = em.public_key(k)
    while True:
        msg = rng.fr()
        r8, s = em.sign(k, R - 1, msg)
        if em.challenge(r8, a, msg) < (1 << em.HM_BITS) - R:
            return a, msg, r8, s


def flip(value, bit):
    return value ^ (1 << bit)


@functools.lru_cache(maxsize=None)
def status_cases():
    """(name, A, M, R8, S, status): every status on constructed inputs; the status is the one the construction intends and
    test_eddsa.py holds the model to it"""
    a, msg, r8, s = base()
    out = [("valid", a, msg, r8, s, em.VALID),
           ("s_plus_l", a, msg, r8, s + L, em.S_RANGE),                 # satisfies the equation
           ("s_is_l", a, msg, r8, L, em.S_RANGE),
           ("a_x_is_r", (R, a[1]), msg, r8, s, em.RANGE),
           ("a_y_is_r", (a[0], R), msg, r8, s, em.RANGE),
           ("r8_x_is_r", a, msg, (R, r8[1]), s, em.RANGE),
           ("r8_y_is_r", a, msg, (r8[0], R), s, em.RANGE),
           ("msg_is_r", a, R, r8, s, em.RANGE),
           ("s_is_r", a, msg, r8, R, em.RANGE),
           ("all_ones", ((1 << 256) - 1,) * 2, (1 << 256) - 1, ((1 << 256) - 1,) * 2, (1 << 256) - 1, em.RANGE),
           ("key_off_curve", (a[0], (a[1] + 1) % R), msg, r8, s, em.KEY_OFF_CURVE),
           ("r_off_curve", a, msg, (r8[0], (r8[1] + 1) % R), s, em.R_OFF_CURVE),
           ("both_off_curve", (1, 1), msg, (0, 0), s, em.KEY_OFF_CURVE),
           ("key_off_curve_s_range", (a[0], (a[1] + 1) % R), msg, r8, L, em.KEY_OFF_CURVE),
           ("wrong_message", a, (msg + 1) % R, r8, s, em.MISMATCH),
           ("wrong_key", em.public_key(5), msg, r8, s, em.MISMATCH),
           ("s_zero", a, msg, r8, 0, em.MISMATCH)]
    # the identity as key: any S with R8 = [S] Base8 is valid -- no small-order check, as documented
    for sv in (0, 1, L - 1):
        out.append(("identity_key_%d" % (sv % 7), bm.IDENTITY, msg, bm.pmul(sv) if sv else bm.IDENTITY, sv, em.VALID))
    # keys of order 2, 4 and 8: [8] ([hm] A) is the identity whatever hm is
    for name, pt in (("order2", gc.ORDER_2), ("order4", gc.ORDER_4), ("order8", gc.ORDER_8)):
        out.append(("%s_valid" % name, pt, msg, bm.pmul(s), s, em.VALID))
        out.append(("%s_mismatch" % name, pt, msg, r8, s, em.MISMATCH))
    # one flipped bit in each of the six words
    for name, bit in (("low", 0), ("mid", 130), ("top", 253)):
        out.append(("flip_ax_%s" % name, (flip(a[0], bit), a[1]), msg, r8, s, None))
        out.append(("flip_ay_%s" % name, (a[0], flip(a[1], bit)), msg, r8, s, None))
        out.append(("flip_rx_%s" % name, a, msg, (flip(r8[0], bit), r8[1]), s, None))
        out.append(("flip_ry_%s" % name, a, msg, (r8[0], flip(r8[1], bit)), s, None))
        out.append(("flip_msg_%s" % name, a, flip(msg, bit), r8, s, None))
        out.append(("flip_s_%s" % name, a, msg, r8, flip(s, bit), None))
    done = []
    for name, pa, pm_, pr, ps, want in out:
        got = em.verify(pa, pm_, pr, ps)
        if want is None:                                    # a flipped bit: a mismatch, or the earlier status where one applies
            assert got != em.VALID, name
            want = got
        assert got == want, (name, got, want)
        done.append((name, pa, pm_, pr, ps, want))
    assert {c[5] for c in done} == set(range(6))
    return tuple(done)


def signatures(count, seed=3200):
    """`count` valid signatures (A, M, R8, S) over four keys, drawn messages and nonce keys"""
    rng = SplitMix64(seed)
    ks = keys()
    out = []
    for j in range(count):
        k, a = ks[j % len(ks)]
        msg = rng.fr()
        r8, s = em.sign(k, rng.fr(), msg)
        out.append((a, msg, r8, s))
    return out


# ---- the gadget circuit ---------------------------------------------------------------------------------
class Pair(gc.Pair):
    def __init__(self):
        super().__init__()
        self.model = em.Gadget()


GATE_R8_CURVE = 3
GATE_S_BELOW_L = 4 + em.compare_less_gates(em.S_BITS)
GATE_HM_BELOW_R = GATE_S_BELOW_L + 1 + em.compare_less_gates(em.HM_BITS)
GATE_HM_SUM = GATE_HM_BELOW_R + 1 + 325
GATE_A_CURVE = GATE_HM_SUM + 1 + 3


def circuit_row(a, msg, r8, s_value, hm_value):
    return em.field_row(a, msg, r8) + em.bits_of(s_value, em.S_BITS) + em.bits_of(hm_value, em.HM_BITS)


@functools.lru_cache(maxsize=None)
def gadget_case():
    """the circuit of zk_builder_eddsa_verify with the key and the message public, and its edge instances with the gates each leaves
    unsatisfied"""
    p = Pair()
    ax, ay, rx, ry, m = [p.field() for _ in range(5)]
    s_bits = p.bits(em.S_BITS)
    hm_bits = p.bits(em.HM_BITS)
    p.both("eddsa_verify", [ax, ay], [rx, ry], m, s_bits, hm_bits)
    gates = p.lib.dims()[1]
    assert gates == em.eddsa_gates() == 73384
    c, f = p.finish([ax, ay, m])
    a, msg, r8, s = base()
    hm = em.challenge(r8, a, msg)
    last = (gates - 4, gates - 1)                           # the two closing assertions
    named = [("valid", circuit_row(a, msg, r8, s, hm), []),
             ("tampered", circuit_row(a, msg, r8, flip(s, 3), hm), list(last)),
             ("s_plus_l", circuit_row(a, msg, r8, s + L, hm), [GATE_S_BELOW_L])]
    aa, amsg, ar8, a_s = alias()
    ahm = em.challenge(ar8, aa, amsg)
    named.append(("alias_canonical", circuit_row(aa, amsg, ar8, a_s, ahm), []))
    named.append(("alias", circuit_row(aa, amsg, ar8, a_s, ahm + R), None))
    named.append(("order8_key", circuit_row(gc.ORDER_8, msg, bm.pmul(s), s, em.challenge(bm.pmul(s), gc.ORDER_8, msg)), []))
    named.append(("identity_key", circuit_row(bm.IDENTITY, msg, bm.pmul(s), s, em.challenge(bm.pmul(s), bm.IDENTITY, msg)), []))
    named.append(("r_off_curve", circuit_row(a, msg, (r8[0], (r8[1] + 1) % R), s, em.challenge((r8[0], (r8[1] + 1) % R), a, msg)), None))
    rows, failing = [], []
    for name, row, bad in named:
        want = f.failing_gates(f.evaluate(row))
        if name == "alias":                                 # hm + r passes the sum, fails the comparison, and [hm + r] A is another point
            assert GATE_HM_BELOW_R in want and GATE_HM_SUM not in want and GATE_S_BELOW_L not in want
        elif name == "r_off_curve":
            assert GATE_R8_CURVE in want
        else:
            assert want == bad, (name, want, bad)
        rows.append(row)
        failing.append(want)
    return gc.Case("eddsa_verify", c, f, rows, range(len(rows)), failing, names=[n for n, _, _ in named], gates=gates)
