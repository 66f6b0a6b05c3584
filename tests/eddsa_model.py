"""EdDSA-Poseidon on Baby Jubjub in Python integers: the model tests/test_eddsa*.py and tests/test_gpu_eddsa.py hold the library
against.  Written from the scheme in include/zkgpu.h over babyjub_model and poseidon_model's Grain stream; nothing here calls the
library.

    params6, permute6, h6     Poseidon of width 6 (R_P = 60): its own R_P, its own Grain seed and its own permutation call, because
                              poseidon_model offers the three public widths only
    public_key, sign, verify  the scheme; verify returns a status code
    challenge                 H6(R8.x, R8.y, A.x, A.y, M)
    bit_row, field_row        what zk_eddsa_verify_batch writes for zk_mixgen_run: 251 bits of S then 254 of hm, and the five fields
    Gadget                    babyjub_model.Gadget with eddsa_verify, emitting the rows the builder must emit
    eddsa_gates()             the gate count, from the parts
"""
import babyjub_model as bm
import poseidon_model as pm
from builder_model import ONE, ZERO, R
from poseidon_model import form_add, form_of, form_terms

L = bm.L
T6, R_P6 = 6, 60
S_BITS, HM_BITS = 251, 254
VALID, RANGE, KEY_OFF_CURVE, R_OFF_CURVE, S_RANGE, MISMATCH = range(6)
STATUS_NAMES = ["VALID", "RANGE", "KEY_OFF_CURVE", "R_OFF_CURVE", "S_RANGE", "MISMATCH"]
H6_12345 = 0x0dab9449e4a1398a15224c0b15a49d598b2174d305a316c918125f8feeb123c0   # circomlibjs, go-iden3-crypto


def _grain6():
    """poseidon_model.grain_int's register seeded for t = 6, R_P = 60"""
    s = 0
    for value, width in [(1, 2), (0, 4), (254, 12), (T6, 12), (pm.R_F, 10), (R_P6, 10), ((1 << 30) - 1, 30)]:
        s = (s << width) | value
    mask = (1 << 80) - 1

    def step(s):
        new = 0
        for k in pm.TAPS:
            new ^= (s >> (79 - k)) & 1
        return ((s << 1) & mask) | new, new

    for _ in range(160):
        s, _ = step(s)
    while True:
        s, first = step(s)
        s, second = step(s)
        if first:
            yield second


_PARAMS6 = []


def params6():
    """(408 round constants, M [6][6]) as integers, by the procedure of poseidon_model.params"""
    if not _PARAMS6:
        draw = pm._elements(_grain6())
        c = []
        while len(c) < (pm.R_F + R_P6) * T6:
            x = next(draw)
            if x < R:
                c.append(x)
        while True:
            xy = [next(draw) % R for _ in range(2 * T6)]
            xs, ys = xy[:T6], xy[T6:]
            if len(set(xy)) == 2 * T6 and all((x + y) % R for x in xs for y in ys):
                break
        _PARAMS6.append((c, [[pow(x + y, R - 2, R) for y in ys] for x in xs]))
    return _PARAMS6[0]


def permute6(state):
    c, m = params6()
    assert len(state) == T6
    for rnd in range(pm.R_F + R_P6):
        state = [(x + c[rnd * T6 + i]) % R for i, x in enumerate(state)]
        if rnd < 4 or rnd >= 4 + R_P6:
            state = [pow(x, 5, R) for x in state]
        else:
            state[0] = pow(state[0], 5, R)
        state = [sum(m[i][j] * state[j] for j in range(T6)) % R for i in range(T6)]
    return state


def h6(a, b, c, d, e):
    assert all(0 <= x < R for x in (a, b, c, d, e))
    return permute6([0, a, b, c, d, e])[0]


def challenge(r8, a, msg):
    return h6(r8[0], r8[1], a[0], a[1], msg)


def public_key(k):
    assert 0 < k < L
    return bm.pmul(k)


def sign(k, nonce_key, msg):
    """-> (R8, S)"""
    assert 0 < k < L and 0 <= nonce_key < R and 0 <= msg < R
    rho = h6(nonce_key, msg, 0, 0, 0) % L
    r8 = bm.pmul(rho) if rho else bm.IDENTITY
    hm = challenge(r8, public_key(k), msg)
    return r8, (rho + 8 * hm * k) % L


def verify(a, msg, r8, s):
    """the status of one signature over any integers below 2^256"""
    if any(x >= R for x in (a[0], a[1], r8[0], r8[1], msg, s)):
        return RANGE
    if not bm.on_curve(a):
        return KEY_OFF_CURVE
    if not bm.on_curve(r8):
        return R_OFF_CURVE
    if s >= L:
        return S_RANGE
    hm = challenge(r8, a, msg)
    right = bm.add(r8, bm.mul(8, bm.mul(hm, a)))
    return VALID if bm.mul(s) == right else MISMATCH


def bit_row(a, msg, r8, s, stride=64):
    """the row of d_bits_out: S mod 2^251, then hm, least significant bit first; zero where the status is RANGE"""
    if any(x >= R for x in (a[0], a[1], r8[0], r8[1], msg, s)):
        return bytes(stride)
    value = (s & ((1 << S_BITS) - 1)) | (challenge(r8, a, msg) << S_BITS)
    return value.to_bytes(64, "little") + bytes(stride - 64)


def field_row(a, msg, r8):
    return [a[0], a[1], r8[0], r8[1], msg]


def bits_of(value, n):
    return [(value >> i) & 1 for i in range(n)]


# ---- the gadget ---------------------------------------------------------------------------------------
class Gadget(bm.Gadget):
    """babyjub_model.Gadget with H6 over forms and the signature statement"""

    def poseidon6_forms(self, forms):
        c, m = params6()
        state = [{}] + [dict(f) for f in forms]
        assert len(state) == T6
        for rnd in range(pm.R_F + R_P6):
            state = [form_add(f, {ONE: c[rnd * T6 + i]}) for i, f in enumerate(state)]
            if rnd < 4 or rnd >= 4 + R_P6:
                state = [self._sbox(f) for f in state]
            else:
                state[0] = self._sbox(state[0])
            mixed = []
            for i in range(T6):
                acc = {}
                for j in range(T6):
                    acc = form_add(acc, state[j], m[i][j])
                mixed.append(acc)
            state = mixed
        return self.sub_circuit(form_terms(state[0]), [(1, ONE)])

    def _assert_below(self, bits, bound):
        lt = self.compare("less_than", bits, [ONE if (bound >> i) & 1 else ZERO for i in range(len(bits))])
        self.assert_forms(form_add(form_of(lt), bm.const_form(-1)), form_of(ONE))

    def eddsa_verify(self, a_xy, r8_xy, msg, s_bits, hm_bits):
        assert len(s_bits) == S_BITS and len(hm_bits) == HM_BITS
        self.babyjub_assert_on_curve(r8_xy)
        self._assert_below(s_bits, L)
        self._assert_below(hm_bits, R)
        digest = self.poseidon6_forms([form_of(w) for w in (r8_xy[0], r8_xy[1], a_xy[0], a_xy[1], msg)])
        total = {}
        for i, b in enumerate(hm_bits):
            total = form_add(total, form_of(b), 1 << i)
        self.assert_forms(form_add(total, form_of(digest), -1), form_of(ONE))
        p = self.babyjub_mul(a_xy, hm_bits)
        for _ in range(3):
            p = self._dbl_forms(*[form_of(w) for w in p])
        right = self._add_forms(form_of(p[0]), form_of(p[1]), form_of(p[2]), form_of(r8_xy[0]), form_of(r8_xy[1]), None)
        left = self.babyjub_mul_fixed(s_bits)
        for k in range(2):
            t1 = self._mulf(form_of(left[k]), form_of(right[2]))
            t2 = self._mulf(form_of(right[k]), form_of(left[2]))
            self.assert_forms(form_add(form_of(t1), form_of(t2), -1), form_of(ONE))


def compare_less_gates(n):
    """zk_builder_compare(ZK_CMP_LESS) over n bits: greater_than (n comparisons, n - 1 equalities, and per bit below the top the fold
    of the equalities above it, an AND and an OR of two), a NOT, is_equal (n XNOR, n - 1 AND), a NOT, an AND"""
    greater = n + (n - 1) + sum((n - 2 - k) + 1 + 2 for k in range(n - 1))
    return greater + 1 + (2 * n - 1) + 1 + 1


def eddsa_gates():
    parts = [4, compare_less_gates(S_BITS) + 1, compare_less_gates(HM_BITS) + 1, 3 * (pm.R_F * T6 + R_P6) + 1, 1, bm.var_gates(HM_BITS), 3 * 7 + 10,
             bm.fixed_gates(S_BITS), 6]
    return sum(parts)
