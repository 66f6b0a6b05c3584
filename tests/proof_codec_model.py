"""A big-integer model of the compressed proof form (include/zkgpu.h "Compressed proof bytes"), independent of the library:
square roots are pow(a, (q+1)//4, q) and the complex method over oracle/pyref.py's Fq2 helpers, the sign is taken on the canonical
integer.  Points are pyref's: None = infinity, G1 = (x, y), G2 = ((x0, x1), (y0, y1)).  Shared by test_proof_codec_host.py and
test_gpu_proof_codec.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402
from pyref import Q, B1, B2, fq2_add, fq2_sub, fq2_mul, fq2_neg  # noqa: E402

HALF = (Q - 1) // 2
INF_G1C = b"\x40" + bytes(31)
INF_G2C = b"\x40" + bytes(63)
INF_PROOF_C = INF_G1C + INF_G2C + INF_G1C
BAD_DECOMPRESSED = b"\xff" * 259
BAD_COMPRESSED = bytes(128)


def fq_sqrt(a):
    r = pow(a % Q, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def fq2_sqrt(a):
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        return (0, fq_sqrt(-a0))
    s = fq_sqrt(a0 * a0 + a1 * a1)
    if s is None:
        return None
    inv2 = pow(2, -1, Q)
    x0 = fq_sqrt((a0 + s) * inv2)
    if x0 is None:
        x0 = fq_sqrt((a0 - s) * inv2)
    x1 = a1 * pow(2 * x0, -1, Q) % Q
    assert fq2_mul((x0, x1), (x0, x1)) == (a0, a1)
    return (x0, x1)


def g1_rhs(x):
    return (x * x * x + B1) % Q


def g2_rhs(x):
    return fq2_add(fq2_mul(fq2_mul(x, x), x), B2)


def larger1(y):
    return y > HALF


def larger2(y):
    return y[1] > HALF if y[1] else y[0] > HALF


def g1_from_x(x, larger):
    """the point with this x whose y has the asked sign, None if x is on no point"""
    y = fq_sqrt(g1_rhs(x))
    if y is None:
        return None
    return (x, y if larger1(y) == larger else (-y) % Q)


def g2_from_x(x, larger):
    y = fq2_sqrt(g2_rhs(x))
    if y is None:
        return None
    return (x, y if larger2(y) == larger else fq2_neg(y))


def enc_g1c(P):
    if P is None:
        return INF_G1C
    b = bytearray(P[0].to_bytes(32, "big"))
    b[0] |= 0xC0 if larger1(P[1]) else 0x80
    return bytes(b)


def enc_g2c(P):
    if P is None:
        return INF_G2C
    (x0, x1), y = P
    b = bytearray(x1.to_bytes(32, "big") + x0.to_bytes(32, "big"))
    b[0] |= 0xC0 if larger2(y) else 0x80
    return bytes(b)


def dec_g1c(b):
    """(valid, point)"""
    flag = b[0] >> 6
    v = int.from_bytes(b, "big") & ((1 << 254) - 1)
    if flag == 1:
        return v == 0, None
    if flag == 0 or v >= Q:
        return False, None
    y = fq_sqrt(g1_rhs(v))
    if y is None or (y == 0 and flag == 3):
        return False, None
    return True, (v, y if larger1(y) == (flag == 3) else (-y) % Q)


def dec_g2c(b):
    flag = b[0] >> 6
    x1 = int.from_bytes(b[:32], "big") & ((1 << 254) - 1)
    x0 = int.from_bytes(b[32:], "big")
    if flag == 1:
        return x0 == 0 and x1 == 0, None
    if flag == 0 or x0 >= Q or x1 >= Q:      # x0 >= q covers a bit set in the top two of byte 32
        return False, None
    y = fq2_sqrt(g2_rhs((x0, x1)))
    if y is None or (y == (0, 0) and flag == 3):
        return False, None
    return True, ((x0, x1), y if larger2(y) == (flag == 3) else fq2_neg(y))


def dec_g1u(b):
    """a 65-byte block: tag, range, curve"""
    if b[0] == 0:
        return not any(b[1:]), None
    if b[0] != 4:
        return False, None
    x, y = int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:], "big")
    return x < Q and y < Q and (y * y - g1_rhs(x)) % Q == 0, (x, y)


def dec_g2u(b):
    """a 129-byte block: tag, range, the twist's equation -- NOT the subgroup"""
    if b[0] == 0:
        return not any(b[1:]), None
    if b[0] != 4:
        return False, None
    x1, x0, y1, y0 = (int.from_bytes(b[1 + 32 * i:33 + 32 * i], "big") for i in range(4))
    ok = max(x0, x1, y0, y1) < Q and fq2_sub(fq2_mul((y0, y1), (y0, y1)), g2_rhs((x0, x1))) == (0, 0)
    return ok, ((x0, x1), (y0, y1))


def compress(p):
    """259 -> 128 bytes, None when the library must refuse"""
    (oa, A), (ob, B), (oc, C) = dec_g1u(p[:65]), dec_g2u(p[65:194]), dec_g1u(p[194:])
    return enc_g1c(A) + enc_g2c(B) + enc_g1c(C) if oa and ob and oc else None


def decompress(c):
    """128 -> 259 bytes, None when the library must refuse"""
    (oa, A), (ob, B), (oc, C) = dec_g1c(c[:32]), dec_g2c(c[32:96]), dec_g1c(c[96:])
    return pyref.enc_proof(A, B, C) if oa and ob and oc else None


def malformed_compressed(honest):
    """one 128-byte string of every refusal class, made from an honest compressed proof: [(name, bytes)]"""
    a, b, c = honest[:32], honest[32:96], honest[96:]
    flagged = lambda v, f: bytes([(v >> 248) | f]) + (v & ((1 << 248) - 1)).to_bytes(31, "big")   # noqa: E731
    out = [("A flag 00", bytes([a[0] & 0x3F]) + a[1:] + b + c),
           ("A all zero", bytes(32) + b + c),
           ("B all zero", a + bytes(64) + c),
           ("B flag 00", a + bytes([b[0] & 0x3F]) + b[1:] + c),
           ("A infinity with a low bit", b"\x40" + bytes(30) + b"\x01" + b + c),
           ("C infinity with a bit in byte 0", a + b + b"\x41" + bytes(31)),
           ("B infinity with a bit in x.c0", a + b"\x40" + bytes(62) + b"\x80" + c),
           ("B flag bit in byte 32", a + b[:32] + bytes([b[32] | 0x80]) + b[33:] + c),
           ("B x.c0 = q", a + b[:32] + Q.to_bytes(32, "big") + c),
           ("B x.c1 = q", a + flagged(Q, 0x80) + b[32:] + c)]
    for name, v in (("q", Q), ("q + 1", Q + 1), ("2^254 - 1", (1 << 254) - 1)):
        out.append(("A x = %s flag 10" % name, flagged(v, 0x80) + b + c))
        out.append(("C x = %s flag 11" % name, a + b + flagged(v, 0xC0)))
    x = next(v for v in range(2, 100) if fq_sqrt(g1_rhs(v)) is None)
    out.append(("A x on no point", flagged(x, 0x80) + b + c))
    x = next((0, v) for v in range(1, 100) if fq2_sqrt(g2_rhs((0, v))) is None)
    out.append(("B x on no point", a + enc_g2c((x, (1, 0)))[:64] + c))
    assert all(decompress(s) is None for _, s in out)
    return out


def malformed_uncompressed(honest):
    """one 259-byte string of every class zk_proof_compress refuses: [(name, bytes)]"""
    a, b, c = honest[:65], honest[65:194], honest[194:]
    out = [("A off the curve", b"\x04" + (1).to_bytes(32, "big") + (3).to_bytes(32, "big") + b + c),
           ("A unknown tag", b"\x02" + a[1:] + b + c),
           ("C infinity tag over a point", a + b + b"\x00" + c[1:]),
           ("B tag 0xFF", a + b"\xff" + b[1:] + c),
           ("B y.c0 changed", a + b[:128] + bytes([b[128] ^ 1]) + c),
           ("A x = x + q", b"\x04" + (int.from_bytes(a[1:33], "big") + Q).to_bytes(32, "big") + a[33:] + b + c),
           ("all 0xFF", BAD_DECOMPRESSED)]
    assert all(compress(s) is None for _, s in out)
    return out
