"""-m "not gpu": zk_proof_compress / zk_proof_decompress (host code in libzkgpu.so, the same ZK_HD routines of csrc/point_codec.cuh
the decompress kernels run) against a big-integer model of the encoding (tests/proof_codec_model.py), byte for byte."""
import ctypes as C
import json
import os
import random

import pytest

import proof_codec_model as M
from proof_codec_model import Q, pyref
from zksnark_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROOFS = json.load(open(os.path.join(ROOT, "tests", "golden", "proofs.json")))
GOLDEN = [bytes.fromhex(c["proof"]) for c in PROOFS["cases"]]


def lib_compress(p):
    """(status, 128 bytes)"""
    assert len(p) == 259
    src = (C.c_uint8 * 259).from_buffer_copy(p)
    dst = (C.c_uint8 * 128)(*([0xAA] * 128))
    return _lib.load().zk_proof_compress(src, dst), bytes(dst)


def lib_decompress(c):
    """(status, 259 bytes)"""
    assert len(c) == 128
    src = (C.c_uint8 * 128).from_buffer_copy(c)
    dst = (C.c_uint8 * 259)(*([0xAA] * 259))
    return _lib.load().zk_proof_decompress(src, dst), bytes(dst)


def accepts(c, want):
    """c decompresses to exactly `want` and `want` compresses back to exactly c"""
    assert lib_decompress(c) == (_lib.ZK_OK, want), c.hex()
    assert lib_compress(want) == (_lib.ZK_OK, c), c.hex()


def refuses(c):
    assert lib_decompress(c) == (_lib.ZK_ERR_RANGE, M.BAD_DECOMPRESSED), c.hex()


def with_a(blk):
    return blk + M.INF_G2C + M.INF_G1C


def with_b(blk):
    return M.INF_G1C + blk + M.INF_G1C


def test_golden_proofs_round_trip():
    assert len(GOLDEN) >= 4
    for p in GOLDEN:
        want = M.compress(p)
        assert want is not None and len(want) == 128
        assert lib_compress(p) == (_lib.ZK_OK, want)
        assert lib_decompress(want) == (_lib.ZK_OK, p)
        assert M.decompress(want) == p
        assert lib_compress(lib_decompress(want)[1]) == (_lib.ZK_OK, want)


def test_g1_known_answers():
    one = bytes(31) + b"\x01"
    accepts(with_a(b"\x80" + one[1:]), pyref.enc_proof((1, 2), None, None))
    accepts(with_a(b"\xc0" + one[1:]), pyref.enc_proof((1, Q - 2), None, None))
    accepts(M.INF_PROOF_C, bytes(259))
    assert b"\x40" + bytes(31) == M.INF_G1C
    # x = 0 is on no point: 3 is a non-residue mod q
    assert pow(3, (Q - 1) // 2, Q) == Q - 1
    refuses(with_a(b"\x80" + bytes(31)))
    refuses(with_a(b"\xc0" + bytes(31)))
    # the same in slot C
    accepts(M.INF_G1C + M.INF_G2C + b"\xc0" + one[1:], pyref.enc_proof(None, None, (1, Q - 2)))


def test_refusals():
    honest = M.compress(GOLDEN[0])
    classes = M.malformed_compressed(honest)
    assert len(classes) >= 18
    for name, c in classes:
        assert lib_decompress(c) == (_lib.ZK_ERR_RANGE, M.BAD_DECOMPRESSED), name
    refuses(bytes(128))
    refuses(with_a(bytes(32)))
    refuses(with_b(bytes(64)))
    # 0x40 with any other bit set, in any byte
    for i in range(32):
        for bit in (0x01, 0x20) if i == 0 else (0x01, 0x80):
            blk = bytearray(M.INF_G1C)
            blk[i] |= bit
            refuses(with_a(bytes(blk)))
            refuses(M.INF_G1C + M.INF_G2C + bytes(blk))
    for i in range(64):
        for bit in (0x01, 0x20) if i == 0 else (0x01, 0x80):
            blk = bytearray(M.INF_G2C)
            blk[i] |= bit
            refuses(with_b(bytes(blk)))
    # x = q, q + 1, 2^254 - 1 under both finite flags, in G1 and in either half of G2
    gx = M.enc_g2c(pyref.G2_GEN)
    for v in (Q, Q + 1, (1 << 254) - 1):
        for f in (0x80, 0xC0):
            blk = bytearray(v.to_bytes(32, "big"))
            blk[0] |= f
            refuses(with_a(bytes(blk)))
            refuses(with_b(bytes(blk) + gx[32:]))              # x.c1 >= q
            refuses(with_b(gx[:32] + v.to_bytes(32, "big")))   # x.c0 >= q
    # x - q of a valid x must not be read as x: (1 + q) is out of range although 1 is on the curve
    refuses(with_a(bytes([0x80 | ((1 + Q) >> 248)]) + ((1 + Q) & ((1 << 248) - 1)).to_bytes(31, "big")))
    # a flag bit in byte 32 of an otherwise honest G2 block
    for bit in (0x80, 0x40, 0xC0):
        refuses(with_b(gx[:32] + bytes([gx[32] | bit]) + gx[33:]))
    accepts(with_b(gx), pyref.enc_proof(None, pyref.G2_GEN, None))
    # the first eight small x whose right-hand side is a non-residue
    bad = [x for x in range(64) if M.fq_sqrt(M.g1_rhs(x)) is None][:8]
    assert len(bad) == 8 and bad[0] == 0
    for x in bad:
        for f in (0x80, 0xC0):
            refuses(with_a(bytes([f]) + x.to_bytes(31, "big")))
    bad2 = [(x0, x1) for x1 in range(4) for x0 in range(16) if M.fq2_sqrt(M.g2_rhs((x0, x1))) is None][:8]
    assert len(bad2) == 8
    for x in bad2:
        for f in (0x80, 0xC0):
            refuses(with_b(bytes([f]) + x[1].to_bytes(31, "big") + x[0].to_bytes(32, "big")))


def test_random_g1_points_both_signs():
    """random x, the decodable half kept; the sign rule is on the canonical integer, which a sign taken on the Montgomery
    residue gets wrong for about half of these"""
    rng = random.Random(20260101)
    pts = []
    while len(pts) < 1000:
        x = rng.randrange(Q)
        if M.fq_sqrt(M.g1_rhs(x)) is not None:
            pts.append(x)
    seen = set()
    for i in range(0, len(pts), 2):
        for la, lc in ((False, True), (True, False)):
            A, Cc = M.g1_from_x(pts[i], la), M.g1_from_x(pts[i + 1], lc)
            assert M.larger1(A[1]) == la and M.larger1(Cc[1]) == lc
            c = M.enc_g1c(A) + M.INF_G2C + M.enc_g1c(Cc)
            assert c[0] >> 6 == (3 if la else 2) and c[96] >> 6 == (3 if lc else 2)
            accepts(c, pyref.enc_proof(A, None, Cc))
            seen.add((la, A[1] & 1))
    assert len(seen) == 4     # the sign is not the parity either


def random_twist_x(rng, count):
    out = []
    while len(out) < count:
        x = (rng.randrange(Q), rng.randrange(Q))
        if M.fq2_sqrt(M.g2_rhs(x)) is not None:
            out.append(x)
    return out


def test_random_twist_points_both_signs():
    rng = random.Random(20260102)
    rejected = 0
    for x in random_twist_x(rng, 256):
        for larger in (False, True):
            B = M.g2_from_x(x, larger)
            assert pyref.g2_on_curve(B) and M.larger2(B[1]) == larger
            accepts(with_b(M.enc_g2c(B)), pyref.enc_proof(None, B, None))
    while rejected < 32:      # and the other half: x on no twist point
        x = (rng.randrange(Q), rng.randrange(Q))
        if M.fq2_sqrt(M.g2_rhs(x)) is None:
            rejected += 1
            refuses(with_b(M.enc_g2c((x, (1, 0)))))
            refuses(with_b(M.enc_g2c((x, (Q - 1, 0)))))


def test_twist_points_with_a_zero_half_of_y():
    """y.c1 = 0 (the a.c1 == 0 branch of the Fq2 root with a square real part, and the sign rule's fallback to y.c0) and y.c0 = 0
    (the same branch with a non-square real part): x^3 + b' must be real, so solve Im(x^3) = -Im(b') for x.c0 given x.c1"""
    rng = random.Random(20260103)
    found = {"c1": 0, "c0": 0}
    tries = 0
    while min(found.values()) < 2:
        tries += 1
        assert tries < 200
        t = rng.randrange(1, Q)
        s = M.fq_sqrt((t * t * t - M.B2[1]) * pow(3 * t, -1, Q))     # 3 s^2 t - t^3 = -Im(b')
        if s is None:
            continue
        for x in ((s, t), ((-s) % Q, t)):
            rhs = M.g2_rhs(x)
            assert rhs[1] == 0 and rhs[0] != 0
            y = M.fq2_sqrt(rhs)
            kind = "c1" if y[1] == 0 else "c0"
            assert (y[0] == 0) != (y[1] == 0)
            found[kind] += 1
            for larger in (False, True):
                B = M.g2_from_x(x, larger)
                assert pyref.g2_on_curve(B) and (B[1][1] == 0 if kind == "c1" else B[1][0] == 0)
                c = with_b(M.enc_g2c(B))
                assert c[32] >> 6 == (3 if larger else 2)
                accepts(c, pyref.enc_proof(None, B, None))


def test_twist_point_outside_g2_is_accepted():
    """decompression and compression check the curve only; the subgroup test stays behind verify"""
    rng = random.Random(20260104)
    x = random_twist_x(rng, 1)[0]
    P = M.g2_from_x(x, True)
    assert pyref.g2_on_curve(P)
    assert pyref.g2_add(pyref.g2_mul(P, pyref.R - 1), P) is not None      # [r]P != infinity (g2_mul reduces its scalar mod r)
    G = pyref.G2_GEN
    assert pyref.g2_add(pyref.g2_mul(G, pyref.R - 1), G) is None
    accepts(with_b(M.enc_g2c(P)), pyref.enc_proof(None, P, None))


def test_compress_refuses_malformed_proofs():
    for name, p in M.malformed_uncompressed(GOLDEN[0]):
        assert lib_compress(p) == (_lib.ZK_ERR_RANGE, M.BAD_COMPRESSED), name
    p = GOLDEN[0]
    off = b"\x04" + (1).to_bytes(32, "big") + (3).to_bytes(32, "big") + p[65:]
    assert lib_compress(off) == (_lib.ZK_ERR_RANGE, bytes(128))


def test_decompress_fills_a_bad_string_with_ff():
    c = bytearray(M.compress(GOLDEN[1]))
    c[0] &= 0x3F
    assert lib_decompress(bytes(c)) == (_lib.ZK_ERR_RANGE, b"\xff" * 259)
    # one bad block is enough, whichever it is
    good = M.compress(GOLDEN[1])
    for cut in (good[:32] + bytes(64) + good[96:], good[:96] + bytes(32)):
        assert lib_decompress(cut) == (_lib.ZK_ERR_RANGE, b"\xff" * 259)


def test_null_pointers():
    lib = _lib.load()
    buf = (C.c_uint8 * 259)()
    assert lib.zk_proof_compress(None, buf) == _lib.ZK_ERR_ARG
    assert lib.zk_proof_compress(buf, None) == _lib.ZK_ERR_ARG
    assert lib.zk_proof_decompress(None, buf) == _lib.ZK_ERR_ARG
    assert lib.zk_proof_decompress(buf, None) == _lib.ZK_ERR_ARG
    assert lib.zk_proof_compress_batch(None, buf, 1, buf, None) == _lib.ZK_ERR_ARG
    assert lib.zk_proof_decompress_batch(None, buf, 1, buf, None) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch_compressed(None, None, None, 0, buf, 1, None) == _lib.ZK_ERR_ARG


def test_host_routines_under_sanitizers(tmp_path):
    """tests/cpp/point_codec_fuzz.hip: csrc/point_codec.cuh's host side as a stand-alone program under ASan + UBSan"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "point_codec_fuzz")
    subprocess.run([hipcc, "-O0", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "point_codec_fuzz.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=600)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("decompressed ") and "ERROR" not in res.stderr
