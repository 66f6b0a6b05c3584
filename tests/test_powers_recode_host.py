"""-m "not gpu": the host side of a powers-of-tau contribution.  The split and the REGULAR signed-window recoding every lane of
k_mul_each does for its own scalar (csrc/mul_each_recode.hpp, the same functions compiled for the host, reached through the test
accessor ZK_LAZY_REGULAR_RECODE of zk_lazy29_batch) against Python integers; the three-part record (zk_powers_contribution_prove /
_verify) against a Python restatement with hashlib; and the same host code as a stand-alone program under ASan + UBSan.  No GPU and no
context anywhere."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import PowersContribution, SplitMix64, ZkError, _lib, ints_to_limbs, limbs_to_int, powers_contribution_prove, powers_role_tag

import crs_check_model as ccm
import crs_contribute_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = zk.R_MODULUS
LAM = cm.LAMBDA
SLOTS, WORDS = _lib.REGULAR_RECODE_DIGITS, _lib.REGULAR_RECODE_WORDS
WIDTH = {0: 4, 1: 3}              # field -> window width: ME_W_G1, ME_W_G2 (csrc/mul_each_recode.hpp)
DIGITS = {0: 32, 1: 43}           # RegularRecode<W>::ND


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def edge_scalars():
    """the issue's list: the ends, lambda's neighbourhood, the powers of two around the halves' width, scalars whose k1 or k2 is 0"""
    fixed = [0, 1, 2, LAM, LAM + 1, LAM - 1, R - LAM, R - 1, R - 2, (R - 1) // 2, 1 << 127, (1 << 128) - 1, 1 << 128, 1 << 253]
    return fixed + [j * LAM % R for j in range(1, 17)] + list(range(1, 17))


def drawn_scalars(count, seed=81000):
    rng = SplitMix64(seed)
    return [rng.fr() for _ in range(count)]


def recode(scalars, field):
    """[(|k1|, |k2|, neg1, neg2, even1, even2, nd, digits1, digits2)] through the test accessor (host code: the context is NULL)"""
    lib = _lib.load()
    n = len(scalars)
    k32 = np.ascontiguousarray(ints_to_limbs(scalars).reshape(n, 4)).view(np.uint32).view(np.int32).copy()
    out = np.zeros((n, 4), np.uint64)
    raw = np.full((n, WORDS), 0x55555555, np.int32)
    rc = lib.zk_lazy29_batch(None, field, _lib.LAZY_REGULAR_RECODE, k32.ctypes.data_as(_lib.i32p), None, None, None, n,
                             out.ctypes.data_as(_lib.u64p), raw.ctypes.data_as(_lib.i32p))
    assert rc == 0
    res = []
    for i in range(n):
        res.append((limbs_to_int(out[i, :2]), limbs_to_int(out[i, 2:]), bool(raw[i, 0]), bool(raw[i, 1]), bool(raw[i, 2]), bool(raw[i, 3]),
                    int(raw[i, 4]), [int(x) for x in raw[i, 5:5 + SLOTS]], [int(x) for x in raw[i, 5 + SLOTS:]]))
    return res


def check_recoding(scalars, field):
    w, nd_want = WIDTH[field], DIGITS[field]
    signs, evens = set(), set()
    for k, (m1, m2, n1, n2, e1, e2, nd, d1, d2) in zip(scalars, recode(scalars, field)):
        k1, k2 = (-m1 if n1 else m1), (-m2 if n2 else m2)
        assert (k1 + k2 * LAM - k) % R == 0, hex(k)
        assert (k1, k2) == cm.glv_split(k), hex(k)                           # the nearest-rounding split of the library
        assert m1 < (1 << 127) + (1 << 65) and m2 < (1 << 127) + (1 << 65), hex(k)
        assert nd == nd_want, "the digit count is fixed"
        for m, even, digits in ((m1, e1, d1), (m2, e2, d2)):
            assert even == (m % 2 == 0), hex(k)
            used, rest = digits[:nd], digits[nd:]
            assert all(d == 0 for d in rest), hex(k)
            assert all(d % 2 == 1 and -(1 << w) < d < (1 << w) for d in used), (hex(k), used)      # every digit odd, non-zero, in range
            assert sum(d << (w * i) for i, d in enumerate(used)) == m + (1 if even else 0), hex(k)  # recomposes to the (odd) magnitude
        signs.add((n1, n2))
        evens.add((e1, e2))
    return signs, evens


@pytest.mark.parametrize("field", [0, 1], ids=["g1_w4", "g2_w3"])
def test_edge_scalars_split_and_recode(field):
    scalars = edge_scalars()
    check_recoding(scalars, field)
    rec = dict(zip(scalars, recode(scalars, field)))
    assert rec[0][:2] == (0, 0) and rec[0][4:6] == (True, True)
    for j in range(1, 17):
        assert rec[j * LAM % R][0] == 0 and rec[j * LAM % R][1] == j          # k1 = 0
        assert rec[j][0] == j and rec[j][1] == 0                              # k2 = 0
    # a zero half is recoded as 1: the top digit 1, every other digit -(2^W - 1)
    w, nd = WIDTH[field], DIGITS[field]
    assert rec[0][7][:nd] == [-(2 ** w - 1)] * (nd - 1) + [1]


@pytest.mark.parametrize("field", [0, 1], ids=["g1_w4", "g2_w3"])
def test_drawn_scalars_split_and_recode(field):
    signs, evens = check_recoding(drawn_scalars(10000), field)
    assert len(signs) == 4 and len(evens) == 4       # every sign and every parity combination of (k1, k2) occurred


def test_accessor_statuses():
    lib = _lib.load()
    k = np.zeros(8, np.int32)
    out, raw = np.zeros(4, np.uint64), np.zeros(WORDS, np.int32)
    p32, p64 = (lambda a: a.ctypes.data_as(_lib.i32p)), (lambda a: a.ctypes.data_as(_lib.u64p))
    assert lib.zk_lazy29_batch(None, 0, _lib.LAZY_REGULAR_RECODE, None, None, None, None, 1, p64(out), p32(raw)) == _lib.ZK_ERR_ARG
    assert lib.zk_lazy29_batch(None, 2, _lib.LAZY_REGULAR_RECODE, p32(k), None, None, None, 1, p64(out), p32(raw)) == _lib.ZK_ERR_ARG
    assert lib.zk_lazy29_batch(None, 0, _lib.LAZY_REGULAR_RECODE, p32(k), None, None, None, 1, p64(out), None) == _lib.ZK_ERR_ARG


# ---- the record --------------------------------------------------------------------------------------------------------------------
TAGS = [None, bytes([0xFF]) * 32, bytes(SplitMix64(83000).next() & 0xFF for _ in range(32))]


def some_points(grp, seed):
    rng = SplitMix64(seed)
    g = grp.orc.enc_base_g1()
    return np.stack([grp.mul1(g, rng.fr()) for _ in range(3)])


def record_bytes(grp, before, secrets, nonces, tag):
    """the Python restatement: three of crs_contribute_model's records, each under SHA-256("ZKPOWv1\\0" | role | tag)"""
    out = b""
    for role in (1, 2, 3):
        role_tag = hashlib.sha256(b"ZKPOWv1\0" + bytes([role]) + (tag if tag is not None else bytes(32))).digest()
        out += cm.record_bytes(grp, before[role - 1], secrets[role - 1], nonces[role - 1], role_tag)
    return out


@pytest.mark.parametrize("tag", TAGS, ids=["none", "ff", "random"])
def test_known_answer_records(grp, tag):
    rng = SplitMix64(83100)
    before = some_points(grp, 83101)
    for secrets in ((1, 1, 1), (2, R - 1, (R - 1) // 2), (rng.fr(), rng.fr(), rng.fr())):
        nonces = (rng.fr(), rng.fr(), rng.fr())
        rec = powers_contribution_prove(before, secrets, nonces=nonces, tag=tag)
        assert rec.to_bytes() == record_bytes(grp, before, secrets, nonces, tag), secrets
        assert len(rec.to_bytes()) == 672 and PowersContribution.from_bytes(rec.to_bytes()) == rec
        assert rec.verify(tag)
        for role, part in ((1, rec.tau), (2, rec.alpha), (3, rec.beta)):
            assert powers_role_tag(role, tag) == hashlib.sha256(b"ZKPOWv1\0" + bytes([role]) + (tag or bytes(32))).digest()
            assert part.verify(powers_role_tag(role, tag)) and cm.verify(grp, part, powers_role_tag(role, tag))
            assert np.array_equal(part.delta_before_g1, before[role - 1])
            assert np.array_equal(part.delta_after_g1, grp.mul1(before[role - 1], secrets[role - 1]))
    assert powers_contribution_prove(before, (5, 6, 7), tag=tag).verify(tag)          # nonces from the OS
    assert powers_contribution_prove(before, (5, 6, 7), tag=tag).to_bytes() != powers_contribution_prove(before, (5, 6, 7), tag=tag).to_bytes()


def test_wrong_role_wrong_tag_and_swapped_roles_are_refused(grp):
    tag = TAGS[2]
    before = some_points(grp, 83200)
    rec = powers_contribution_prove(before, (11, 22, 33), nonces=(44, 55, 66), tag=tag)
    assert rec.verify(tag)
    flipped = bytearray(tag)
    flipped[31] ^= 0x80
    assert not rec.verify(bytes(flipped)) and not rec.verify(None)
    raw = rec.to_bytes()
    parts = [raw[224 * i:224 * (i + 1)] for i in range(3)]
    for order in ((1, 0, 2), (0, 2, 1), (2, 1, 0), (1, 2, 0)):                     # every part verifies only in its own role
        assert not PowersContribution.from_bytes(b"".join(parts[i] for i in order)).verify(tag), order
    # a part proved under the PLAIN tag (zk_crs_contribution_prove's binding, no role) is refused in every role
    plain = zk.contribution_prove(before[0], 11, nonce=44, tag=tag)
    assert plain.verify(tag)
    assert not PowersContribution.from_bytes(plain.to_bytes() + parts[1] + parts[2]).verify(tag)
    # and a record under another role's tag: the tau part re-proved as role 2
    as_alpha = zk.contribution_prove(before[0], 11, nonce=44, tag=powers_role_tag(2, tag))
    assert not PowersContribution.from_bytes(as_alpha.to_bytes() + parts[1] + parts[2]).verify(tag)
    one_bit = bytearray(raw)
    one_bit[224 + 200] ^= 1                                                         # a response word of the alpha part
    assert not PowersContribution.from_bytes(bytes(one_bit)).verify(tag)


def test_prove_statuses(grp):
    lib = _lib.load()
    before = some_points(grp, 83300).reshape(24)
    out = _lib.PowersContribution()
    untouched = bytes(bytearray(out))
    p = lambda a: np.ascontiguousarray(a, np.uint64).ctypes.data_as(_lib.u64p)   # noqa: E731
    ones, with_zero, with_big = ints_to_limbs([1, 1, 1]), ints_to_limbs([1, 0, 1]), ints_to_limbs([1, 1, R])
    assert lib.zk_powers_contribution_prove(None, p(ones), None, None, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_contribution_prove(p(before), None, None, None, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_contribution_prove(p(before), p(ones), None, None, None) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_contribution_prove(p(before), p(with_zero), None, None, C.byref(out)) == _lib.ZK_ERR_DIV_BY_ZERO
    assert lib.zk_powers_contribution_prove(p(before), p(with_big), None, None, C.byref(out)) == _lib.ZK_ERR_RANGE
    assert lib.zk_powers_contribution_prove(p(before), p(ones), p(with_big), None, C.byref(out)) == _lib.ZK_ERR_RANGE
    off = before.copy()
    off[4] ^= 1
    assert lib.zk_powers_contribution_prove(p(off), p(ones), None, None, C.byref(out)) == _lib.ZK_ERR_RANGE   # off the curve
    assert bytes(bytearray(out)) == untouched                                  # untouched on every failure
    ok = C.c_int(7)
    assert lib.zk_powers_contribution_verify(None, None, C.byref(ok)) == _lib.ZK_ERR_ARG
    assert lib.zk_powers_contribution_verify(C.byref(out), None, None) == _lib.ZK_ERR_ARG
    # an infinity before-point: that part stays zero and never verifies; the other two do
    inf = before.copy()
    inf[:8] = 0
    rec = powers_contribution_prove(inf, (3, 4, 5))
    assert rec.tau.to_bytes() == bytes(224) and not rec.verify() and rec.alpha.verify(powers_role_tag(2)) and rec.beta.verify(powers_role_tag(3))
    with pytest.raises(ZkError):
        powers_contribution_prove(before, (1, 0, 1))
    with pytest.raises(ValueError):
        PowersContribution.from_bytes(bytes(671))


# ---- the same host code under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("powers_host") / "powers_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "powers_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


def test_host_code_under_sanitizers(grp, host_exe):
    """tests/cpp/powers_host.hip: csrc/powers_record.hip, csrc/crs_contribution.hip and csrc/mul_each_recode.hpp compiled alone for the
    host with ASan + UBSan as a stand-alone program; never loaded into Python, never run on a GPU.  Its record for fixed nonces is the
    Python restatement's, byte for byte."""
    before, secrets, nonces, tag = some_points(grp, 85000), (0x1234567, 0x89abcde, 0xf012345), (0x7654321, 0x1357, 0x2468), TAGS[2]
    hexw = lambda a: np.asarray(a, np.uint64).astype("<u8").tobytes().hex()   # noqa: E731
    req = "%s\n%s\n%s\n%s\n" % (hexw(before.reshape(24)), hexw(ints_to_limbs(secrets)), hexw(ints_to_limbs(nonces)), tag.hex())
    res = subprocess.run([host_exe], input=req, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[0] == "record " + record_bytes(grp, before, secrets, nonces, tag).hex()
    assert lines[1] == "verify 1 wrongtag 0 swapped 0"
    assert lines[2] == "recoded 1200"
