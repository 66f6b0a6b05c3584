"""-m "not gpu": the host side of a delta contribution (csrc/crs_contribution.hip) -- the record (zk_crs_contribution_prove /
_verify) against a Python restatement (hashlib.sha256, Python integers, the oracle's group operations), the GLV split and the width-4
recoding of the one scalar of k_g1_scale against Python integers, the model of zk_crs_contribution_check
(tests/crs_contribute_model.py) tied to the ORACLE's setup, and the same host code as a stand-alone program under ASan + UBSan.
No GPU and no context anywhere.  Bytes and bits only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import Contribution, SplitMix64, ZkError, _lib, contribution_prove, ints_to_limbs, limbs_to_int
from zksnark_rs_amd.circuits import chain_rows

import crs_check_model as ccm
import crs_contribute_model as cm
from test_arbitrary_roots import dense_from_rows, root_poly
from test_crs_check_model import build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = zk.R_MODULUS
LAM = cm.LAMBDA
DIGITS, WORDS = 132, 3 + 2 * 132      # ZK_GLV_RECODE_DIGITS, ZK_GLV_RECODE_WORDS (include/zkgpu_measure.h)
GLV_RECODE = 9                        # ZK_LAZY_GLV_RECODE


@pytest.fixture(scope="module")
def grp(orc):
    return ccm.Groups(orc)


def fixed_scalars():
    return [0, 1, LAM, LAM + 1, LAM - 1, R - 1, (R - 1) // 2, 1 << 127, (1 << 128) - 1, 1 << 128, 1 << 253]


def drawn_scalars(count, seed=61000):
    rng = SplitMix64(seed)
    return [rng.fr() for _ in range(count)]


def recode(scalars):
    """[(|k1|, |k2|, neg1, neg2, top, digits1, digits2)] through the test accessor (host code: the context is NULL)"""
    lib = _lib.load()
    n = len(scalars)
    k32 = np.ascontiguousarray(ints_to_limbs(scalars).reshape(n, 4)).view(np.uint32).view(np.int32).copy()
    out = np.zeros((n, 4), np.uint64)
    raw = np.zeros((n, WORDS), np.int32)
    rc = lib.zk_lazy29_batch(None, 0, GLV_RECODE, k32.ctypes.data_as(_lib.i32p), None, None, None, n, out.ctypes.data_as(_lib.u64p),
                             raw.ctypes.data_as(_lib.i32p))
    assert rc == 0
    res = []
    for i in range(n):
        res.append((limbs_to_int(out[i, :2]), limbs_to_int(out[i, 2:]), bool(raw[i, 0]), bool(raw[i, 1]), int(raw[i, 2]),
                    [int(x) for x in raw[i, 3:3 + DIGITS]], [int(x) for x in raw[i, 3 + DIGITS:]]))
    return res


# ---- the scalar preparation ------------------------------------------------------------------------------------------------------
def test_glv_split_and_recoding_against_python_integers():
    scalars = fixed_scalars() + drawn_scalars(1000)
    signs = set()
    for k, (m1, m2, n1, n2, top, d1, d2) in zip(scalars, recode(scalars)):
        k1, k2 = (-m1 if n1 else m1), (-m2 if n2 else m2)
        assert (k1, k2) == cm.glv_split(k), hex(k)                      # the host restatement is the Python split
        assert (k1 + k2 * LAM - k) % R == 0, hex(k)
        assert m1 < (1 << 127) + (1 << 65) and m2 < (1 << 127) + (1 << 65), hex(k)   # the stated bound
        for half, digits in ((k1, d1), (k2, d2)):
            assert sum(d << i for i, d in enumerate(digits)) == half, hex(k)      # the digits recompose, sign included
            assert all(d == 0 or (d % 2 == 1 and -7 <= d <= 7) for d in digits), hex(k)
            nz = [i for i, d in enumerate(digits) if d]
            assert all(b - a >= 4 for a, b in zip(nz, nz[1:])), hex(k)            # non-adjacent form of width 4
        nz = [i for i in range(DIGITS) if d1[i] or d2[i]]
        assert top == (nz[-1] if nz else -1) and top <= 128, hex(k)
        signs.add((k1 < 0, k2 < 0))
    assert len(signs) == 4                                              # every sign combination of (k1, k2) occurred


def test_recoding_density_is_what_the_kernel_is_costed_with():
    """about 52 mixed additions: 2 x 128 / 5 non-zero digits on average (arithmetic, not a measurement)"""
    rec = recode(drawn_scalars(400, 62000))
    mean = sum(sum(1 for d in r[5] + r[6] if d) for r in rec) / len(rec)
    assert 48 < mean < 56, mean


# ---- the record --------------------------------------------------------------------------------------------------------------------
def some_delta(grp, seed):
    return grp.mul1(grp.orc.enc_base_g1(), SplitMix64(seed).fr())


TAGS = [None, bytes([0xFF]) * 32, bytes(SplitMix64(63000).next() & 0xFF for _ in range(32))]


@pytest.mark.parametrize("tag", TAGS, ids=["none", "ff", "random"])
def test_known_answer_records(grp, tag):
    rng = SplitMix64(63100)
    delta = some_delta(grp, 63101)
    for d in (1, 2, R - 1, rng.fr()):
        nonce = rng.fr()
        rec = contribution_prove(delta, d, nonce=nonce, tag=tag)
        assert rec.to_bytes() == cm.record_bytes(grp, delta, d, nonce, tag), d
        assert len(rec.to_bytes()) == 224 and Contribution.from_bytes(rec.to_bytes()) == rec
        assert rec.verify(tag) and cm.verify(grp, rec, tag)
        # the verification equation with the oracle's groups, spelt out: z delta_before = T + c delta_after
        c = cm.challenge(tag, rec.delta_before_g1, rec.delta_after_g1, rec.commit_g1)
        assert np.array_equal(grp.mul1(rec.delta_before_g1, rec.response), grp.add1(rec.commit_g1, grp.mul1(rec.delta_after_g1, c)))
    assert contribution_prove(delta, 5, tag=tag).verify(tag)          # nonce from the OS
    assert contribution_prove(delta, 5, tag=tag).to_bytes() != contribution_prove(delta, 5, tag=tag).to_bytes()


def with_field(rec, offset_words, values):
    raw = np.frombuffer(rec.to_bytes(), dtype="<u8").copy()
    raw[offset_words:offset_words + len(values)] = values
    return Contribution.from_bytes(raw.tobytes())


def test_altered_records_are_rejected(grp):
    tag = TAGS[2]
    delta = some_delta(grp, 63200)
    rec = contribution_prove(delta, 77, nonce=99, tag=tag)
    assert rec.verify(tag)
    flipped = bytearray(tag)
    flipped[31] ^= 0x80
    bad = {"a flipped tag bit": (rec, bytes(flipped)), "no tag": (rec, None)}
    bad["a flipped response word"] = (with_field(rec, 26, [int(np.frombuffer(rec.to_bytes(), "<u8")[26]) ^ 1]), tag)
    bad["before and after swapped"] = (with_field(with_field(rec, 0, rec.delta_after_g1), 8, rec.delta_before_g1), tag)
    bad["T replaced"] = (with_field(rec, 16, grp.add1(rec.commit_g1, delta)), tag)
    bad["response = r"] = (with_field(rec, 24, ints_to_limbs([R]).reshape(4)), tag)
    off = rec.delta_after_g1.copy()
    off[4] ^= 1
    bad["an off-curve delta_after"] = (with_field(rec, 8, off), tag)
    bad["an infinity delta_after"] = (with_field(rec, 8, np.zeros(8, np.uint64)), tag)
    bad["an infinity delta_before"] = (with_field(rec, 0, np.zeros(8, np.uint64)), tag)
    big = rec.commit_g1.copy()
    big[:4] = ints_to_limbs([cm.Q]).reshape(4)
    bad["a coordinate = q"] = (with_field(rec, 16, big), tag)
    for name, (r_, t_) in bad.items():
        assert not r_.verify(t_), name
        assert not cm.verify(grp, r_, t_), name


def test_prove_statuses(grp):
    lib = _lib.load()
    delta = some_delta(grp, 63300)
    out = _lib.CrsContribution()
    before = bytes(bytearray(out))
    p = lambda a: np.ascontiguousarray(a, np.uint64).ctypes.data_as(_lib.u64p)   # noqa: E731
    one, zero, big = ints_to_limbs([1]).reshape(4), ints_to_limbs([0]).reshape(4), ints_to_limbs([R]).reshape(4)
    assert lib.zk_crs_contribution_prove(None, p(one), None, None, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_crs_contribution_prove(p(delta), None, None, None, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_crs_contribution_prove(p(delta), p(one), None, None, None) == _lib.ZK_ERR_ARG
    assert lib.zk_crs_contribution_prove(p(delta), p(zero), None, None, C.byref(out)) == _lib.ZK_ERR_DIV_BY_ZERO
    assert lib.zk_crs_contribution_prove(p(delta), p(big), None, None, C.byref(out)) == _lib.ZK_ERR_RANGE
    assert lib.zk_crs_contribution_prove(p(delta), p(one), p(big), None, C.byref(out)) == _lib.ZK_ERR_RANGE
    assert lib.zk_crs_contribution_prove(p(np.zeros(8, np.uint64)), p(one), None, None, C.byref(out)) == _lib.ZK_ERR_RANGE
    assert bytes(bytearray(out)) == before                                  # untouched on every failure
    ok = C.c_int(7)
    assert lib.zk_crs_contribution_verify(None, None, C.byref(ok)) == _lib.ZK_ERR_ARG
    assert lib.zk_crs_contribution_verify(C.byref(out), None, None) == _lib.ZK_ERR_ARG
    with pytest.raises(ZkError):
        contribution_prove(delta, 0)
    with pytest.raises(ValueError):
        Contribution.from_bytes(bytes(223))


# ---- the model of the check, tied to the oracle's setup --------------------------------------------------------------------------------
def oracle_setup(orc, recipe, td):
    """the oracle's CRS arrays for the QAP of a build_case recipe and the trapdoor td (ints)"""
    kind, args = recipe
    tdl = ints_to_limbs(td)
    if kind == "unity":
        log_n, m, l, u, v, w = args
        return orc.setup_sparse(zk.Context.sparse_desc(log_n, m, l, u, v, w), tdl, 1 << log_n, m, l, True)
    if kind == "dense":
        du, dv, dw, dt, l = args
        return orc.setup_dense(du, dv, dw, dt, l, tdl)
    roots_or_n, m, l, u, v, w = args
    roots = list(range(1, roots_or_n + 1)) if kind == "integers" else [limbs_to_int(r) for r in roots_or_n]
    return orc.setup_dense(dense_from_rows(roots, u, m), dense_from_rows(roots, v, m), dense_from_rows(roots, w, m), root_poly(roots), l, tdl)


# roots of unity need a power of two: 4 stands where the other kinds take 5
MODEL_CASES = [("unity", n) for n in (1, 2, 4)] + [(kind, n) for kind in ("dense", "integers", "arbitrary") for n in (1, 2, 5)]


@pytest.mark.parametrize("kind,n", MODEL_CASES)
def test_model_accepts_the_oracles_successor_and_names_every_alteration(orc, grp, kind, n):
    before, _, td, recipe = build_case(orc, kind, n)
    rng = SplitMix64(64000 + n)
    d, s, tag = rng.fr(), rng.fr(), TAGS[2]
    td2 = list(td)
    td2[3] = td[3] * d % R
    after = oracle_setup(orc, recipe, td2)
    assert all(np.array_equal(before[k], oracle_setup(orc, recipe, td)[k]) for k in before)      # the recipe is build_case's QAP
    mine = cm.successor(grp, before, d)
    assert all(np.array_equal(after[k], mine[k]) for k in after), "d^-1 on sum_delta and xi_t, d on the deltas, is setup's CRS"
    rec = contribution_prove(before["delta_g1"], d, nonce=rng.fr(), tag=tag)
    assert cm.check(grp, before, after, rec, tag, s) == 0
    assert cm.check(grp, before, after, rec, tag, rng.fr()) == 0
    for name, b, a, r_, t_, bits in cm.alterations(grp, before, after, rec, tag, d):
        assert cm.check(grp, b, a, r_, t_, s) == bits, (name, kind, n)


# ---- the same host code under the sanitizers ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("contrib_host") / "crs_contribution_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "crs_contribution_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


def test_host_code_under_sanitizers(grp, host_exe):
    """tests/cpp/crs_contribution_host.hip: csrc/crs_contribution.hip (SHA-256, the recoding, prove / verify) compiled alone for the
    host with ASan + UBSan as a stand-alone program; never loaded into Python, never run on a GPU.  Its record for a fixed nonce is the
    Python restatement's, byte for byte."""
    delta, d, nonce, tag = some_delta(grp, 65000), 0x1234567, 0x7654321, TAGS[2]
    hexw = lambda a: np.asarray(a, np.uint64).astype("<u8").tobytes().hex()   # noqa: E731
    req = "%s\n%s\n%s\n%s\n" % (hexw(delta), hexw(ints_to_limbs([d])), hexw(ints_to_limbs([nonce])), tag.hex())
    res = subprocess.run([host_exe], input=req, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[0] == "record " + cm.record_bytes(grp, delta, d, nonce, tag).hex()
    assert lines[1] == "verify 1 tampered 0 malformed 0"
    assert lines[2].startswith("recoded ") and int(lines[2].split()[1]) >= 1000
    assert lines[3] == "sha256 ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"     # FIPS 180-4, "abc"
