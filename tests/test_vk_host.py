"""-m "not gpu": the verifying key as a host object (csrc/vk.hip) -- zk_vk_create / zk_vk_verify / the ZKVKv1 byte form -- over the
CRSs of tests/golden/proofs.json, whose trapdoors are known: the key's points come from pyref.setup_with_trapdoor, and every
verdict is compared with the zk_pairing-based check of tests/test_verify_all_device_code.py.  No GPU and no context anywhere."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import _lib, ints_to_limbs
from test_verify_all_device_code import case, verdict, _points, g1_words, g2_words   # noqa: F401  (`case` is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGIC = b"ZKVKv1\0\0"


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & (2 ** 64 - 1)
    return h


def vk_bytes(l):
    return 24 + 8 * (56 + 8 * (l + 1))


def payload_of(s1, s2, l):
    words = g1_words(s1["alpha"]) + g2_words(s2["beta"]) + g2_words(s2["gamma"]) + g2_words(s2["delta"])
    for P in s1["sum_gamma"][:l + 1]:
        words += g1_words(P)
    return b"".join(struct.pack("<Q", w) for w in words)


def byte_form(payload, l):
    return MAGIC + struct.pack("<QQ", l, fnv1a(payload)) + payload


def key_of(vk):
    s1, s2, l = vk
    return zk.VerifyingKey.from_points(np.array(g1_words(s1["alpha"]), np.uint64), np.array(g2_words(s2["beta"]), np.uint64),
                                       np.array(g2_words(s2["gamma"]), np.uint64), np.array(g2_words(s2["delta"]), np.uint64),
                                       np.array([g1_words(P) for P in s1["sum_gamma"][:l + 1]], np.uint64))


def status_from_bytes(data):
    lib = _lib.load()
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    p = C.c_void_p(0x1234)
    rc = lib.zk_vk_from_bytes(buf, len(data), C.byref(p))
    if rc == 0:
        lib.zk_vk_free(p)
    else:
        assert not p.value          # *out = NULL on every failure
    return rc


def test_golden_proofs_and_tampered_ones_match_the_pairing_check(case):
    import pyref
    key = key_of(case["vk"])
    assert key.input == case["l"]
    row, p = case["row"], case["proof"]
    assert key.verify(row, p) and verdict(case["vk"], row, p)
    A, B, Cc = _points(p)
    tampered = [(row, p[194:] + p[65:194] + p[:65]),                                   # A and C swapped
                (row, pyref.enc_proof(A, B, pyref.g1_add(Cc, pyref.G1_GEN)))]          # C + G: well formed, wrong
    if case["l"]:
        bad_row = list(row); bad_row[0] = (bad_row[0] + 1) % pyref.R
        tampered.append((bad_row, p))                                                  # one input changed
    for r, q in tampered:
        want = verdict(case["vk"], r, q)
        assert not want and key.verify(r, q) == want
    for bit in (9, 300, 1000, 1600, 2000):                                             # one flipped bit: off the curve, rejected
        bad = bytearray(p); bad[bit // 8] ^= 1 << (bit % 8)
        assert not key.verify(row, bytes(bad))
    # further honest proofs for other input rows, simulated with the trapdoor
    for _ in range(2):
        r = [case["rng"].fr() for _ in range(case["l"])]
        q = case["simulate"](r)
        assert verdict(case["vk"], r, q) and key.verify(r, q)
        if case["l"]:
            assert not key.verify(row, q) or r == row


def test_rows_longer_and_shorter_than_l(case):
    """zip truncation as zk_verify documents: entries behind l are never read (not even range-checked); a short row sums fewer bases"""
    key = key_of(case["vk"])
    row, p, l = case["row"], case["proof"], case["l"]
    assert key.verify(list(row) + [zk.R_MODULUS + 5, 7], p)
    if l:
        short = list(row)[:l - 1]
        assert key.verify(short, p) == verdict(case["vk"], short, p)
        with pytest.raises(zk.ZkError) as e:
            key.verify([zk.R_MODULUS] + list(row)[1:], p)
        assert e.value.status == _lib.ZK_ERR_RANGE
        with pytest.raises(zk.ZkError) as e:
            key.verify(list(row)[:l - 1] + [2 ** 256 - 1], p)
        assert e.value.status == _lib.ZK_ERR_RANGE
    # a malformed proof is rejected before the inputs are looked at, as in zk_verify
    assert key.verify([zk.R_MODULUS] * l, b"\x07" + p[1:]) is False


def test_byte_form_round_trip_and_file(case, tmp_path):
    s1, s2, l = case["vk"]
    key = key_of(case["vk"])
    want = byte_form(payload_of(s1, s2, l), l)
    got = key.to_bytes()
    assert got == want and len(got) == vk_bytes(l) == _lib.load().zk_vk_bytes(l)
    again = zk.VerifyingKey.from_bytes(got)
    assert again.to_bytes() == got and again.input == l
    assert again.verify(case["row"], case["proof"])
    path = tmp_path / "key.zkvk"
    key.save(path)
    assert open(path, "rb").read() == got
    loaded = zk.VerifyingKey.load(path)
    assert loaded.to_bytes() == got and loaded.verify(case["row"], case["proof"])
    with pytest.raises(zk.ZkError) as e:
        zk.VerifyingKey.load(tmp_path / "missing.zkvk")
    assert e.value.status == _lib.ZK_ERR_IO


def _crafted_key_bytes(l):
    """a key of multiples of the generators with l inputs (no circuit behind it)"""
    import pyref
    sg = [pyref.g1_mul(pyref.G1_GEN, 3 + i) for i in range(l + 1)]
    s1 = dict(alpha=pyref.g1_mul(pyref.G1_GEN, 5), sum_gamma=sg)
    s2 = dict(beta=pyref.g2_mul(pyref.G2_GEN, 7), gamma=pyref.g2_mul(pyref.G2_GEN, 11), delta=pyref.g2_mul(pyref.G2_GEN, 13))
    return s1, s2, byte_form(payload_of(s1, s2, l), l)


@pytest.mark.parametrize("l", [0, 2, 257])
def test_length_formula(l):
    lib = _lib.load()
    assert lib.zk_vk_bytes(l) == vk_bytes(l)
    s1, s2, data = _crafted_key_bytes(l)
    assert len(data) == vk_bytes(l)
    key = zk.VerifyingKey.from_bytes(data)
    assert key.input == l and key.to_bytes() == data
    assert key_of((s1, s2, l)).to_bytes() == data


def test_malformed_byte_strings():
    import pyref
    from test_verify import twist_point_outside_g2
    IO, RANGE = _lib.ZK_ERR_IO, _lib.ZK_ERR_RANGE
    s1, s2, good = _crafted_key_bytes(2)
    assert status_from_bytes(good) == 0
    assert status_from_bytes(good[:-1]) == IO                      # truncated by one byte
    assert status_from_bytes(good + b"\0") == IO                   # one extra byte
    assert status_from_bytes(b"") == IO and status_from_bytes(good[:23]) == IO and status_from_bytes(good[:24]) == IO
    assert status_from_bytes(b"ZKVKv2\0\0" + good[8:]) == IO       # altered magic
    assert status_from_bytes(b"ZKCRSv1\0" + good[8:]) == IO
    bad = bytearray(good); bad[24 + 100] ^= 1
    assert status_from_bytes(bytes(bad)) == IO                     # altered payload byte: checksum
    bad = bytearray(good); bad[16] ^= 1
    assert status_from_bytes(bytes(bad)) == IO                     # altered checksum
    for l_claimed in (1, 3, 2 ** 61, 2 ** 64 - 1):                 # a header whose l does not match the length
        assert status_from_bytes(good[:8] + struct.pack("<Q", l_claimed) + good[16:]) == IO
    payload = good[24:]
    # a point moved off its curve, checksum recomputed: every slot in turn (alpha, sum_gamma_0, the last sum_gamma)
    for off in (0, 56 * 8, len(payload) - 64):
        moved = bytearray(payload); moved[off] ^= 1
        assert status_from_bytes(byte_form(bytes(moved), 2)) == RANGE
    for off in (8 * 8, 24 * 8, 40 * 8):                            # beta, gamma, delta
        moved = bytearray(payload); moved[off] ^= 1
        assert status_from_bytes(byte_form(bytes(moved), 2)) == RANGE
    # a coordinate == q
    over = bytearray(payload); over[0:32] = pyref.Q.to_bytes(32, "little")
    assert status_from_bytes(byte_form(bytes(over), 2)) == RANGE
    # a twist point outside G2 as gamma: on the curve, refused by the subgroup test
    P = twist_point_outside_g2(3)
    assert pyref.g2_on_curve(P)
    outside = payload_of(s1, dict(s2, gamma=P), 2)
    assert status_from_bytes(byte_form(outside, 2)) == RANGE
    with pytest.raises(zk.ZkError) as e:
        key_of((s1, dict(s2, gamma=P), 2))
    assert e.value.status == RANGE
    # infinity (all zero) is a legal point in every slot
    inf = bytes(len(payload))
    assert status_from_bytes(byte_form(inf, 2)) == 0


def test_null_pointers():
    lib = _lib.load()
    s1, s2, good = _crafted_key_bytes(1)
    key = zk.VerifyingKey.from_bytes(good)
    ARG = _lib.ZK_ERR_ARG
    p = C.c_void_p(0x55)
    buf = (C.c_uint8 * len(good)).from_buffer_copy(good)
    assert lib.zk_vk_create(None, C.byref(p)) == ARG and p.value == 0x55          # nothing written
    words = np.zeros(64, np.uint64)
    wp = words.ctypes.data_as(_lib.u64p)
    assert lib.zk_vk_create(C.byref(_lib.VkDesc(1, wp, wp, wp, wp, wp)), None) == ARG
    for hole in range(5):
        args = [wp] * 5
        args[hole] = None
        assert lib.zk_vk_create(C.byref(_lib.VkDesc(1, *args)), C.byref(p)) == ARG and p.value == 0x55
    assert lib.zk_vk_from_bytes(None, 10, C.byref(p)) == ARG and p.value == 0x55
    assert lib.zk_vk_from_bytes(buf, len(good), None) == ARG
    assert lib.zk_vk_load(None, C.byref(p)) == ARG and lib.zk_vk_load(b"/nonexistent", None) == ARG
    assert lib.zk_vk_save(None, b"/nonexistent") == ARG and lib.zk_vk_save(key.ptr, None) == ARG
    n = C.c_size_t(77)
    assert lib.zk_vk_dims(None, C.byref(n)) == ARG and n.value == 77 and lib.zk_vk_dims(key.ptr, None) == ARG
    out = (C.c_uint8 * len(good))(*([0xAA] * len(good)))
    assert lib.zk_vk_to_bytes(None, out, len(good)) == ARG and lib.zk_vk_to_bytes(key.ptr, None, len(good)) == ARG
    assert lib.zk_vk_to_bytes(key.ptr, out, len(good) - 1) == ARG and bytes(out) == b"\xaa" * len(good)
    ok = C.c_int(9)
    proof = (C.c_uint8 * 259)()
    x = ints_to_limbs([1])
    xp = x.ctypes.data_as(_lib.u64p)
    assert lib.zk_vk_verify(None, xp, 1, proof, C.byref(ok)) == ARG
    assert lib.zk_vk_verify(key.ptr, None, 1, proof, C.byref(ok)) == ARG
    assert lib.zk_vk_verify(key.ptr, xp, 1, None, C.byref(ok)) == ARG
    assert ok.value == 9
    assert lib.zk_vk_verify(key.ptr, xp, 1, proof, None) == ARG
    assert lib.zk_vk_verify(key.ptr, None, 0, proof, C.byref(ok)) == 0              # no inputs is legal
    lib.zk_vk_free(None)
    # the batch forms without a context
    assert lib.zk_vk_verify_batch(None, key.ptr, xp, 1, proof, 1, C.byref(ok)) == ARG
    assert lib.zk_vk_verify_batch_compressed(None, key.ptr, xp, 1, proof, 1, C.byref(ok)) == ARG
    assert lib.zk_vk_verify_batch_all(None, key.ptr, xp, 1, proof, 1, xp, C.byref(ok)) == ARG
    assert lib.zk_vk_input_sums(None, key.ptr, xp, 1, 1, 1, xp) == ARG
    assert lib.zk_vk_from_crs(None, None, C.byref(p)) == ARG and p.value == 0x55


def test_three_infinities_against_a_key_with_infinite_points():
    """259 zero bytes are a valid encoding (A = B = C = infinity): accepted iff e(alpha, beta) e(S, gamma) == 1"""
    import pyref
    s1, s2, _ = _crafted_key_bytes(1)
    assert not key_of((s1, s2, 1)).verify([4], bytes(259))
    flat = (dict(s1, alpha=None, sum_gamma=[None, None]), s2, 1)
    assert key_of(flat).verify([4], bytes(259))
    # sum_gamma_0 + x sum_gamma_1 = infinity for x = -3 / 4 ... here 3 G + x 4 G: x = -3 / 4 mod r
    x = (-3 * pow(4, -1, pyref.R)) % pyref.R
    assert key_of((dict(s1, alpha=None), s2, 1)).verify([x], bytes(259))
    assert not key_of((dict(s1, alpha=None), s2, 1)).verify([x + 1], bytes(259))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("vk_host") / "vk_host_fuzz")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "vk_host_fuzz.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


def test_host_code_under_sanitizers(case, fuzz_exe):
    """tests/cpp/vk_host_fuzz.hip: csrc/vk.hip compiled alone for the host with ASan + UBSan, as a stand-alone program, over
    malformed byte strings in exact-size heap buffers and two verifications; never loaded into Python, never run on a GPU"""
    s1, s2, l = case["vk"]
    good = byte_form(payload_of(s1, s2, l), l)
    row = b"".join(struct.pack("<Q", int(w)) for w in ints_to_limbs(list(case["row"])).reshape(-1)) if l else b""
    req = "%s\n%s\n%d %s\n" % (good.hex(), case["proof"].hex(), l, row.hex() or "-")
    res = subprocess.run([fuzz_exe], input=req, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == "verify 1 tampered 0", res.stdout
    assert lines[0].startswith("malformed ") and int(lines[0].split()[1]) >= 20
