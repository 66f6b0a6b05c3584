"""zk_verify_batch (csrc/verify_batch.hip): the verdict of every proof in a batch equals zk_verify's for the same proof and
inputs -- honest proofs from the GPU prover, tampered and malformed encodings, truncated input rows, batches larger than one
chunk, a call next to an outstanding proof ticket, and the Python, groth16 and C++ layers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ZK_DIR = os.path.join(ROOT, "tests", "golden", "zk")
CHUNK = 65536   # ZK_VERIFY_BATCH_CHUNK (include/zkgpu.h)


def wide_program(k):
    """a .zk program with k + 1 `verify` wires: the inputs a0..a(k-1) and their running product"""
    names = " ".join("a%d" % i for i in range(k))
    lines = ["(in %s)" % names, "(out y)", "(verify %s y)" % names, "", "(program"]
    prev = "a0"
    for i in range(1, k):
        out = "y" if i == k - 1 else "t%d" % i
        lines.append("    (= %s (* %s a%d))" % (out, prev, i))
        prev = out
    return "\n".join(lines) + ")"


def single(ctx, crs, rows, proofs):
    return np.array([ctx.verify(crs, r, p) for r, p in zip(rows, proofs)], dtype=bool)


@pytest.fixture(scope="module")
def simple(ctx):
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(open(os.path.join(ZK_DIR, "simple.zk")).read())
    weights = c.weights([3, 2, 4])
    qap = c.qap(ctx)
    rng = SplitMix64(2027)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    proofs = [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(4)]
    other = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    foreign = ctx.prove(other, qap, weights, rng.fr(), rng.fr())
    return dict(qap=qap, crs=crs, weights=weights, proofs=proofs, foreign=foreign)


def _program_proofs(ctx, code, inputs, count, seed, sparse=False):
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(code)
    weights = c.weights(inputs)
    qap = c.qap_sparse(ctx) if sparse else c.qap(ctx)
    rng = SplitMix64(seed)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    proofs = [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(count)]
    return crs, weights[1:1 + c.input], proofs


@pytest.mark.gpu
def test_honest_proofs_all_accepted(ctx, simple):
    from zksnark_rs_amd.circuit import Circuit
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    cases = [(simple["crs"], simple["weights"][1:3], simple["proofs"])]
    code = open(os.path.join(ZK_DIR, "deg_15.zk")).read()
    rng = SplitMix64(15)
    cases.append(_program_proofs(ctx, code, [rng.fr() for _ in range(Circuit(code).n_in)], 3, 16))
    log_n = 10
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    cases.append((crs, weights[1:1 + l], [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(3)]))
    cases.append(_program_proofs(ctx, wide_program(256), [rng.fr() for _ in range(256)], 2, 257, sparse=True))
    assert cases[-1][1].shape[0] >= 256
    for crs, x, proofs in cases:
        rows = np.repeat(x[None], len(proofs), axis=0)
        got = ctx.verify_batch(crs, rows, proofs)
        assert got.dtype == bool and got.all()
        assert np.array_equal(got, single(ctx, crs, rows, proofs))


def _tampered_batch(simple, seed):
    """(rows, proofs) of a mixed batch over simple.zk's CRS, shuffled"""
    import pyref
    from test_verify import twist_point_outside_g2, g2_mul_raw
    good = [2, 34]
    p0, p1 = simple["proofs"][0], simple["proofs"][1]
    B_out = twist_point_outside_g2(seed)
    B_in = g2_mul_raw(B_out, 2 * pyref.Q - pyref.R)       # cofactor cleared: in G2, but not the proof's B
    q_words = pyref.Q.to_bytes(32, "big")
    cases = [(good, p) for p in simple["proofs"]]
    cases += [([2, 25], p0), ([3, 34], p1),                # wrong public input
              (good, p0[194:] + p0[65:194] + p0[:65]),     # A and C swapped
              (good, simple["foreign"]),                   # made under another CRS
              (good, p0[:65] + pyref.enc_g2(B_out) + p0[194:]),
              (good, p0[:65] + pyref.enc_g2(B_in) + p0[194:])]
    for off, size in ((0, 65), (65, 129), (194, 65)):
        cases.append((good, p0[:off] + bytes(size) + p0[off + size:]))                         # infinity, zero tail
        cases.append((good, p0[:off] + b"\x00" + p0[off + 1:]))                                 # tag 0x00, non-zero tail
        cases.append((good, p0[:off] + b"\x04" + bytes(size - 1) + p0[off + size:]))           # tag 0x04 with (0, 0)
        for tag in (1, 2, 3, 5, 0xff):
            cases.append((good, p0[:off] + bytes([tag]) + p0[off + 1:]))                        # unknown tags
        cases.append((good, p0[:off + 1] + q_words + p0[off + 33:]))                           # a coordinate == q
    for bit in (0, 9, 300, 1000, 1600, 2000):
        bad = bytearray(p1); bad[bit // 8] ^= 1 << (bit % 8)
        cases.append((good, bytes(bad)))                                                       # a single flipped bit
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(cases))
    return [cases[i][0] for i in order], [cases[i][1] for i in order]


@pytest.mark.gpu
def test_mixed_shuffled_batch_matches_verify(ctx, simple):
    rows, proofs = _tampered_batch(simple, 5)
    got = ctx.verify_batch(simple["crs"], rows, proofs)
    want = single(ctx, simple["crs"], rows, proofs)
    assert np.array_equal(got, want)
    assert 4 <= want.sum() < len(want)


@pytest.mark.gpu
def test_input_rows_truncate_like_verify(ctx, simple):
    """n_inputs < l, = l, > l (l = 2), n_inputs = 0; an input >= r beyond l is ignored, as zk_verify ignores it"""
    crs, p = simple["crs"], simple["proofs"]
    R = zk.R_MODULUS
    for rows in ([[2]] * 4, [[2, 34]] * 4, [[2, 34, R + 5]] * 4, [[2, 34, 7, R]] * 4, [[]] * 4, [[2, 25, 1]] * 4):
        got = ctx.verify_batch(crs, rows, p)
        assert np.array_equal(got, single(ctx, crs, rows, p)), rows
    assert ctx.verify_batch(crs, [[2, 34, R + 5]] * 4, p).all()


@pytest.mark.gpu
def test_error_codes(ctx, simple):
    lib, crs, p = ctx.lib, simple["crs"], simple["proofs"]
    R = zk.R_MODULUS
    x = ints_to_limbs([2, 34, 2, R + 1, 2, 34])                      # proof 1's second input >= r, inside l
    pb = np.frombuffer(b"".join(p[:3]), dtype=np.uint8).copy()
    ok = np.full(3, 7, np.int32)
    okp = ok.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, x.ctypes.data_as(_lib.u64p), 2, pb.ctypes.data_as(_lib.u8p), 3, okp) == _lib.ZK_ERR_RANGE
    assert (ok == 0).all()
    with pytest.raises(zk.ZkError):
        ctx.verify_batch(crs, [[2, 34], [2, R], [2, 34]], p[:3])
    good = ints_to_limbs([2, 34] * 3)
    gp, pp = good.ctypes.data_as(_lib.u64p), pb.ctypes.data_as(_lib.u8p)
    assert lib.zk_verify_batch(None, crs.ptr, gp, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch(ctx.ptr, None, gp, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, gp, 2, None, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, gp, 2, pp, 3, None) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, None, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    ok[:] = 7
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, gp, 2, pp, 0, okp) == _lib.ZK_OK
    assert (ok == 7).all()
    assert lib.zk_verify_batch(ctx.ptr, crs.ptr, None, 0, pp, 3, okp) == _lib.ZK_OK     # no inputs: the zip stops at 1
    assert np.array_equal(ok.astype(bool), single(ctx, crs, [[]] * 3, p[:3]))


@pytest.mark.gpu
def test_batch_larger_than_one_chunk(ctx, simple):
    """CHUNK + 77 proofs: an honest proof, the same with a wrong input, a flipped byte, in a pattern with known verdicts"""
    p = simple["proofs"][0]
    bad = bytearray(p); bad[100] ^= 4
    n = CHUNK + 77
    kind = np.arange(n) % 3
    proofs = np.frombuffer(p, dtype=np.uint8)[None].repeat(n, axis=0)
    proofs[kind == 2] = np.frombuffer(bytes(bad), dtype=np.uint8)
    x = ints_to_limbs([2, 34, 2, 25]).reshape(2, 2, 4)
    rows = x[(kind == 1).astype(int)]
    want = kind == 0
    assert not ctx.verify(simple["crs"], [2, 34], bytes(bad)) and not ctx.verify(simple["crs"], [2, 25], p)
    got = ctx.verify_batch(simple["crs"], rows, proofs)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_call_next_to_an_outstanding_proof(ctx, simple):
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    log_n = 12
    rng = SplitMix64(4243)
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    r, s = rng.fr(), rng.fr()
    want_proof = ctx.prove(crs, qap, weights, r, s)
    host = ctx.host_alloc(weights.shape)
    host[:] = weights
    try:
        t = ctx.prove_submit_host(crs, qap, host.ctypes.data, weights.shape[0], r, s)
        rows, proofs = _tampered_batch(simple, 9)
        got = ctx.verify_batch(simple["crs"], rows, proofs)
        proof = ctx.prove_wait(t)
    finally:
        ctx.host_free(host)
    assert proof == want_proof
    assert np.array_equal(got, single(ctx, simple["crs"], rows, proofs))
    assert ctx.verify_batch(crs, weights[None, 1:1 + l], [proof]).all()


@pytest.mark.gpu
def test_layers_agree(ctx, simple, tmp_path):
    from zksnark_rs_amd import groth16
    code = open(os.path.join(ZK_DIR, "simple.zk")).read()
    qap = groth16.QAP.from_zk(ctx, code)
    w = groth16.weights(code, [3, 2, 4])
    sigma = groth16.setup(qap)
    proofs = [groth16.prove(qap, sigma, w) for _ in range(3)]
    rows = [[2, 34], [2, 25], [2, 34]]
    via_groth16 = groth16.verify_batch(sigma, rows, proofs)
    via_ctx = ctx.verify_batch(sigma[0].crs, ints_to_limbs([x for r in rows for x in r]).reshape(3, 2, 4),
                               np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(3, -1))
    assert np.array_equal(via_groth16, via_ctx) and via_groth16.tolist() == [True, False, True]
    assert via_groth16.tolist() == [groth16.verify(sigma, r, p) for r, p in zip(rows, proofs)]
    # the C++ layer (include/zksnark.hpp)
    libdir = os.path.join(ROOT, "zksnark_rs_amd")
    exe = str(tmp_path / "verify_batch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "verify_batch_check.cpp"),
                    "-o", exe, "-L", libdir, "-lzkgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([exe, os.path.join(ZK_DIR, "simple.zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split(" ", 1) for line in res.stdout.strip().splitlines())
    assert lines["batch"] == lines["single"] == "1 1 0 1 0 1"
