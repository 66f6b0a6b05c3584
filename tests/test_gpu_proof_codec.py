"""The compressed proof form on the GPU (csrc/proof_codec.hip): zk_proof_decompress_batch / zk_proof_compress_batch give the bytes
and status of the single host forms for every entry of batches that mix honest proofs, infinities and every refusal class;
zk_verify_batch_compressed equals zk_verify_batch run on the host-decompressed strings; argument rules, a batch larger than one
chunk, a call next to an outstanding proof ticket, and the Python, groth16 and C++ layers."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import proof_codec_model as M
from proof_codec_model import Q, pyref
import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_DIR = os.path.join(ROOT, "tests", "golden", "zk")
CHUNK = 65536   # ZK_VERIFY_BATCH_CHUNK (include/zkgpu.h)
GOOD = [2, 34]  # simple.zk's verify wires for the inputs (3, 2, 4)


def host_decompress(c):
    """(ok, 259 bytes) from the single host form; 259 x 0xFF when it refuses"""
    src = (C.c_uint8 * 128).from_buffer_copy(c)
    dst = (C.c_uint8 * 259)()
    st = _lib.load().zk_proof_decompress(src, dst)
    assert st in (_lib.ZK_OK, _lib.ZK_ERR_RANGE)
    return st == _lib.ZK_OK, bytes(dst)


def host_compress(p):
    src = (C.c_uint8 * 259).from_buffer_copy(p)
    dst = (C.c_uint8 * 128)()
    st = _lib.load().zk_proof_compress(src, dst)
    assert st in (_lib.ZK_OK, _lib.ZK_ERR_RANGE)
    return st == _lib.ZK_OK, bytes(dst)


@pytest.fixture(scope="module")
def simple(ctx):
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(open(os.path.join(ZK_DIR, "simple.zk")).read())
    weights = c.weights([3, 2, 4])
    qap = c.qap(ctx)
    rng = SplitMix64(2031)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    proofs = [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(4)]
    other = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    foreign = ctx.prove(other, qap, weights, rng.fr(), rng.fr())
    packed = [zk.proof_compress(p) for p in proofs]
    assert [zk.proof_decompress(c) for c in packed] == proofs
    return dict(qap=qap, crs=crs, weights=weights, proofs=proofs, foreign=foreign, packed=packed)


@pytest.fixture(scope="module")
def outside_g2():
    """a twist point that is not in the order-r subgroup"""
    rng = random.Random(77)
    while True:
        P = M.g2_from_x((rng.randrange(Q), rng.randrange(Q)), True)
        if P is not None:
            break
    assert pyref.g2_on_curve(P) and pyref.g2_add(pyref.g2_mul(P, pyref.R - 1), P) is not None
    return P


@pytest.fixture(scope="module")
def pools(simple, outside_g2):
    """(128-byte strings, 259-byte strings) that interleave honest proofs, infinities and every refusal class, each with the
    single host form's (ok, bytes) computed once"""
    rng = random.Random(78)
    packed = simple["packed"]
    valid_c = list(packed) + [M.INF_PROOF_C, M.INF_G1C + packed[0][32:], packed[1][:32] + M.INF_G2C + packed[1][96:], packed[2][:96] + M.INF_G1C,
                              packed[0][:32] + M.enc_g2c(outside_g2) + packed[0][96:],
                              bytes([packed[3][0] ^ 0x40]) + packed[3][1:]]
    pts = [x for x in (rng.randrange(Q) for _ in range(40)) if M.fq_sqrt(M.g1_rhs(x)) is not None][:6]
    for i, x in enumerate(pts):                                   # random points, both signs, in both G1 slots
        valid_c.append(M.enc_g1c(M.g1_from_x(x, i & 1 == 0)) + M.INF_G2C + M.enc_g1c(M.g1_from_x(x, i & 1 == 1)))
    bad_c = [s for _, s in M.malformed_compressed(packed[0])]
    pool_c = []
    for i in range(max(len(valid_c), len(bad_c)) * 2):            # valid and invalid lanes side by side
        pool_c.append((bad_c if i & 1 else valid_c)[(i // 2) % len(bad_c if i & 1 else valid_c)])
    single_c = [host_decompress(c) for c in pool_c]
    assert all(ok for ok, _ in single_c[0::2]) and not any(ok for ok, _ in single_c[1::2])
    assert all(p == M.BAD_DECOMPRESSED for _, p in single_c[1::2])
    valid_u = [p for ok, p in single_c if ok]
    bad_u = [s for _, s in M.malformed_uncompressed(simple["proofs"][0])]
    pool_u = []
    for i in range(len(valid_u) * 2):
        pool_u.append(bad_u[(i // 2) % len(bad_u)] if i & 1 else valid_u[i // 2])
    single_u = [host_compress(p) for p in pool_u]
    assert all(ok for ok, _ in single_u[0::2]) and all((ok, c) == (False, M.BAD_COMPRESSED) for ok, c in single_u[1::2])
    return dict(c=pool_c, single_c=single_c, u=pool_u, single_u=single_u)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_batch_equals_single(ctx, pools, n):
    """blocks end mid-wave (63, 65, 200) and waves hold valid and invalid lanes side by side"""
    for key, single, call in (("c", "single_c", ctx.proof_decompress_batch), ("u", "single_u", ctx.proof_compress_batch)):
        pool, want = pools[key], pools[single]
        idx = [(j + n) % len(pool) for j in range(n)]              # another phase for every n
        out, ok = call([pool[i] for i in idx])
        assert out.shape == (n, len(want[0][1])) and ok.dtype == bool
        for j, i in enumerate(idx):
            assert (bool(ok[j]), out[j].tobytes()) == want[i], (key, n, j)


def _verify_cases(simple, outside_g2):
    """(rows, 128-byte strings, what is known about each)"""
    packed = simple["packed"]
    flipped = bytes([packed[0][0] ^ 0x40]) + packed[0][1:]
    assert host_decompress(flipped)[0] and host_decompress(flipped)[1] != simple["proofs"][0]
    swapped_b = packed[1][:32] + M.enc_g2c(outside_g2) + packed[1][96:]
    assert host_decompress(swapped_b)[0]
    cases = [(GOOD, c, True) for c in packed]
    cases += [(GOOD, flipped, False), (GOOD, swapped_b, False), (GOOD, zk.proof_compress(simple["foreign"]), False),
              ([2, 25], packed[2], False), (GOOD, M.INF_PROOF_C, False)]
    cases += [(GOOD, s, False) for _, s in M.malformed_compressed(packed[3])]
    order = np.random.default_rng(12).permutation(len(cases))
    return [cases[i] for i in order]


@pytest.mark.gpu
def test_verify_batch_compressed_equals_verify_batch_on_decompressed(ctx, simple, outside_g2):
    cases = _verify_cases(simple, outside_g2)
    rows, strings = [r for r, _, _ in cases], [c for _, c, _ in cases]
    plain = [host_decompress(c)[1] for c in strings]
    got = ctx.verify_batch_compressed(simple["crs"], rows, strings)
    want = ctx.verify_batch(simple["crs"], rows, plain)
    assert got.dtype == bool and np.array_equal(got, want)
    assert got.tolist() == [k for _, _, k in cases] and got.sum() == 4
    # truncated input rows: n_inputs < l, > l (l = 2), and none; an input >= r beyond l is not read
    for row in ([2], [2, 34, 7], [2, 34, zk.R_MODULUS + 5], []):
        r = [row] * len(strings)
        assert np.array_equal(ctx.verify_batch_compressed(simple["crs"], r, strings), ctx.verify_batch(simple["crs"], r, plain)), row
    assert ctx.verify_batch_compressed(simple["crs"], [[2, 34, 7]] * 4, simple["packed"]).all()


@pytest.mark.gpu
def test_argument_rules(ctx, simple):
    lib, crs = ctx.lib, simple["crs"]
    R = zk.R_MODULUS
    pb = np.frombuffer(b"".join(simple["packed"][:3]), dtype=np.uint8).copy()
    ok = np.full(3, 7, np.int32)
    okp, pp = ok.ctypes.data_as(C.POINTER(C.c_int)), pb.ctypes.data_as(_lib.u8p)
    x = ints_to_limbs([2, 34, 2, R + 1, 2, 34])                      # proof 1's second input >= r, inside l
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, x.ctypes.data_as(_lib.u64p), 2, pp, 3, okp) == _lib.ZK_ERR_RANGE
    assert (ok == 0).all()
    with pytest.raises(zk.ZkError):
        ctx.verify_batch_compressed(crs, [[2, 34], [2, R], [2, 34]], simple["packed"][:3])
    good = ints_to_limbs(GOOD * 3)
    gp = good.ctypes.data_as(_lib.u64p)
    assert lib.zk_verify_batch_compressed(None, crs.ptr, gp, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch_compressed(ctx.ptr, None, gp, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, gp, 2, None, 3, okp) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, gp, 2, pp, 3, None) == _lib.ZK_ERR_ARG
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, None, 2, pp, 3, okp) == _lib.ZK_ERR_ARG
    ok[:] = 7
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, gp, 2, pp, 0, okp) == _lib.ZK_OK
    assert (ok == 7).all()
    assert lib.zk_verify_batch_compressed(ctx.ptr, crs.ptr, gp, 2, pp, 3, okp) == _lib.ZK_OK and (ok == 1).all()
    # the two codec calls
    out = np.full(3 * 259, 0x55, np.uint8)
    op = out.ctypes.data_as(_lib.u8p)
    for fn in (lib.zk_proof_decompress_batch, lib.zk_proof_compress_batch):
        assert fn(None, pp, 3, op, okp) == _lib.ZK_ERR_ARG
        assert fn(ctx.ptr, None, 3, op, okp) == _lib.ZK_ERR_ARG
        assert fn(ctx.ptr, pp, 3, None, okp) == _lib.ZK_ERR_ARG
        assert fn(ctx.ptr, pp, 3, op, None) == _lib.ZK_ERR_ARG
        ok[:] = 7
        assert fn(ctx.ptr, pp, 0, op, okp) == _lib.ZK_OK and fn(ctx.ptr, None, 0, None, None) == _lib.ZK_OK
        assert (ok == 7).all() and (out == 0x55).all()
    empty, none = ctx.proof_decompress_batch([])
    assert empty.shape == (0, 259) and none.shape == (0,)


@pytest.mark.gpu
def test_batch_larger_than_one_chunk(ctx, simple):
    """CHUNK + 3 compressed proofs cycled from the four, one malformed entry among the last three"""
    n = CHUNK + 3
    four = np.frombuffer(b"".join(simple["packed"]), dtype=np.uint8).reshape(4, 128)
    strings = four[np.arange(n) % 4].copy()
    strings[n - 2, 32] &= 0x3F                                     # flag 00 on B
    rows = np.repeat(ints_to_limbs(GOOD).reshape(1, 2, 4), n, axis=0)
    want = np.ones(n, dtype=bool)
    want[n - 2] = False
    got = ctx.verify_batch_compressed(simple["crs"], rows, strings)
    assert np.array_equal(got, want)
    out, ok = ctx.proof_decompress_batch(strings)
    assert np.array_equal(ok, want) and (out[n - 2] == 0xFF).all()
    plain = np.frombuffer(b"".join(simple["proofs"]), dtype=np.uint8).reshape(4, 259)
    assert np.array_equal(out[want], plain[np.arange(n) % 4][want])
    back, ok2 = ctx.proof_compress_batch(out)
    assert np.array_equal(ok2, want) and np.array_equal(back[want], strings[want]) and not back[n - 2].any()


@pytest.mark.gpu
def test_call_next_to_an_outstanding_proof(ctx, simple, outside_g2):
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    log_n = 12
    rng = SplitMix64(4245)
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    r, s = rng.fr(), rng.fr()
    want_proof = ctx.prove(crs, qap, weights, r, s)
    cases = _verify_cases(simple, outside_g2)
    rows, strings = [c[0] for c in cases], [c[1] for c in cases]
    host = ctx.host_alloc(weights.shape)
    host[:] = weights
    try:
        t = ctx.prove_submit_host(crs, qap, host.ctypes.data, weights.shape[0], r, s)
        got = ctx.verify_batch_compressed(simple["crs"], rows, strings)
        out, ok = ctx.proof_decompress_batch(strings)
        back, ok2 = ctx.proof_compress_batch(out)
        proof = ctx.prove_wait(t)
    finally:
        ctx.host_free(host)
    assert proof == want_proof
    assert got.tolist() == [k for _, _, k in cases]
    assert [(bool(o), p.tobytes()) for o, p in zip(ok, out)] == [host_decompress(c) for c in strings]
    assert np.array_equal(ok2, ok) and all(back[j].tobytes() == strings[j] for j in np.flatnonzero(ok))
    assert ctx.verify_batch_compressed(crs, weights[None, 1:1 + l], [zk.proof_compress(proof)]).all()


@pytest.mark.gpu
def test_layers_agree(ctx, simple, tmp_path):
    from zksnark_rs_amd import groth16
    code = open(os.path.join(ZK_DIR, "simple.zk")).read()
    qap = groth16.QAP.from_zk(ctx, code)
    w = groth16.weights(code, [3, 2, 4])
    sigma = groth16.setup(qap)
    proofs = [groth16.prove(qap, sigma, w) for _ in range(3)]
    packed = [groth16.compress(p) for p in proofs]
    assert [len(c) for c in packed] == [128] * 3 and [groth16.decompress(c) for c in packed] == proofs
    assert packed == [ctx.proof_compress(p) for p in proofs] and proofs == [ctx.proof_decompress(c) for c in packed]
    with pytest.raises(zk.ZkError) as e:
        groth16.decompress(bytes(128))
    assert e.value.status == _lib.ZK_ERR_RANGE
    rows = [[2, 34], [2, 25], [2, 34]]
    via_groth16 = groth16.verify_batch_compressed(sigma, rows, packed)
    via_ctx = ctx.verify_batch_compressed(sigma[0].crs, ints_to_limbs([x for r in rows for x in r]).reshape(3, 2, 4),
                                          np.frombuffer(b"".join(packed), dtype=np.uint8).reshape(3, -1))
    assert np.array_equal(via_groth16, via_ctx) and via_groth16.tolist() == [True, False, True]
    assert via_groth16.tolist() == groth16.verify_batch(sigma, rows, proofs).tolist()
    out, ok = ctx.proof_compress_batch(proofs)
    assert ok.all() and [o.tobytes() for o in out] == packed
    # the C++ layer (include/zksnark.hpp)
    libdir = os.path.join(ROOT, "zksnark_rs_amd")
    exe = str(tmp_path / "proof_codec_api")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "proof_codec_api.cpp"),
                    "-o", exe, "-L", libdir, "-lzkgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([exe, os.path.join(ZK_DIR, "simple.zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split(" ", 1) for line in res.stdout.strip().splitlines())
    assert lines["roundtrip"] == "1 1 1 1 1 1"
    assert lines["compressed"] == lines["plain"] == "1 1 0 0 0 1"
    assert lines["refused"] == "%d %d" % (_lib.ZK_ERR_RANGE, _lib.ZK_ERR_RANGE)
