"""zk_verify_batch_all (csrc/verify_batch_all.hip): one verdict for a whole batch, by a random linear combination of the proofs'
pairing equations.  Honest batches pass for every admissible z; a batch with a proof zk_verify rejects fails (deterministically
when it does not decode, with the fixed multipliers used here otherwise: a false pass has probability 2^-128, so a mismatch is a
bug); z is applied exactly (cancellation pairs); points at infinity, truncated rows, error codes, batches over several chunks,
a call next to an outstanding proof ticket, and the Python, groth16 and C++ layers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64, _lib
from test_gpu_verify_batch import simple, _tampered_batch, _program_proofs, wide_program, single, ROOT, ZK_DIR, CHUNK  # noqa: F401
from test_verify_all_device_code import _qap, _points

Z_MAX = 2 ** 128 - 1


def z_words(z):
    return np.array([[v & (2 ** 64 - 1), v >> 64] for v in z], dtype=np.uint64).reshape(-1, 2)


def splitmix_z(rng, n):
    out = []
    for _ in range(n):
        v = (rng.next() << 64 | rng.next()) & Z_MAX
        out.append(v or 1)
    return out


@pytest.mark.gpu
def test_honest_batches_accepted_for_every_z(ctx, simple):
    from zksnark_rs_amd.circuit import Circuit
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    cases = [(simple["crs"], simple["weights"][1:3], simple["proofs"])]
    code = open(os.path.join(ZK_DIR, "deg_15.zk")).read()
    rng = SplitMix64(1515)
    cases.append(_program_proofs(ctx, code, [rng.fr() for _ in range(Circuit(code).n_in)], 3, 17))
    log_n = 10
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    cases.append((crs, weights[1:1 + l], [ctx.prove(crs, qap, weights, rng.fr(), rng.fr()) for _ in range(3)]))
    cases.append(_program_proofs(ctx, wide_program(256), [rng.fr() for _ in range(256)], 2, 258, sparse=True))
    assert cases[-1][1].shape[0] >= 256
    for crs, x, proofs in cases:
        rows = np.repeat(x[None], len(proofs), axis=0)
        assert ctx.verify_batch(crs, rows, proofs).all()
        n = len(proofs)
        for z in (None, splitmix_z(rng, n), [1] * n, [Z_MAX] * n):
            assert ctx.verify_batch_all(crs, rows, proofs, z) is True, z


@pytest.mark.gpu
def test_each_tampered_case_at_first_middle_last_index(ctx, simple):
    """every case of _tampered_batch among five honest proofs gives exactly zk_verify's verdict"""
    crs = simple["crs"]
    rows, proofs = _tampered_batch(simple, 5)
    honest = [simple["proofs"][j % 4] for j in range(5)]
    rng = SplitMix64(77)
    verdicts = single(ctx, crs, rows, proofs)
    assert 4 <= verdicts.sum() < len(verdicts)
    for row, p, want in zip(rows, proofs, verdicts):
        for at in (0, 2, 5):
            batch = honest[:at] + [p] + honest[at:]
            batch_rows = [[2, 34]] * at + [row] + [[2, 34]] * (5 - at)
            assert ctx.verify_batch_all(crs, batch_rows, batch, splitmix_z(rng, 6)) == bool(want), (row, at)
    assert ctx.verify_batch_all(crs, rows, proofs) is False
    assert ctx.verify_batch_all(crs, rows, proofs, [1] * len(proofs)) is False


@pytest.mark.gpu
def test_random_sub_batches_match_verify_batch(ctx, simple):
    crs = simple["crs"]
    rows, proofs = _tampered_batch(simple, 11)
    pool_rows = rows + [[2, 34]] * 4
    pool = proofs + simple["proofs"]
    honest = [j for j in range(len(pool)) if ctx.verify(crs, pool_rows[j], pool[j])]
    rng = SplitMix64(2024)
    passed = 0
    for t in range(200):
        n = 1 + rng.next() % 40
        if t % 2:   # half of the batches mostly honest, so that both verdicts are common
            idx = [honest[rng.next() % len(honest)] for _ in range(n)]
            if t % 4 == 1:
                idx[rng.next() % n] = rng.next() % len(pool)
        else:
            idx = [rng.next() % len(pool) for _ in range(n)]
        b_rows, b_proofs = [pool_rows[j] for j in idx], [pool[j] for j in idx]
        want = bool(ctx.verify_batch(crs, b_rows, b_proofs).all())
        got = ctx.verify_batch_all(crs, b_rows, b_proofs, splitmix_z(rng, n))
        assert got == want, (t, idx)
        passed += got
    assert 20 <= passed <= 180


def _honest_points(simple):
    import pyref
    return [_points(p) for p in simple["proofs"][:2]], pyref


@pytest.mark.gpu
def test_cancellation_pairs_pin_exact_z(ctx, simple):
    """(A1, B1, C1 + D), (A2, B2, C2 - D) and (A + E, B, C), (A - E, B, C): each proof alone fails; z = (1, 1) cancels the
    tampering, z = (1, 2) and z drawn by the Python layer do not -- which is why z must be secret"""
    (P1, P2), pyref = _honest_points(simple)
    crs = simple["crs"]
    D = pyref.g1_mul(pyref.G1_GEN, 987654321)
    E = pyref.g1_mul(pyref.G1_GEN, 123456789)
    c_pair = [pyref.enc_proof(P1[0], P1[1], pyref.g1_add(P1[2], D)), pyref.enc_proof(P2[0], P2[1], pyref.g1_add(P2[2], pyref.g1_neg(D)))]
    a_pair = [pyref.enc_proof(pyref.g1_add(P1[0], E), P1[1], P1[2]), pyref.enc_proof(pyref.g1_add(P1[0], pyref.g1_neg(E)), P1[1], P1[2])]
    rows = [[2, 34], [2, 34]]
    for pair in (c_pair, a_pair):
        assert not ctx.verify(crs, rows[0], pair[0]) and not ctx.verify(crs, rows[1], pair[1])
        assert not ctx.verify_batch(crs, rows, pair).any()
        assert ctx.verify_batch_all(crs, rows, pair, [1, 1]) is True
        assert ctx.verify_batch_all(crs, rows, pair, [1, 2]) is False
        assert ctx.verify_batch_all(crs, rows, pair) is False


@pytest.fixture(scope="module")
def trapdoor_crs(ctx):
    """simple.zk under a trapdoor the test chose, and a simulator of proofs for it: C = (a b - alpha beta - s) / delta"""
    import pyref
    from zksnark_rs_amd.circuit import Circuit
    c = Circuit(open(os.path.join(ZK_DIR, "simple.zk")).read())
    qap = c.qap(ctx)
    rng = SplitMix64(4141)
    td = [rng.fr() for _ in range(5)]
    crs = ctx.setup(qap, ints_to_limbs(td))
    pq = _qap({"name": "simple.zk", "input": 2})
    alpha, beta, gamma, delta, x = td
    F = pyref.FR
    comb = [F.add(F.add(F.mul(beta, pyref.poly_eval(F, u, x)), F.mul(alpha, pyref.poly_eval(F, v, x))), pyref.poly_eval(F, w, x))
            for u, v, w in zip(pq["u"], pq["v"], pq["w"])]
    s = sum(xi * ci for xi, ci in zip([1, 2, 34], comb)) % pyref.R
    ab0 = (alpha * beta + s) % pyref.R      # a b - delta c must equal this

    def enc(a, b, cc):
        g1 = lambda k: None if k % pyref.R == 0 else pyref.encrypt_g1(k % pyref.R)   # noqa: E731
        return pyref.enc_proof(g1(a), None if b % pyref.R == 0 else pyref.encrypt_g2(b % pyref.R), g1(cc))

    def with_c(a, b):
        return enc(a, b, F.div((a * b - ab0) % pyref.R, delta))

    def with_ab(a, cc):   # b = (ab0 + delta c) / a
        return enc(a, F.div((ab0 + delta * cc) % pyref.R, a), cc)
    return dict(crs=crs, with_c=with_c, with_ab=with_ab, rng=rng)


@pytest.mark.gpu
def test_points_at_infinity(ctx, trapdoor_crs):
    import pyref
    crs, rng = trapdoor_crs["crs"], trapdoor_crs["rng"]
    a, b = rng.fr(), rng.fr()
    inf_a = trapdoor_crs["with_c"](0, b)
    inf_b = trapdoor_crs["with_c"](a, 0)
    inf_c = trapdoor_crs["with_ab"](a, 0)
    plain = trapdoor_crs["with_c"](rng.fr(), rng.fr())
    assert inf_a[0] == 0 and inf_b[65] == 0 and inf_c[194] == 0
    proofs = [inf_a, inf_b, inf_c, plain]
    rows = [[2, 34]] * 4
    assert single(ctx, crs, rows, proofs).all()
    for p in proofs:
        assert ctx.verify_batch_all(crs, [[2, 34]], [p]) is True
    assert ctx.verify_batch_all(crs, rows, proofs) is True
    assert ctx.verify_batch_all(crs, rows, proofs, [Z_MAX] * 4) is True
    # z_1 c_1 + z_2 c_2 = 0: T_C is infinity
    c1 = rng.fr()
    pair = [trapdoor_crs["with_ab"](rng.fr(), c1), trapdoor_crs["with_ab"](rng.fr(), (-3 * c1) % pyref.R)]
    assert single(ctx, crs, rows[:2], pair).all()
    assert pyref.g1_add(pyref.g1_mul(_points(pair[0])[2], 3), _points(pair[1])[2]) is None
    assert ctx.verify_batch_all(crs, rows[:2], pair, [3, 1]) is True


@pytest.mark.gpu
def test_input_rows_truncate_like_verify_batch(ctx, simple):
    crs, p = simple["crs"], simple["proofs"]
    R = zk.R_MODULUS
    for rows in ([[2]] * 4, [[2, 34]] * 4, [[2, 34, R + 5]] * 4, [[2, 34, 7, R]] * 4, [[]] * 4, [[2, 25, 1]] * 4,
                 [[2, 34, 1]] * 3 + [[2, 25, 1]]):
        want = bool(ctx.verify_batch(crs, rows, p).all())
        assert ctx.verify_batch_all(crs, rows, p) == want, rows
    assert ctx.verify_batch_all(crs, [[2, 34, R + 5]] * 4, p) is True
    assert ctx.verify_batch_all(crs, [[2]] * 4, p) is False


@pytest.mark.gpu
def test_error_codes(ctx, simple):
    lib, crs, p = ctx.lib, simple["crs"], simple["proofs"]
    R = zk.R_MODULUS
    pb = np.frombuffer(b"".join(p[:3]), dtype=np.uint8).copy()
    good = ints_to_limbs([2, 34] * 3)
    z = z_words([5, 6, 7])
    ok = C.c_int(7)
    gp, pp, zp, okp = good.ctypes.data_as(_lib.u64p), pb.ctypes.data_as(_lib.u8p), z.ctypes.data_as(_lib.u64p), C.byref(ok)
    f = lib.zk_verify_batch_all
    assert f(ctx.ptr, crs.ptr, gp, 2, pp, 3, zp, okp) == _lib.ZK_OK and ok.value == 1
    assert f(None, crs.ptr, gp, 2, pp, 3, zp, okp) == _lib.ZK_ERR_ARG
    assert f(ctx.ptr, None, gp, 2, pp, 3, zp, okp) == _lib.ZK_ERR_ARG
    assert f(ctx.ptr, crs.ptr, gp, 2, None, 3, zp, okp) == _lib.ZK_ERR_ARG
    assert f(ctx.ptr, crs.ptr, gp, 2, pp, 3, None, okp) == _lib.ZK_ERR_ARG
    assert f(ctx.ptr, crs.ptr, gp, 2, pp, 3, zp, None) == _lib.ZK_ERR_ARG
    assert f(ctx.ptr, crs.ptr, None, 2, pp, 3, zp, okp) == _lib.ZK_ERR_ARG
    for zero_at in range(3):
        zz = z.copy()
        zz[zero_at] = 0
        ok.value = 7
        assert f(ctx.ptr, crs.ptr, gp, 2, pp, 3, zz.ctypes.data_as(_lib.u64p), okp) == _lib.ZK_ERR_ARG and ok.value == 0
    zz = z.copy()
    zz[1] = [0, 1]                                                          # 2^64 is not 0
    assert f(ctx.ptr, crs.ptr, gp, 2, pp, 3, zz.ctypes.data_as(_lib.u64p), okp) == _lib.ZK_OK and ok.value == 1
    ok.value = 7
    assert f(ctx.ptr, crs.ptr, gp, 2, pp, 0, zp, okp) == _lib.ZK_OK and ok.value == 1
    x = ints_to_limbs([2, 34, 2, R + 1, 2, 34])                             # proof 1's second input >= r, inside l
    ok.value = 7
    assert f(ctx.ptr, crs.ptr, x.ctypes.data_as(_lib.u64p), 2, pp, 3, zp, okp) == _lib.ZK_ERR_RANGE and ok.value == 0
    with pytest.raises(zk.ZkError):
        ctx.verify_batch_all(crs, [[2, 34], [2, R], [2, 34]], p[:3])
    with pytest.raises(zk.ZkError):
        ctx.verify_batch_all(crs, [[2, 34]] * 3, p[:3], [1, 0, 1])
    assert ctx.verify_batch_all(crs, [], []) is True
    assert f(ctx.ptr, crs.ptr, None, 0, pp, 3, zp, okp) == _lib.ZK_OK
    assert ok.value == int(ctx.verify_batch(crs, [[]] * 3, p[:3]).all())


@pytest.mark.gpu
def test_batch_larger_than_one_chunk(ctx, simple):
    p = simple["proofs"][0]
    bad = bytearray(p); bad[100] ^= 4
    n = CHUNK + 77
    proofs = np.frombuffer(p, dtype=np.uint8)[None].repeat(n, axis=0)
    rows = ints_to_limbs([2, 34])[None].repeat(n, axis=0)
    rng = SplitMix64(65613)
    z = z_words(splitmix_z(rng, n))
    assert ctx.verify_batch_all(simple["crs"], rows, proofs, z) is True
    for at in (5, CHUNK + 50):
        pr = proofs.copy()
        pr[at] = np.frombuffer(bytes(bad), dtype=np.uint8)
        assert ctx.verify_batch_all(simple["crs"], rows, pr, z) is False, at
    rw = rows.copy()
    rw[CHUNK + 10] = ints_to_limbs([2, 25])
    assert ctx.verify_batch_all(simple["crs"], rw, proofs, z) is False


@pytest.mark.gpu
def test_call_next_to_an_outstanding_proof(ctx, simple):
    from zksnark_rs_amd.circuits import chain_rows, chain_weights
    log_n = 12
    rng = SplitMix64(4244)
    m, l, u, v, w = chain_rows(log_n)
    weights = chain_weights(log_n, rng.fr(), [rng.fr() for _ in range(1 << log_n)])
    qap = ctx.qap_sparse(log_n, m, l, u, v, w)
    crs = ctx.setup(qap, ints_to_limbs([rng.fr() for _ in range(5)]))
    r, s = rng.fr(), rng.fr()
    want_proof = ctx.prove(crs, qap, weights, r, s)
    host = ctx.host_alloc(weights.shape)
    host[:] = weights
    rows, proofs = _tampered_batch(simple, 9)
    try:
        t = ctx.prove_submit_host(crs, qap, host.ctypes.data, weights.shape[0], r, s)
        got_mixed = ctx.verify_batch_all(simple["crs"], rows, proofs)
        got_honest = ctx.verify_batch_all(simple["crs"], [[2, 34]] * 4, simple["proofs"])
        proof = ctx.prove_wait(t)
    finally:
        ctx.host_free(host)
    assert proof == want_proof
    assert got_mixed is False and got_honest is True
    assert ctx.verify_batch_all(crs, weights[None, 1:1 + l], [proof]) is True


@pytest.mark.gpu
def test_layers_agree(ctx, simple, tmp_path):
    from zksnark_rs_amd import groth16
    code = open(os.path.join(ZK_DIR, "simple.zk")).read()
    qap = groth16.QAP.from_zk(ctx, code)
    w = groth16.weights(code, [3, 2, 4])
    sigma = groth16.setup(qap)
    proofs = [groth16.prove(qap, sigma, w) for _ in range(3)]
    for rows, want in (([[2, 34]] * 3, True), ([[2, 34], [2, 25], [2, 34]], False)):
        z = [3, 1, Z_MAX]
        via_groth16 = groth16.verify_batch_all(sigma, rows, proofs)
        via_ctx = ctx.verify_batch_all(sigma[0].crs, ints_to_limbs([x for r in rows for x in r]).reshape(3, 2, 4),
                                       np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(3, -1), z_words(z))
        x = ints_to_limbs([v for r in rows for v in r])
        pb = np.frombuffer(b"".join(proofs), dtype=np.uint8).copy()
        ok = C.c_int(7)
        assert ctx.lib.zk_verify_batch_all(ctx.ptr, sigma[0].crs.ptr, x.ctypes.data_as(_lib.u64p), 2, pb.ctypes.data_as(_lib.u8p), 3,
                                           z_words(z).ctypes.data_as(_lib.u64p), C.byref(ok)) == _lib.ZK_OK
        assert via_groth16 == via_ctx == bool(ok.value) == want == all(groth16.verify(sigma, r, p) for r, p in zip(rows, proofs))
    # the C++ layer (include/zksnark.hpp)
    libdir = os.path.join(ROOT, "zksnark_rs_amd")
    exe = str(tmp_path / "verify_batch_all_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "verify_batch_all_check.cpp"),
                    "-o", exe, "-L", libdir, "-lzkgpu", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([exe, os.path.join(ZK_DIR, "simple.zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = dict(line.split(" ", 1) for line in res.stdout.strip().splitlines())
    assert lines == {"honest": "1 1 1 1 1 1", "wrong_input": "0 0 1 1 0 1", "flipped_byte": "0 0 1 0 1 1"}
