"""zk_verify_batch_all's device code (csrc/verify_all.cuh: the per-lane step, the reductions' combine, the column sums, T_S and
the final combination) compiled for the HOST (tests/cpp/verify_all_check.hip) and run on batches over the CRSs of
tests/golden/proofs.json, whose trapdoors are known: the verifying points come from pyref.setup_with_trapdoor, further honest
proofs are simulated with the trapdoor, and every per-proof verdict is checked against zk_pairing (host).  No GPU needed."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs, SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLD = os.path.join(ROOT, "tests", "golden")
PROOFS = json.load(open(os.path.join(GOLD, "proofs.json")))
CIRCUITS = json.load(open(os.path.join(GOLD, "circuits.json")))
H = lambda s: s if isinstance(s, int) else int(s, 16)   # noqa: E731


def g1_words(P):
    return [0] * 8 if P is None else [int(x) for x in ints_to_limbs([P[0], P[1]]).reshape(8)]


def g2_words(P):
    return [0] * 16 if P is None else [int(x) for x in ints_to_limbs([P[0][0], P[0][1], P[1][0], P[1][1]]).reshape(16)]


def hexw(words):
    return " ".join("%x" % w for w in words)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("verify_all") / "verify_all_check")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "verify_all_check.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)

    def run(vk, batch):
        """vk = (s1, s2, l); batch = [(proof bytes, z, input row)] -> (verdict, [t_0 .. t_k])"""
        s1, s2, l = vk
        k = l
        req = ["crs %d %s %s %s %s %s" % (k, hexw(g1_words(s1["alpha"])), hexw(g2_words(s2["beta"])), hexw(g2_words(s2["gamma"])),
                                          hexw(g2_words(s2["delta"])), " ".join(hexw(g1_words(P)) for P in s1["sum_gamma"][:k + 1])),
               "batch %d" % len(batch)]
        for proof, z, row in batch:
            assert len(row) == k and 0 < z < 2 ** 128
            req.append("%s %s %s" % (bytes(proof).hex(), hexw([z & (2 ** 64 - 1), z >> 64]),
                                     hexw([int(w) for w in ints_to_limbs(list(row)).reshape(-1)]) if k else ""))
        res = subprocess.run([exe], input="\n".join(req) + "\n", capture_output=True, text=True, timeout=900, check=True)
        out = res.stdout.splitlines()
        assert out[0] in ("ok 0", "ok 1"), res.stdout
        t = zk.limbs_to_ints([int(w, 16) for w in out[1].split()[1:]])
        return out[0] == "ok 1", list(t)
    return run


def _qap(c):
    """the pyref QAP of a fixture's circuit, cut to the wires the verifying key reads (the constant and the l inputs)"""
    import pyref
    if "log_n" in c:
        n = 1 << H(c["log_n"])
        w = pyref.omega(H(c["log_n"]))
        rr = pyref.chain_root_rep(n, [pow(w, j, pyref.R) for j in range(n)])
    else:
        rr = dict(CIRCUITS[c["name"]])
    l = H(c["input"])
    rr = dict(rr, u=rr["u"][:l + 1], v=rr["v"][:l + 1], w=rr["w"][:l + 1], input=l)
    return pyref.qap_from_root_rep(pyref.FR, rr)


def _inputs(c):
    if "verify_inputs" in c:
        return [H(x) for x in c["verify_inputs"]]
    from zksnark_rs_amd.circuits import chain_weights
    log_n = H(c["log_n"])
    rng = SplitMix64(H(c["input_seed"]))
    x = rng.fr()
    weights = chain_weights(log_n, x, [rng.fr() for _ in range(1 << log_n)])
    return zk.limbs_to_ints(weights[1:1 + H(c["input"])])


@pytest.fixture(scope="module", params=[c["name"] for c in PROOFS["cases"]])
def case(request):
    """verifying key, the fixture's proof with its inputs, and a simulator of further honest proofs for any input row"""
    import pyref
    c = next(c for c in PROOFS["cases"] if c["name"] == request.param)
    qap = _qap(c)
    td = [H(t) for t in c["trapdoor"]]
    s1, s2 = pyref.setup_with_trapdoor(qap, td)
    alpha, beta, gamma, delta, x = td
    F = pyref.FR
    comb = [F.add(F.add(F.mul(beta, pyref.poly_eval(F, u, x)), F.mul(alpha, pyref.poly_eval(F, v, x))), pyref.poly_eval(F, w, x))
            for u, v, w in zip(qap["u"], qap["v"], qap["w"])]
    l = qap["input"]
    rng = SplitMix64(H(c["seed"]) + 1)

    def simulate(row):
        """A = a G, B = b H, C = (a b - alpha beta - sum_i x_i comb_i) / delta G: e(A, B) = e(alpha, beta) e(S, gamma) e(C, delta)"""
        a, b = rng.fr(), rng.fr()
        s = sum(xi * ci for xi, ci in zip([1] + list(row), comb)) % pyref.R
        cc = F.div((a * b - alpha * beta - s) % pyref.R, delta)
        return pyref.enc_proof(pyref.encrypt_g1(a), pyref.encrypt_g2(b), pyref.encrypt_g1(cc))

    return dict(vk=(s1, s2, l), proof=bytes.fromhex(c["proof"]), row=_inputs(c), simulate=simulate, rng=rng, l=l)


def _points(proof):
    import pyref

    def g1(b):
        return None if b[0] == 0 else (int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:65], "big"))
    b = proof[65:194]
    B = None if b[0] == 0 else ((int.from_bytes(b[33:65], "big"), int.from_bytes(b[1:33], "big")),
                                (int.from_bytes(b[97:129], "big"), int.from_bytes(b[65:97], "big")))
    assert pyref.enc_proof(g1(proof[:65]), B, g1(proof[194:])) == proof
    return g1(proof[:65]), B, g1(proof[194:])


def verdict(vk, row, proof):
    """zk_verify's equation through zk_pairing (host): e(A, B) == e(alpha, beta) e(S, gamma) e(C, delta)"""
    import pyref
    s1, s2, l = vk
    A, B, C = _points(proof)
    S = None
    for g, x in zip(s1["sum_gamma"], [1] + list(row)[:l]):
        S = pyref.g1_add(S, pyref.g1_mul(g, x))

    def e(P, Q):
        return _unflatten(zk.pairing(np.array(g1_words(P), np.uint64), np.array(g2_words(Q), np.uint64)))
    rhs = pyref.fq12_mul(pyref.fq12_mul(e(s1["alpha"], s2["beta"]), e(S, s2["gamma"])), e(C, s2["delta"]))
    return rhs == e(A, B)


def _unflatten(flat):
    it = iter(int(v) for v in flat)
    return tuple(tuple((next(it), next(it)) for _ in range(3)) for _ in range(2))


def _honest(case, count):
    rows = [case["row"]] + [[case["rng"].fr() for _ in range(case["l"])] for _ in range(count - 1)]
    proofs = [case["proof"]] + [case["simulate"](r) for r in rows[1:]]
    return rows, proofs


def _z(case, n):
    return [(case["rng"].fr() % (2 ** 128)) or 1 for _ in range(n)]


def test_honest_batches_accepted_and_column_sums(check, case):
    import pyref
    rows, proofs = _honest(case, 4)
    assert all(verdict(case["vk"], r, p) for r, p in zip(rows, proofs))
    for z in (_z(case, 4), [1] * 4, [2 ** 128 - 1] * 4):
        ok, t = check(case["vk"], list(zip(proofs, z, rows)))
        assert ok
        want = [sum(z) % pyref.R] + [sum(zj * r[i] for zj, r in zip(z, rows)) % pyref.R for i in range(case["l"])]
        assert t == want


def test_each_single_tampered_proof_fails_its_batch(check, case):
    import pyref
    rows, proofs = _honest(case, 3)
    p = proofs[1]
    A, B, C = _points(p)
    bad_row = list(rows[1]); bad_row[0] = (bad_row[0] + 1) % pyref.R
    tampered = [(bad_row, p),                                                                        # a wrong input
                (rows[1], p[194:] + p[65:194] + p[:65]),                                             # A and C swapped
                (rows[1], pyref.enc_proof(A, B, pyref.g1_add(C, pyref.G1_GEN)))]                     # C + G
    z = _z(case, 3)
    for row, bad in tampered:
        assert not verdict(case["vk"], row, bad)
        batch = list(zip(proofs, z, rows))
        batch[1] = (bad, z[1], row)
        assert check(case["vk"], batch)[0] is False


def test_cancellation_pair_passes_only_with_equal_multipliers(check, case):
    """(A1, B1, C1 + D), (A2, B2, C2 - D): each fails alone; z = (1, 1) cancels D in T_C, z = (1, 2) does not"""
    import pyref
    rows, proofs = _honest(case, 2)
    D = pyref.g1_mul(pyref.G1_GEN, 0x1234567)
    (A1, B1, C1), (A2, B2, C2) = _points(proofs[0]), _points(proofs[1])
    pair = [pyref.enc_proof(A1, B1, pyref.g1_add(C1, D)), pyref.enc_proof(A2, B2, pyref.g1_add(C2, pyref.g1_neg(D)))]
    assert not verdict(case["vk"], rows[0], pair[0]) and not verdict(case["vk"], rows[1], pair[1])
    assert check(case["vk"], [(pair[0], 1, rows[0]), (pair[1], 1, rows[1])])[0] is True
    assert check(case["vk"], [(pair[0], 1, rows[0]), (pair[1], 2, rows[1])])[0] is False


def test_same_proof_twice_with_the_same_multiplier(check, case):
    """z C + z C: the C sum meets P + P and must double"""
    z = _z(case, 1)[0]
    assert check(case["vk"], [(case["proof"], z, case["row"])] * 2)[0] is True
    assert check(case["vk"], [(case["proof"], z, case["row"])] * 3)[0] is True
