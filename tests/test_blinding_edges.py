"""-m "not gpu": the yardstick of tests/test_gpu_blinding_edges.py -- the expected bytes of a proof whose blinding scalars (r, s) steer
the closing additions into a doubling, a cancellation or an infinity operand (blinding_edge_cases.py), tied to the reference
restatements before any GPU is involved.

For every named case, on the chain circuit of 4 and 8 gates, for a satisfying witness and for one broken at one gate:

  pyref.prove_with_rs (groth16::prove, mod.rs:213-296, affine big integers) == pyref.trapdoor_proof (the closed form)
  == the oracle's closed form == the oracle's faithful prover over the oracle's faithful setup == the helper's own logarithms;

the elements the helper predicts to be infinity are the all-zero encodings and no others are; pyref.verify_bn (groth16::verify,
mod.rs:299-320) accepts every proof of the satisfying witness, those with an element at infinity included.  The helper's U, V, L, HT for
the other circuits of the device module (2^6 gates, the integer roots, simple.zk in coefficient form) are tied to the oracle's closed
forms too."""
import os
import sys

import numpy as np
import pytest

import zksnark_rs_amd as zk
from zksnark_rs_amd import ints_to_limbs

import blinding_edge_cases as bec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
ZK_DIR = os.path.join(ROOT, "tests", "golden", "zk")
LOG_SIZES = (2, 3)


def infinite_elements(proof):
    """which of a, b, c are encoded as infinity; such a block is all zero, a finite one starts with 4"""
    out = ""
    for k, (at, size) in zip("abc", ((0, 65), (65, 129), (194, 65))):
        block = proof[at:at + size]
        assert block[0] in (0, 4)
        if block[0] == 0:
            assert block == bytes(size)
            out += k
    return out


def encode_logs(orc, logs):
    """the proof whose elements are [a]_1, [b]_2, [c]_1 for the encryption bases, through the oracle's scalar multiplication"""
    a, b, c = logs
    g1 = orc.g1_mul_batch(np.tile(orc.enc_base_g1(), (2, 1)), ints_to_limbs([a, c]))
    g2 = orc.g2_mul_batch(orc.enc_base_g2().reshape(1, 16), ints_to_limbs([b]))

    def block(words, order):
        coords = zk.limbs_to_ints(words)
        if not any(coords):
            return bytes(1 + 32 * len(coords))
        return b"\x04" + b"".join(coords[k].to_bytes(32, "big") for k in order)
    return block(g1[0], (0, 1)) + block(g2[0], (1, 0, 3, 2)) + block(g1[1], (0, 1))


@pytest.fixture(scope="module")
def chains(orc):
    import functools
    import pyref
    out = {}
    # verify_bn pairs (alpha, beta) and (the input sum, gamma) anew for every proof; over one CRS and one input row they are the same
    # two pure function calls each time, and the final exponentiation is most of a verdict's cost: remember them
    patch = pytest.MonkeyPatch()
    patch.setattr(pyref, "pairing", functools.lru_cache(maxsize=None)(pyref.pairing))
    for log_n in LOG_SIZES:
        inst = bec.chain_instance(log_n)
        n, m, l = inst["n"], inst["m"], inst["l"]
        assert inst["roots"][1] == pyref.omega(log_n) == zk.limbs_to_int(orc.root_of_unity(log_n))
        qap = pyref.qap_from_root_rep(pyref.FR, pyref.chain_root_rep(n, inst["roots"]))
        assert (len(qap["u"]), qap["input"]) == (m, l)
        s1, s2 = pyref.setup_with_trapdoor(qap, inst["td"])
        desc = zk.Context.sparse_desc(log_n, m, l, *inst["rows"])
        tdl = ints_to_limbs(inst["td"])
        arrs = orc.setup_sparse(desc, tdl, n, m, l, True)
        inst.update(qap=qap, s1=s1, s2=s2, desc=desc, tdl=tdl, cdesc=zk.Context.crs_desc(n, m, l, arrs))
        out[log_n] = inst
    yield out
    patch.undo()


def test_every_named_case_is_there():
    names = bec.CASE_NAMES
    assert len(set(names)) == len(names) == 14 + 5 + 4 + 4 + 5 + 4
    values = dict(bec.DIGIT_VALUES)
    assert len(set(values.values())) == len(values) and all(0 <= v < bec.R for v in values.values())
    assert values["0x0f0f.."] == int("0f" * 32, 16) and values["0xf0f0.."] == int("f0" * 32, 16) % bec.R != int("f0" * 32, 16)
    assert values["(r-1)/2"] * 2 + 1 == bec.R and values["3*16^63"] >> 252 == 3 and bec.R >> 252 == 3


@pytest.mark.parametrize("name", bec.CASE_NAMES)
@pytest.mark.parametrize("log_n", LOG_SIZES)
def test_reference_restatements_agree(orc, chains, log_n, name):
    import pyref
    inst = chains[log_n]
    at = bec.CASE_NAMES.index(name)
    for which in bec.WITNESSES:
        case = inst["cases"][which][at]
        assert case.name == name
        wts = inst["witnesses"][which]
        ints = zk.limbs_to_ints(wts)
        points = pyref.trapdoor_proof(inst["qap"], inst["td"], ints, case.r, case.s)
        want = pyref.enc_proof(*points)
        assert pyref.enc_proof(*pyref.prove_with_rs(inst["qap"], inst["s1"], inst["s2"], ints, case.r, case.s)) == want, which
        assert orc.trapdoor_proof_sparse(inst["desc"], inst["tdl"], wts, case.r, case.s) == want, which
        assert orc.prove_sparse(inst["desc"], inst["cdesc"], wts, case.r, case.s, True) == want, which
        assert encode_logs(orc, bec.proof_logs(inst["td"], inst["scalars"][which], case.r, case.s)) == want, which
        assert infinite_elements(want) == case.infinite, which
        if which == "satisfying":
            assert pyref.verify_bn(inst["s1"], inst["s2"], inst["inputs"], points)


def test_a_broken_witness_is_rejected(chains):
    """the control of the verdicts above: verify_bn does reject (a drawn pair and the case whose A is infinity)"""
    import pyref
    inst = chains[2]
    ints = zk.limbs_to_ints(inst["witnesses"]["broken"])
    for name in ("pair:r*s=1", "a:infinity"):
        case = inst["cases"]["broken"][bec.CASE_NAMES.index(name)]
        assert not pyref.verify_bn(inst["s1"], inst["s2"], inst["inputs"], pyref.trapdoor_proof(inst["qap"], inst["td"], ints, case.r, case.s))


def _other_instances(orc):
    yield "chain 2^6", bec.chain_instance(6)
    yield "integers 5", bec.integers_instance(5)
    yield "simple.zk", bec.dense_instance(orc, open(os.path.join(ZK_DIR, "simple.zk")).read())


def closed_form(orc, inst, wts, r, s):
    tdl = ints_to_limbs(inst["td"])
    if inst["kind"] == "dense":
        q = inst["dense"]
        return orc.trapdoor_proof_dense(q["u"], q["v"], q["w"], q["t"], q["input"], tdl, wts, r, s)
    desc = zk.Context.sparse_desc(inst.get("log_n", 0), inst["m"], inst["l"], *inst["rows"])
    if inst["kind"] == "integers":
        return orc.trapdoor_proof_integers(desc, inst["n"], tdl, wts, r, s)
    return orc.trapdoor_proof_sparse(desc, tdl, wts, r, s)


def test_helper_scalars_on_the_device_modules_other_circuits(orc):
    """U, V, L, HT of the helper give the oracle's closed-form bytes on every case, and the predicted infinities are the encoded ones"""
    for label, inst in _other_instances(orc):
        for which in bec.WITNESSES:
            for case in inst["cases"][which]:
                want = closed_form(orc, inst, inst["witnesses"][which], case.r, case.s)
                assert encode_logs(orc, bec.proof_logs(inst["td"], inst["scalars"][which], case.r, case.s)) == want, (label, which, case.name)
                assert infinite_elements(want) == case.infinite, (label, which, case.name)
