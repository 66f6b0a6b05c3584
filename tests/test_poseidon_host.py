"""-m "not gpu": Poseidon's host code (csrc/poseidon.hpp, the gadgets of csrc/builder.hpp, zk_builder_finish and the three host
evaluators on what they emit) as a stand-alone program under ASan + UBSan (tests/cpp/poseidon_host.hip), held against
tests/poseidon_model.py.  Never loaded into Python, never run on a GPU."""
import os
import shutil
import subprocess

import pytest

import poseidon_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("poseidon_host") / "poseidon_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "poseidon_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


@pytest.mark.parametrize("index", [0, 3, 4])
def test_poseidon_host_code_under_sanitizers(host_exe, index):
    abcd = [pm.R - 1, 0, 0x1234567890abcdef << 180 | 77, pm.hash([5])]
    res = subprocess.run([host_exe], input=" ".join("%064x" % x for x in abcd) + " %d\n" % index, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    want = []
    for arity in (1, 2, 4):
        c, m = pm.params(arity + 1)
        want.append("params %d %d %064x %064x %064x %064x" % (arity, pm.R_P[arity + 1], c[0], c[-1], m[0][0], m[-1][-1]))
    for arity in (1, 2, 4):
        want.append("hash %d %064x" % (arity, pm.hash(abcd[:arity])))
    want.append("zero %064x" % pm.zero_hashes(3)[3])
    for arity in (1, 2, 4):
        want.append("gadget %d %d %064x" % (arity, pm.gate_count(arity), pm.hash(abcd[:arity])))
    levels = pm.tree_levels(abcd + abcd[:1], 3)
    assert pm.fold(*pm.path(levels, 3, index)) == pm.tree_root(levels, 3)
    want.append("merkle %d %064x" % (3 * 246, pm.tree_root(levels, 3)))
    want.append("refused 9 of 9")
    assert res.stdout.strip().splitlines() == want
