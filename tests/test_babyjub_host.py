"""-m "not gpu": Baby Jubjub's host code (csrc/babyjub.hpp, the gadgets of csrc/builder.hpp, zk_builder_finish and the three host
evaluators on what they emit) as a stand-alone program under ASan + UBSan (tests/cpp/babyjub_host.hip), held against
tests/babyjub_model.py.  Never loaded into Python, never run on a GPU."""
import os
import shutil
import subprocess

import pytest

import babyjub_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("babyjub_host") / "babyjub_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "babyjub_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


@pytest.mark.parametrize("k, n_bits", [((1 << 256) - 1, 256), (bm.L + 0x1234567, 251), (0b1011010, 7), (1, 1), (0x2e, 2)])
def test_babyjub_host_code_under_sanitizers(host_exe, k, n_bits):
    res = subprocess.run([host_exe], input="%064x %d\n" % (k, n_bits), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    s = k & ((1 << n_bits) - 1)
    point = lambda p: "%064x %064x" % p   # noqa: E731
    want = ["params %d %d %064x" % (bm.A, bm.D, bm.L),
            "mul " + point(bm.mul(k)),
            "mulgen " + point(bm.mul(k, bm.GENERATOR)),
            "add " + point(bm.add(bm.mul(k), bm.GENERATOR)),
            "fixed %d %s" % (bm.fixed_gates(n_bits) + 4, point(bm.mul(s))),
            "var %d %s" % (bm.var_gates(n_bits) + 4, point(bm.mul(s, bm.GENERATOR))),
            "refused 10 of 10"]
    assert res.stdout.strip().splitlines() == want
