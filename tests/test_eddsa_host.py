"""-m "not gpu": EdDSA-Poseidon's host code (csrc/eddsa.hpp, the gadget of csrc/builder.hpp, zk_builder_finish and the three host
evaluators on what it emits) as a stand-alone program under ASan + UBSan (tests/cpp/eddsa_host.hip), held against
tests/eddsa_model.py -- all 408 round constants and 36 matrix entries of width 6 among it.  Never loaded into Python, never run on
a GPU."""
import os
import shutil
import subprocess

import pytest

import babyjub_model as bm
import eddsa_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, L = bm.R, bm.L


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("eddsa_host") / "eddsa_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "eddsa_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


@pytest.mark.parametrize("k, nonce_key, msg", [(L - 1, R - 1, R - 1), (1, 0, 0), (0x1234567890abcdef << 120, 77, 1 << 253)])
def test_eddsa_host_code_under_sanitizers(host_exe, k, nonce_key, msg):
    res = subprocess.run([host_exe], input="%064x %064x %064x\n" % (k, nonce_key, msg), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    a = em.public_key(k)
    r8, s = em.sign(k, nonce_key, msg)
    c, m = em.params6()
    statuses = [em.verify(a, msg, r8, s), em.verify(a, (msg + 1) % (1 << 256), r8, s), em.verify(a, msg, r8, s + L), em.verify((R, a[1]), msg, r8, s),
                em.verify((a[0], a[1] + 1), msg, r8, s), em.verify(a, msg, (r8[0], r8[1] + 1), s)]
    assert statuses[0] == em.VALID and statuses[2] in (em.S_RANGE, em.RANGE) and statuses[3] == em.RANGE
    want = ["challenge %064x" % em.H6_12345]
    want += ["c %d %064x" % (i, x) for i, x in enumerate(c)]
    want += ["m %d %064x" % (i, x) for i, x in enumerate(x for row in m for x in row)]
    want += ["public %064x %064x" % a,
             "sign %064x %064x %064x" % (r8[0], r8[1], s),
             "status " + " ".join(str(x) for x in statuses),
             "gadget %d 0" % em.eddsa_gates(),
             "refused 9 of 9"]
    assert res.stdout.strip().splitlines() == want
