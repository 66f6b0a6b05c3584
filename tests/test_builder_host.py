"""-m "not gpu": the circuit builder's host code (csrc/builder.hip, csrc/builder.hpp) as a stand-alone program under ASan + UBSan
(tests/cpp/builder_host.hip): every gate, the 64-bit comparators, a 2-round Keccak, finished and run through both host evaluators.
Never loaded into Python, never run on a GPU."""
import os
import shutil
import subprocess

import pytest

import builder_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("builder_host") / "builder_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "builder_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


def test_builder_host_code_under_sanitizers(host_exe):
    msg = bytes(range(40, 77))
    res = subprocess.run([host_exe], input=msg.hex() + "\n", capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    for k, kind in enumerate(bm.GATE_KINDS):
        want = "".join(str(bm.TRUTH[kind](v & 1, v >> 1)) for v in range(4))
        assert lines[k] == "gate %d %s" % (k, want)
    assert lines[10] == "cmp 60"                           # six comparators x ten operand pairs
    assert lines[11] == "keccak %d %s" % (8 * len(msg) + 16 + 2 * 9664 + 1, bm.sponge(msg, 136, 0x06, 2, 32).hex())
    assert lines[12] == "refused 7 of 7"
