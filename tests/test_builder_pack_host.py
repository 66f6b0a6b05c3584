"""-m "not gpu": zk_builder_pack's host code (csrc/builder.hip, csrc/builder.hpp) as a stand-alone program under ASan + UBSan
(tests/cpp/builder_pack_host.hip): packs of every width at a limb edge through both host evaluators, the pack lists a finished circuit
keeps, the classification and the refusals.  Never loaded into Python, never run on a GPU."""
import os
import shutil
import subprocess

import pytest

from zksnark_rs_amd import SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 2, 63, 64, 65, 128, 253)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("builder_pack_host") / "builder_pack_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "builder_pack_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


@pytest.mark.parametrize("fill", ["ones", "random"])
def test_pack_host_code_under_sanitizers(host_exe, fill):
    rng = SplitMix64(7)
    data = bytes([0xFF] * 32) if fill == "ones" else bytes(rng.next() & 0xFF for _ in range(32))
    value = int.from_bytes(data, "little")
    res = subprocess.run([host_exe], input=data.hex() + "\n", capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    for k, width in enumerate(WIDTHS):
        assert lines[k] == "pack %d %064x" % (width, value & ((1 << width) - 1))
    # wires: inputs 2 3 4, the XOR 5, the packs 6 and 7; witness order [1], pack 7 (verify), the inputs, 5, 6; m = 7 stands for the zero wire
    assert lines[7] == "lists 6 1 | 0 6 7 | 4 7 5 0 4 7 7"
    assert lines[8] == "boolean 1 0 0"
    assert lines[9] == "refused 5 of 5"
