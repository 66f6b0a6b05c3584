"""-m "not gpu": the split of a built circuit and its host runner (csrc/builder.hpp: built_split, mixed_run_host) as a stand-alone
program under ASan + UBSan (tests/cpp/mixgen_host.hip): packs of every width at a limb edge read by the tail, every gate kind on a
field operand, a circuit without boolean operations, the refusals.  Never loaded into Python, never run on a GPU."""
import os
import shutil
import subprocess

import pytest

import builder_model as bm
import mixed_model as mm
from zksnark_rs_amd import SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 63, 64, 65, 128, 253)
R = bm.R
ORDER = ("n_bit_inputs", "n_field_inputs", "core_ops", "core_levels", "tail_ops", "tail_levels", "tail_slots")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("mixgen_host") / "mixgen_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-I", os.path.join(ROOT, "zksnark_rs_amd", "csrc"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "cpp", "mixgen_host.hip"), "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    return exe


def gates_case(b):
    """the second circuit of the program"""
    x = b.new_bits(6)
    f = [b.new_field(), b.new_field()]
    g = b.gate("nor", x[0], x[1])
    fg = b.gate("and", x[2], f[0])
    p0 = b.pack([x[3], g, bm.ONE, bm.ZERO, x[3]])
    p1 = b.pack([x[4], fg, bm.ONE])
    last = None
    for kind in bm.GATE_KINDS:
        un = kind in bm.UNARY
        b.gate(kind, f[1], None if un else x[5])
        last = b.gate(kind, g, None if un else f[1])
        last = b.gate(kind, p0, None if un else last)
        last = b.gate(kind, x[5], None if un else g)
    b.assert_bit(f[0])
    b.assert_bit(last)
    return [p1, last]


def field_only_case(b):
    f = [b.new_field(), b.new_field()]
    t = b.sub_circuit([(3, f[0]), (R - 1, f[1])], [(1, f[1])])
    return [b.sub_circuit([(1, t)], [(1, bm.ONE)])]


def dims_line(case):
    model = mm.SplitModel()
    fin = model.finish(case(model))
    shape = mm.mixed_shape(model, fin)
    return " ".join(str(shape[k]) for k in ORDER), model


@pytest.mark.parametrize("fill", ["ones", "random"])
def test_split_and_host_runner_under_sanitizers(host_exe, fill):
    rng = SplitMix64(11)
    data = bytes([0xFF] * 32) if fill == "ones" else bytes(rng.next() & 0xFF for _ in range(32))
    value = int.from_bytes(data, "little")
    res = subprocess.run([host_exe], input=data.hex() + "\n", capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    lines = res.stdout.strip().splitlines()
    for k, width in enumerate(WIDTHS):
        v = value & ((1 << width) - 1)
        assert lines[k] == "pack %d %064x %064x" % (width, v, (v + 7 * (R - 1)) * v % R)
    dims, model = dims_line(gates_case)
    assert lines[6] == "dims %s | 1 0" % dims
    assert model.cat.count("core") > 10 and model.cat.count("tail") > 20
    assert lines[7] == "gates 64"
    assert lines[8] == "field-only " + dims_line(field_only_case)[0]
    assert lines[9] == "refused 4 of 4"
