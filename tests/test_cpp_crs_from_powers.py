"""groth16::setup_from_powers of include/zksnark.hpp and zk_crs_from_powers of include/zkgpu.h through
tests/cpp/crs_from_powers_api.cpp, run the way tests/test_cpp_crs_check.py runs its program.

not gpu: the program compiles and links against libzkgpu.so, which exports the symbol by name (no device call is made).
gpu:     it runs on the device and every test prints "ok"."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crs_from_powers_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")


def build(out_dir):
    exe = os.path.join(str(out_dir), "crs_from_powers_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_the_symbol_is_exported_and_bound():
    """the ABI surface of this feature, by name: the library exports zk_crs_from_powers and the binding types it"""
    from zksnark_rs_amd import _lib
    assert hasattr(ctypes.CDLL(os.path.join(LIBDIR, "libzkgpu.so")), "zk_crs_from_powers")
    res, args = _lib.SIGNATURES["zk_crs_from_powers"]
    assert res is ctypes.c_int and len(args) == 4 and args[2] is ctypes.POINTER(_lib.PowersDesc)
    assert [f[0] for f in _lib.PowersDesc._fields_] == ["n_tau_g1", "n_rest", "tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"]


def test_crs_from_powers_cpp_api_compiles_and_links(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_setup_from_powers_through_cpp_api(tmp_path):
    exe = build(tmp_path)
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("from_powers_equals_setup", "from_powers_refusals"):
        assert "ok " + name in res.stdout, res.stdout + res.stderr
