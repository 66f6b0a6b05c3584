"""groth16::ResidentPowers / check_powers / contribute_powers / check_powers_contribution of include/zksnark.hpp (over zk_powers_*) and
the C ABI's argument refusals, through tests/cpp/powers_api.cpp, run the way tests/test_cpp_crs_contribute.py runs its program; and the
surface of the new symbols (header, library, Python signatures, Rust declarations).

not gpu: the program compiles and links against libzkgpu.so (no device call is made); the surface.
gpu:     it runs on the device and every test prints "ok"."""
import os
import re
import subprocess

import pytest

from zksnark_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "powers_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")
NEW_SYMBOLS = ["zk_g1_mul_each", "zk_g2_mul_each", "zk_powers_upload", "zk_powers_initial", "zk_powers_dims", "zk_powers_download",
               "zk_powers_free", "zk_powers_check", "zk_powers_contribution_prove", "zk_powers_contribution_verify", "zk_powers_contribute",
               "zk_powers_contribution_check"]


def build(out_dir):
    exe = os.path.join(str(out_dir), "powers_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_powers_cpp_api_compiles_and_links(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    assert os.path.exists(exe)


def test_the_new_symbols_are_declared_exported_and_bound():
    """every new entry point is in include/zkgpu.h, exported by the library, typed in _lib.SIGNATURES and declared to Rust"""
    header = open(os.path.join(ROOT, "include", "zkgpu.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|void) %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
        assert re.search(r"\bfn %s\(" % name, rust), name
    assert "ZK_LAZY_REGULAR_RECODE = 10" in open(os.path.join(ROOT, "include", "zkgpu_measure.h")).read()
    bits = dict(re.findall(r"#define ZK_POWERS_CHECK_(\w+) (0x[0-9a-f]+)u", header))
    assert {k: int(v, 16) for k, v in bits.items()} == {n: 1 << k for k, n in enumerate(_lib.POWERS_CHECK_BITS) if n}


@pytest.mark.gpu
def test_powers_through_cpp_api(tmp_path):
    exe = build(tmp_path)
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "zk")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("powers_ceremony", "powers_records", "powers_errors"):
        assert "ok " + name in res.stdout, res.stdout + res.stderr
