"""groth16::contribute / check_contribution of include/zksnark.hpp (over zk_crs_contribute / zk_crs_contribution_check) through
tests/cpp/crs_contribute_api.cpp, run the way tests/test_cpp_crs_check.py runs its program.

not gpu: the program compiles and links against libzkgpu.so (no device call is made).
gpu:     it runs on the device and every test prints "ok"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crs_contribute_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")


def build(out_dir):
    exe = os.path.join(str(out_dir), "crs_contribute_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_crs_contribute_cpp_api_compiles_and_links(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_contribute_through_cpp_api(tmp_path):
    exe = build(tmp_path)
    env = dict(os.environ, ZK_TEST_TMP=str(tmp_path))
    res = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "zk")], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    for name in ("contribute_parsed", "contribute_chain", "contribute_file", "contribute_errors"):
        assert "ok " + name in res.stdout, res.stdout + res.stderr
