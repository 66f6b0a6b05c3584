"""eddsa::sign_batch of include/zksnark.hpp through tests/cpp/eddsa_sign_api.cpp.

not gpu: the program compiles, links against libzkgpu.so and runs its host part.
gpu:     65 instances signed on the device verify on the device, instance 0 equals eddsa::sign, a key of 0 refuses the call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "eddsa_sign_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")


def build(out_dir):
    exe = os.path.join(str(out_dir), "eddsa_sign_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_eddsa_sign_cpp_api_links_without_a_gpu(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    assert "ok links_on_the_host" in run(exe, "host")


@pytest.mark.gpu
def test_eddsa_sign_through_cpp_api(tmp_path):
    out = run(build(tmp_path), "gpu")
    for name in ("links_on_the_host", "batch_on_the_device"):
        assert "ok " + name in out, out
