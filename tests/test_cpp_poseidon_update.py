"""PoseidonTree::update / PoseidonTree::append of include/zksnark.hpp through tests/cpp/poseidon_update_api.cpp.

not gpu: the program compiles, links against libzkgpu.so (both ABI symbols resolve) and runs its host part.
gpu:     one update and one append on the device against trees built over the final leaves, and three refusals; every test prints
         "ok"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "poseidon_update_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")
HOST_TESTS = ("api_links",)


def build(out_dir):
    exe = os.path.join(str(out_dir), "poseidon_update_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_poseidon_update_cpp_api_host_part(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    out = run(exe, "host")
    for name in HOST_TESTS:
        assert "ok " + name in out, out


@pytest.mark.gpu
def test_poseidon_update_through_cpp_api(tmp_path):
    out = run(build(tmp_path), "gpu")
    for name in HOST_TESTS + ("update_and_append_on_the_device",):
        assert "ok " + name in out, out
