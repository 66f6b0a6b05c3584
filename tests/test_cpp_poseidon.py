"""poseidon::hash / zero_hashes / hash_batch, PoseidonTree and builder::Circuit::poseidon / merkle_root of include/zksnark.hpp through
tests/cpp/poseidon_api.cpp.

not gpu: the program compiles, links against libzkgpu.so and runs its host part (the hash and the gadgets need no context).
gpu:     batch hashing, a tree, its paths and the membership circuit's witnesses on the device; every test prints "ok"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "poseidon_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")
HOST_TESTS = ("hash_and_refusals", "gadgets_on_the_host")


def build(out_dir):
    exe = os.path.join(str(out_dir), "poseidon_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_poseidon_cpp_api_host_part(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    out = run(exe, "host")
    for name in HOST_TESTS:
        assert "ok " + name in out, out


@pytest.mark.gpu
def test_poseidon_through_cpp_api(tmp_path):
    out = run(build(tmp_path), "gpu")
    for name in HOST_TESTS + ("tree_paths_and_witnesses_on_the_device",):
        assert "ok " + name in out, out
