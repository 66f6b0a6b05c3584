"""eddsa::challenge / public_key / sign / verify / verify_batch and builder::Circuit::eddsa_verify of include/zksnark.hpp through
tests/cpp/eddsa_api.cpp.

not gpu: the program compiles, links against libzkgpu.so and runs its host part (the scheme and the gadget need no context); the
         values it prints are the model's.
gpu:     batch verification on the device with strided bit rows; every test prints "ok"."""
import os
import subprocess

import pytest

import eddsa_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "eddsa_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")
HOST_TESTS = ("scheme_on_the_host", "gadget_on_the_host")
K1 = 0x0096a5b4c3d2e1f00f1e2d3c4b5a6978fedcba98765432100123456789abcdef


def build(out_dir):
    exe = os.path.join(str(out_dir), "eddsa_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_eddsa_cpp_api_host_part(tmp_path):
    try:
        exe = build(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    out = run(exe, "host")
    for name in HOST_TESTS:
        assert "ok " + name in out, out
    values = {line.split()[1]: tuple(int(x, 16) for x in line.split()[2:]) for line in out.splitlines() if line.startswith("value ")}
    r8, s = em.sign(K1, 9, 1234)
    assert values == {"challenge": (em.H6_12345,), "signature": (r8[0], r8[1], s)}


@pytest.mark.gpu
def test_eddsa_through_cpp_api(tmp_path):
    out = run(build(tmp_path), "gpu")
    for name in HOST_TESTS + ("batch_on_the_device",):
        assert "ok " + name in out, out
