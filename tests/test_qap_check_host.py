"""zk_qap_check / zk_qap_check_dev without a device: the null-argument behaviour, the 12-byte result record in every binding, and the
C++ host API's program (tests/cpp/qap_check_api.cpp) compiling and linking.  The device side: tests/test_gpu_qap_check.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "qap_check_api.cpp")
LIBDIR = os.path.join(ROOT, "zksnark_rs_amd")


def build_qap_check_api(out_dir):
    """as tests/test_cpp_api.py builds its program"""
    exe = os.path.join(str(out_dir), "qap_check_api")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
           "-L", LIBDIR, "-lzkgpu", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lamdhip64"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_null_arguments_without_a_device():
    from zksnark_rs_amd import _lib
    lib = _lib.load()
    out = _lib.QapCheckResult(7, 7, 7)
    w = (C.c_uint64 * 4)(1, 0, 0, 0)
    fake = C.c_void_p(8)            # never dereferenced: every call below fails on a null argument first
    assert lib.zk_qap_check(None, None, None, 0, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(None, fake, w, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(fake, None, w, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(fake, fake, w, 1, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check(fake, fake, None, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(None, None, None, 0, 0, 0, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(None, fake, fake, 1, 1, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(fake, None, fake, 1, 1, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(fake, fake, fake, 1, 1, 1, None) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(fake, fake, None, 1, 1, 1, C.byref(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_qap_check_dev(fake, fake, fake, 2, 1, 1, C.byref(out)) == _lib.ZK_ERR_ARG      # stride < m
    assert (out.bad_gates, out.first_bad, out.flags) == (7, 7, 7)


def test_result_record_is_12_bytes_in_every_binding():
    from zksnark_rs_amd import _lib
    import numpy as np
    import zksnark_rs_amd as zk
    assert C.sizeof(_lib.QapCheckResult) == 12
    assert [f[0] for f in _lib.QapCheckResult._fields_] == ["bad_gates", "first_bad", "flags"]
    assert zk.Context.QAP_CHECK_DTYPE.itemsize == 12 and zk.Context.QAP_CHECK_DTYPE.names == ("bad_gates", "first_bad", "flags")
    header = open(os.path.join(ROOT, "include", "zkgpu.h")).read()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*zk_qap_check_result\s*;", header)
    fields = re.findall(r"\b(uint32_t)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [("uint32_t", "bad_gates"), ("uint32_t", "first_bad"), ("uint32_t", "flags")]
    assert int(re.search(r"#define\s+ZK_QAP_CHECK_NONE\s+(0x[0-9A-Fa-f]+)u", header).group(1), 16) == _lib.QAP_CHECK_NONE
    assert int(re.search(r"#define\s+ZK_QAP_CHECK_WIRE0\s+(\d+)u", header).group(1)) == _lib.QAP_CHECK_WIRE0
    assert "(1u << 28)" in re.search(r"#define\s+ZK_QAP_CHECK_CHUNK_LANES\s+(.*)", header).group(1) and _lib.QAP_CHECK_CHUNK_LANES == 1 << 28
    assert "static_assert(sizeof(zk_qap_check_result) == 12" in open(SRC).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*pub struct ZkQapCheckResult \{([^}]*)\}", rust)
    assert [x.strip() for x in m.group(1).split(",")] == ["pub bad_gates: u32", "pub first_bad: u32", "pub flags: u32"]
    assert "fn zk_qap_check(" in rust and "fn zk_qap_check_dev(" in rust and "pub fn is_satisfied(" in rust
    assert np.dtype(np.uint32).itemsize * 3 == 12


def test_python_apis_exist():
    import zksnark_rs_amd as zk
    from zksnark_rs_amd import groth16
    from zksnark_rs_amd.circuit import Witgen
    assert callable(zk.Context.qap_check) and callable(zk.Context.qap_check_dev)
    assert callable(groth16.is_satisfied) and callable(groth16.first_unsatisfied) and callable(Witgen.run_checked)


def test_cpp_program_compiles_and_links(tmp_path):
    try:
        exe = build_qap_check_api(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail("g++ failed:\n" + e.stderr[-3000:])
    assert os.path.exists(exe)
