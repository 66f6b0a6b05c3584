"""The arithmetic mod l of csrc/eddsa_modl.hpp, which zk_eddsa_sign_batch's kernels compute S with, on raw triples (rho, h, k) through
tests/cpp/eddsa_modl_check.hip, held against Python integers: h % l by the three conditional subtractions (every quotient 0..7) and
(rho + 8 (h % l) k) % l by the schoolbook product and Barrett's reduction, and the constants l, 2 l, 4 l and floor(2^512 / l) the header
derives at compile time.  Signing can never choose h, so this is the only way to the edges.

not gpu: the program built --cuda-host-only under ASan + UBSan, run in its --host mode: a stand-alone program, never loaded into
         Python, never run on a GPU.
gpu:     the program built as the library is built, run once in a fresh child process under a time limit: the same functions on the
         host and in a one-block kernel."""
import os
import re
import shutil
import subprocess

import pytest

from zksnark_rs_amd import SplitMix64

import babyjub_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zksnark_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "eddsa_modl_check.hip")
R, L = bm.R, bm.L
assert 7 * L < R < 8 * L


def triples():
    """the cross product of the edges, then 64 drawn triples: rho, k < l (k != 0), h < r"""
    out = [(rho, h, k) for rho in (0, 1, L - 1) for h in (0, 1, L - 1, L, 4 * L - 1, 4 * L, 7 * L - 1, 7 * L, R - 1) for k in (1, 2, L - 1, 1 << 250)]
    rng = SplitMix64(3600)
    out += [(rng.fr() % L, rng.fr(), rng.fr() % L or 1) for _ in range(64)]
    assert {h // L for _, h, _ in out} == set(range(8))      # every quotient of the conditional subtractions
    return out


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("no hipcc")
    return exe


def check(stdout, tags):
    ts = triples()
    lines = stdout.strip().splitlines()
    want = ["l %064x" % L, "l2 %064x" % (2 * L), "l4 %064x" % (4 * L), "mu %072x" % ((1 << 512) // L)]
    for tag in tags:
        want += ["%s %d %064x %064x" % (tag, i, h % L, (rho + 8 * (h % L) * k) % L) for i, (rho, h, k) in enumerate(ts)]
    assert len(lines) == len(want)
    bad = [(g, w) for g, w in zip(lines, want) if g != w]
    assert not bad, bad[:3]


def stdin_text():
    return "".join("%064x %064x %064x\n" % t for t in triples())


def test_modl_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "eddsa_modl_check")
    subprocess.run([hipcc(), "-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-DMODL_CHECK_HOST_ONLY", "-I", CSRC, "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    res = subprocess.run([exe, "--host"], input=stdin_text(), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr
    check(res.stdout, ["host"])


def library_flags():
    """CXXFLAGS of csrc/Makefile, read (not copied) so that the program is compiled exactly as the library is"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda n: re.search(r"^%s \?= (.*)$" % n, text, re.M).group(1).strip()       # noqa: E731
    return var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


@pytest.mark.gpu
def test_modl_in_a_kernel(tmp_path):
    exe = str(tmp_path / "eddsa_modl_check")
    subprocess.run([hipcc()] + library_flags() + ["-I", CSRC, SRC, "-o", exe], check=True, capture_output=True, text=True, timeout=900)
    res = subprocess.run(["timeout", "-k", "10", "120", exe], input=stdin_text(), capture_output=True, text=True)
    assert res.returncode == 0, "eddsa_modl_check exited with %d\n%s%s" % (res.returncode, res.stdout, res.stderr)
    check(res.stdout, ["host", "device"])
