"""CPU: the operand expansion of the matrix-core Hamming scan (sfmlocalization_amd/csrc/k1_mfma_expand.h) satisfies
(512 - <a', b'>) / 2 = popcount(a ^ b) over random and extreme 64-byte rows, with both operands walking K in the same
order -- checked by a host program (tests/cpp/k1_mfma_identity.cpp) that includes the header the kernel includes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expansion_identity_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/k1_mfma_identity.cpp")
    exe = str(tmp_path / "k1_mfma_identity")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "k1_mfma_identity.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
