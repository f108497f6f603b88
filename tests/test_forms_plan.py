"""CPU: the kernel-form policy of K1 / K3 / K5 (sfmlocalization_amd/csrc/forms.h: thresholds, knobs, credits and the
per-stage plans the launch functions follow) gives, boundary by boundary, the plans DESIGN.md's "Kernel forms" table
describes -- checked by a host program (tests/cpp/forms_plan.cpp) that includes the header the launch functions
include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_form_plans_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/forms_plan.cpp")
    exe = str(tmp_path / "forms_plan")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "forms_plan.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
