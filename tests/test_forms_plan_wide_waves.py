"""CPU: K3Plan::wide_waves (sfmlocalization_amd/csrc/forms.h) -- the waves per workgroup of K3's wide 1 024-match
instance follow SFMLOC_K3_WIDE_WAVES (4 or 8), the 2 048-match instance keeps four, gang sessions and lists above 256
views stay plain, and no other field of the plan moves with the knob -- checked by a host program
(tests/cpp/forms_plan_wide_waves.cpp) that includes the header the launch functions include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_waves_plan_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/forms_plan_wide_waves.cpp")
    exe = str(tmp_path / "forms_plan_wide_waves")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "forms_plan_wide_waves.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
