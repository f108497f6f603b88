"""CPU: the one rule by which a launch raises its kernel's dynamic-LDS limit (sfmlocalization_amd/csrc/devmem.h
"Dynamic-LDS limits", applied by dev_launch of csrc/launch.h to every launch of the library) -- checked by a host program
(tests/cpp/launch.cpp) that includes the header the library includes and supplies a raw function that logs its calls and
can be told to fail: 48 KiB or less makes no raw call; more makes exactly one, and the same or less afterwards none; a
second device ordinal and a second kernel have marks of their own; a failed raw call answers its code, leaves the mark,
and the next request tries again.  Where no HIP device is visible the program is built with the host sanitizers (they are
for CPU machines)."""
import os
import shutil
import subprocess

import pytest

import sfmlocalization_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_limit_marks_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/launch.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "launch")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "launch.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
