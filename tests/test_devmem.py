"""CPU: the owners of device memory that Map, Ctx and Query are built from (sfmlocalization_amd/csrc/devmem.h: DevBuf,
DevGroup) charge and refund their account, never free a borrowed pointer, and a group that fails part-way leaves its
owners, the account and the count of live allocations exactly as they were -- checked by a host program
(tests/cpp/devmem.cpp) that includes the header the library includes and supplies raw allocation over malloc.  The same
program checks the header's owners of streams, events and pinned host memory (Stream, Event, HostBuf) over counters and a
log of raw calls: released exactly once, empty after a failed creation, a borrowed stream never touched, a handle's
buffers freed before its stream goes.  And the header's transfers over memcpy / memset: element counts become bytes, an
owned buffer refuses a span outside it, zero elements issue nothing, a null stream is waited for and a stream is not.
Where no HIP device is visible the program is built with the host sanitizers (they are for CPU machines)."""
import os
import shutil
import subprocess

import pytest

import sfmlocalization_amd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_memory_owners_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/devmem.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "devmem")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "devmem.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
