"""CPU: the host side of the device image reader (sfmloc_imread): its entry points are in the header-derived bindings,
both localisation tools know --device-decode, and the JPEG decoder's split (csrc/jpeg_host.h: entropy stage into the
caller's memory, then the host reconstruction from it) gives sfmloc_image_decode's bytes under the host sanitizers."""
import os
import shutil
import subprocess

import imread_files as F
import sfmlocalization_amd as S
from sfmlocalization_amd import _abi, capi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVGLocalization_AKAZE")


def test_the_entry_points_are_bound_from_the_header():
    names = ["sfmloc_imread_create", "sfmloc_imread_destroy", "sfmloc_imread_decode", "sfmloc_imread_file",
             "sfmloc_imread_read", "sfmloc_imread_dev", "sfmloc_imread_share_stream", "sfmloc_imread_timing",
             "sfmloc_akaze_detect_resident_dev", "sfmloc_akaze_detect_and_compute_dev", "sfmloc_imgbow_compute_dev"]
    L = capi._L()
    for n in names:
        assert n in _abi.PROTOTYPES and n in capi.SYMBOLS, n
        assert getattr(L, n).argtypes == _abi.PROTOTYPES[n][1]
    assert (capi.IMREAD_GRAY, capi.IMREAD_BGR, capi.IMREAD_BGR2GRAY) == (1, 2, 4)
    assert _abi.constants("ABI_VERSION") == (2,)           # entry points were added, no struct changed
    for cls, methods in ((capi.DeviceImread, ("decode", "file", "read", "dev", "share_stream", "close")),
                         (capi.Akaze, ("detect_and_compute_dev", "detect_resident_dev")), (capi.ImgBow, ("compute_dev",))):
        for m in methods:
            assert callable(getattr(cls, m))
    assert S.DeviceImread is capi.DeviceImread


def test_both_tools_know_the_switch():
    _, o = engine.parse_cv_args(["q", "sfm", "matches", "out"], engine.KEYS)
    assert o["device-decode"] is False                                            # without it nothing changes
    _, o = engine.parse_cv_args(["q", "sfm", "matches", "out", "--device-decode"], engine.KEYS)
    assert o["device-decode"] is True
    _, o = engine.parse_cv_args(["q", "sfm", "matches", "out", "--device-decode=false"], engine.KEYS)
    assert o["device-decode"] is False
    import inspect
    assert inspect.signature(engine.LocalizeEngine.localize_file).parameters["device_decode"].default is False
    # the C++ tool: its usage names the switch, and its argument table reads it
    r = subprocess.run([CLI_BIN, "--device-decode"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[--device-decode]" in r.stdout
    with open(os.path.join(ROOT, "sfmlocalization_amd", "csrc", "localize_cli.cpp")) as f:
        assert 'a.flag({"device-decode"})' in f.read()
    with open(os.path.join(ROOT, "include", "sfmloc_engine.hpp")) as f:
        assert "bool deviceDecode = false" in f.read()


def test_the_split_decoder_under_the_host_sanitizers(tmp_path):
    """tests/cpp/jpeg_coef.cpp: a stand-alone host program, CPU only, linked with image_io.hip's host code alone.  Where a
    HIP device is visible it is built without the sanitizers (they are for CPU machines); it checks the same things."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    san = [] if S.device_count() > 0 else ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                            "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "jpeg_coef")
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-w", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "jpeg_coef.cpp"),
                    os.path.join(ROOT, "sfmlocalization_amd", "csrc", "image_io.hip"), "-lz"], check=True, timeout=600)
    files = [os.path.join(F.IMAGES, n) for n in F.golden_jpegs()] + [os.path.join(F.EDGES, n) for n in F.edge_jpegs()]
    for name, data in (("beyond32.jpg", F.with_16bit_quant_of_65535(F.golden("base_420.jpg"))),
                       ("rgb.jpg", F.as_rgb_file(F.golden("base_420.jpg")))):
        (tmp_path / name).write_bytes(data)
        files.append(str(tmp_path / name))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == f"OK {len(files)} files" and len(files) >= 60
