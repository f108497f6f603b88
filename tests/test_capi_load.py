"""CPU: the C-ABI library loads, exports every symbol include/sfmloc.h declares, and compute entry
points fail loudly without a GPU.  (The layout of the structs: tests/test_abi.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import sfmlocalization_amd as S
from sfmlocalization_amd import capi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sfmloc.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sfmloc_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = _lib.load()
    names = declared_symbols()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/sfmloc.h but not exported"
    assert sorted(capi.SYMBOLS) == names, "capi.SYMBOLS out of date with include/sfmloc.h"
    assert capi._L().sfmloc_abi_version() == 2      # 2: sfmloc_params.guided_matching


def test_host_only_entry_points_without_another_caller(tmp_path):
    """sfmloc_view_list_open / _get / _close have no Python wrapper (the C++ tools call them); sfmloc_pack on a directory
    without sfm_data.json is the file contract's refusal.  Both run on the host."""
    L = capi._L()
    with pytest.raises(S.SfmlocError) as ei:
        capi.pack(str(tmp_path), str(tmp_path), str(tmp_path / "map.bin"))
    assert ei.value.code == capi.EIO
    (tmp_path / "sfm_data.json").write_text(
        '{"sfm_data_version": "0.2", "root_path": "/img", "views": [{"key": 3, "value": {"polymorphic_id": 1073741824, '
        '"ptr_wrapper": {"id": 2147483649, "data": {"local_path": "/", "filename": "a.jpg", "width": 640, "height": 480, '
        '"id_view": 3, "id_intrinsic": 0, "id_pose": 3}}}}], "intrinsics": [], "extrinsics": [], "structure": [], '
        '"control_points": []}')
    lst, n = ctypes.c_void_p(), ctypes.c_uint32()
    capi._check(L.sfmloc_view_list_open(os.fsencode(tmp_path / "sfm_data.json"), ctypes.byref(lst), ctypes.byref(n)))
    vid, w, h, path = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_char_p()
    capi._check(L.sfmloc_view_list_get(lst, 0, ctypes.byref(vid), ctypes.byref(w), ctypes.byref(h), ctypes.byref(path)))
    assert (n.value, vid.value, w.value, h.value, path.value) == (1, 3, 640, 480, b"/img/a.jpg")
    assert L.sfmloc_view_list_get(lst, 1, None, None, None, None) == capi.EINVAL
    assert L.sfmloc_view_list_close(lst) is None
    assert L.sfmloc_view_list_open(os.fsencode(tmp_path / "none.json"), ctypes.byref(lst), ctypes.byref(n)) == capi.EIO


def test_default_params_are_the_reference_defaults():
    p = S.default_params()
    assert abs(p.dist_ratio - 0.6) < 1e-7      # localization.cpp:70
    assert p.ransac_round == 200               # localization.cpp:71
    assert p.geom_precision == 4.0             # localization.cpp:81
    assert (p.min_putative, p.min_resection_points, p.min_inliers) == (16, 8, 10)  # localization.cpp:56-58
    assert p.p3p_max_iteration == 4096
    assert p.refine_pose == 0


def test_no_cpu_fallback():
    if S.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(S.SfmlocError) as ei:
        S.Map([0], [0, 1], np.zeros((1, 64), np.uint8))
    assert ei.value.code == capi.ENODEV
    assert "no CPU fallback" in str(ei.value)
