"""CPU: the restatement of the landmark colouring (tests/colorize_np.py) and the package's sampler and PLY writer
(sfmlocalization_amd/colorize.py) on cases small enough to verify by hand -- the expected plans and PLY texts are
written out below.  The device plan is checked against the restatement in tests/test_gpu_colorize.py."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import colorize_np as CN  # noqa: E402
import colorize_scene as CS  # noqa: E402
from sfmlocalization_amd import adjust, capi, colorize, globalcoord, hulo  # noqa: E402

GOLD = os.path.join(HERE, "golden", "images")
U = CN.UNSET


def np_plan(arrays, device=0):
    return CN.plan(len(arrays["view_id"]), arrays["obs_off"], arrays["obs_view"])


def test_three_views_five_landmarks_tie_on_the_first_choice():
    # observations (index: view)   L0: 0:v0 1:v1   L1: 2:v0 3:v2   L2: 4:v1   L3: 5:v1 6:v2   L4: 7:v2 8:v0
    # counts 3 3 3 -> view 0 (lowest index) colours L0 L1 L4; then L2 L3 are left: counts 0 2 1 -> view 1
    off, view = CS.csr([[0, 1], [0, 2], [1], [1, 2], [2, 0]])
    order, it, ob = CN.plan(3, off, view)
    assert order.tolist() == [0, 1]
    assert it.tolist() == [0, 0, 1, 1, 0]
    assert ob.tolist() == [0, 2, 4, 5, 8]


def test_landmark_seen_by_every_view_unobserved_view_and_landmark_without_observations():
    # views 0..3, view 3 observed by nobody   L0: 0:v0 1:v1 2:v2   L1: 3:v2   L2: none   L3: 4:v1 5:v2
    # counts 1 2 3 0 -> view 2 colours L0 L1 L3 and nothing is left: one iteration, L2 stays uncoloured
    off, view = CS.csr([[0, 1, 2], [2], [], [1, 2]])
    order, it, ob = CN.plan(4, off, view)
    assert order.tolist() == [2]
    assert it.tolist() == [0, 0, U, 0]
    assert ob.tolist() == [2, 3, 0, 5]
    order, it, ob = CN.plan(2, *CS.csr([]))
    assert len(order) == len(it) == len(ob) == 0


def test_a_view_named_twice_counts_twice_and_is_read_at_its_first():
    # L0: 0:v1 1:v1   L1: 2:v0   L2: 3:v0   -> counts 2 2 -> view 0 (L1, L2), then view 1 (L0 at observation 0)
    order, it, ob = CN.plan(2, *CS.csr([[1, 1], [0], [0]]))
    assert (order.tolist(), it.tolist(), ob.tolist()) == ([0, 1], [1, 0, 0], [0, 2, 3])


def pattern(v, w=4, h=3):
    """pixel (y, x) of view v = (r, g, b) = (10 v + x, 100 + y, 200 + v)"""
    img = np.zeros((h, w, 3), np.uint8)
    img[:, :, 0] = 10 * v + np.arange(w)[None, :]
    img[:, :, 1] = 100 + np.arange(h)[:, None]
    img[:, :, 2] = 200 + v
    return img


def small_project(folder):
    """three 4 x 3 views (0 and 2 with a pose) and four landmarks:
       L0 (key 10) v0 at (3.99, 0.2), v1     L1 (key 13) v0 at (-0.5, 2.999)     L2 (key 16) no observations
       L3 (key 19) v1 at (4.0, 1.5) [x = width], v2 at (1, 1)
    counts 2 2 1 -> view 0 colours L0, L1; then 0 1 1 -> view 1 colours L3"""
    names = ["a.ppm", "b.ppm", "c.ppm"]
    for v, n in enumerate(names):
        CS.write_ppm(os.path.join(folder, n), pattern(v))
    lms = [([1.5, -2, 3], [(0, 3.99, 0.2), (1, 1.0, 1.0)]), ([0.25, 1e-05, 1234567.0], [(0, -0.5, 2.999)]),
           ([7, 8, 9], []), ([-1, 0, 100000.5], [(1, 4.0, 1.5), (2, 1.0, 1.0)])]
    return CS.document(folder, names, [(4, 3)] * 3, {0: [0, 0.5, -1], 2: [1e6, 2, 3.14159265]}, lms, 10, 3)


SMALL_PLY = """ply
format ascii 1.0
element vertex 6
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
end_header
1.5 -2 3 3 100 200
0.25 1e-05 1.23457e+06 0 102 200
7 8 9 0 0 0
-1 0 100000 13 101 201
0 0.5 -1 0 255 0
1e+06 2 3.14159 0 255 0
"""


def test_sampler_truncates_clamps_and_writes_the_ply(tmp_path):
    doc = small_project(str(tmp_path))
    out = str(tmp_path / "out.ply")
    assert colorize.colorize_doc(doc, out, plan_fn=np_plan) == 0
    assert open(out).read() == SMALL_PLY
    assert CN.document_ply(doc, lambda p: capi.image_read(p, color=True)) == SMALL_PLY
    assert colorize.pixel([3.99, -0.5, 4.0, -7.0, 0.0, float("nan"), 1e30], 4).tolist() == [3, 0, 3, 0, 0, 0, 3]


def test_structure_and_camera_forms_and_an_unreadable_image(tmp_path, capsys):
    doc = small_project(str(tmp_path))
    sfm = str(tmp_path / "sfm_data.json")
    with open(sfm, "w") as fh:
        json.dump(doc, fh)
    head, body = SMALL_PLY.split("end_header\n")
    head, body = head + "end_header\n", body.splitlines(True)
    # structure = []: the camera centres alone, and no plan is needed (no device call)
    assert colorize.save_camera_ply(sfm, str(tmp_path / "cam.ply")) == 0
    assert open(tmp_path / "cam.ply").read() == head.replace("vertex 6", "vertex 2") + "".join(body[4:])
    # extrinsics = []: the landmarks alone
    assert colorize.run(sfm, str(tmp_path / "st.ply"), edit=lambda d: d.__setitem__("extrinsics", []), plan_fn=np_plan) == 0
    assert open(tmp_path / "st.ply").read() == head.replace("vertex 6", "vertex 4") + "".join(body[:4])
    # an image that cannot be read: status 1, the file's name, nothing written
    os.remove(tmp_path / "b.ppm")
    assert colorize.run(sfm, str(tmp_path / "bad.ply"), plan_fn=np_plan) == 1
    assert str(tmp_path / "b.ppm") in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "bad.ply")
    assert colorize.run(str(tmp_path / "missing.json"), str(tmp_path / "bad.ply")) == 1
    assert not os.path.exists(tmp_path / "bad.ply")


def test_gray_png_and_colour_jpeg(tmp_path):
    exp = np.load(os.path.join(GOLD, "expected.npz"))
    gray, jpg = exp["png_gray_bgr"], exp["base_444_rst_bgr"]            # 30 x 21 and 64 x 48
    lms = [([0, 0, 1], [(0, 7.9, 3.2)]), ([0, 0, 2], [(0, 29.0, 20.0)]), ([0, 0, 3], [(1, 40.5, 17.5)]),
           ([0, 0, 4], [(1, 63.99, 47.0)]), ([0, 0, 5], [(1, 5.0, 9.0)])]
    doc = CS.document(GOLD, ["gray.png", "base_444_rst.jpg"], [(30, 21), (64, 48)], {}, lms)
    arrays, _, _ = adjust.sfm_arrays(doc)
    plan = np_plan(arrays)
    assert plan[0].tolist() == [1, 0]                                  # counts 2 3
    rgb = colorize.sample(doc, arrays, plan)
    want = [gray[3, 7], gray[20, 29], jpg[17, 40], jpg[47, 63], jpg[9, 5]]
    assert rgb.tolist() == [w[::-1].tolist() for w in want]
    assert (rgb[0][0] == rgb[0][1] == rgb[0][2]) and (rgb[1][0] == rgb[1][1] == rgb[1][2])   # gray: three equal channels
    assert len({tuple(c) for c in rgb[2:].tolist()}) > 1 and any(c[0] != c[2] for c in rgb[2:].tolist())


def test_save_global_ply(tmp_path):
    src = tmp_path / "in.ply"
    src.write_text("ply \nformat ascii 1.0\nelement vertex 2\n  END_HEADER\n1 2 3 10 20 30\n\n 0.5   -1 2.25 0 255 0 \n")
    A = np.array([[2.0, 0, 0, 1], [0, 2.0, 0, -1], [0, 0, 0.5, 0.125]])
    colorize.save_global_ply(str(src), A, str(tmp_path / "out.ply"))
    assert (tmp_path / "out.ply").read_text() == ("ply\nformat ascii 1.0\nelement vertex 2\nEND_HEADER\n"
                                                  "3.0 3.0 1.625 10 20 30 \n2.0 -3.0 1.25 0 255 0 \n")


def test_arguments():
    assert colorize.parse_args(["-i", "a.json", "-o", "b.ply"]) == ("a.json", "b.ply", 0)
    assert colorize.parse_args(["--output_file=b.ply", "--input_file", "a.json", "--device=2"]) == ("a.json", "b.ply", 2)
    for bad in ([], ["-i", "a.json"], ["-i"], ["-i", "a", "-o", "b", "--what"], ["a.json", "b.ply"]):
        assert colorize.parse_args(bad) is None
    assert colorize.main(["-i", "a.json"]) == 1
    a = globalcoord.parse_args(["p", "m", "s"])
    assert a.ply is False
    a = globalcoord.parse_args(["p", "m", "s", "--ply", "--ref-points"])
    assert a.ply is True and a.ref_points is True
    assert os.path.basename(hulo.COLORIZE_PROJECT_PATH) == hulo.COLORIZE_PROJECT == colorize.NAME
    assert capi.COLOR_CHUNK == 64 and "sfmloc_sfm_color_plan" in capi.SYMBOLS
