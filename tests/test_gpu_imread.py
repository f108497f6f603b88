"""GPU: sfmloc_imread -- a JPEG entropy-decoded once on the host and reconstructed on the device (IDCT, fancy upsampling,
colour) -- against the library's own host decoder on the same bytes: every pixel of the three images a decode can leave
resident (GRAY = imread(IMREAD_GRAYSCALE), BGR = imread(IMREAD_COLOR), BGR2GRAY = cvtColor of the colour read) equals
sfmloc_image_decode's, which tests/test_image_io.py pins against libjpeg-turbo.  No Pillow here.
T1 goldens; T2 sizes at the MCU and filter edges; T3 arithmetic beyond 32 bits; T4 RGB files; T5 other formats;
T6 refusals; T7 reuse of one reader; T8 the extractors on the resident images; T9 the two localisation tools."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import imread_files as F
import sfmlocalization_amd as S
from sfmlocalization_amd import capi, engine
from test_gpu_imgbow import bits, model  # noqa: F401  (the small BoW / PCA model files)

pytestmark = pytest.mark.gpu

GRAY, BGR, BGR2GRAY = capi.IMREAD_GRAY, capi.IMREAD_BGR, capi.IMREAD_BGR2GRAY
ALL = GRAY | BGR | BGR2GRAY


def cv_gray(bgr):
    """cvtColor(BGR2GRAY) as LocalizeEngine.localize_image computes it"""
    b, g, r = (bgr[:, :, i].astype(np.int32) for i in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def host_images(data):
    bgr = S.image_decode(data, color=True)
    return {GRAY: S.image_decode(data, color=False), BGR: bgr, BGR2GRAY: cv_gray(bgr)}


def check_all(reader, data, what):
    """every combination of images a decode can be asked for gives the host decoder's bytes"""
    want = host_images(data)
    h, w = want[GRAY].shape
    for mask in (ALL, GRAY, BGR, BGR2GRAY, GRAY | BGR):
        assert reader.decode(data, mask) == (w, h), what
        for which in (GRAY, BGR, BGR2GRAY):
            if mask & which:
                np.testing.assert_array_equal(reader.read(which), want[which], err_msg=f"{what}: mask {mask}, image {which}")
            else:
                assert reader.dev(which) == 0


@pytest.fixture(scope="module")
def reader():
    r = capi.DeviceImread(64, 48)
    yield r
    r.close()


def test_t1_golden_jpegs(reader):
    names = F.golden_jpegs()
    assert len(names) >= 8 and "narrow_420.jpg" in names
    for name in names:
        check_all(reader, F.golden(name), name)


def test_t2_sizes_at_the_mcu_and_filter_edges(reader):
    names = F.edge_jpegs()
    assert len(names) >= 40
    assert {"prog_420_17x9.jpg", "rst_420_17x9.jpg"} <= set(names)
    sizes = set()
    for name in names:
        with open(os.path.join(F.EDGES, name), "rb") as f:
            data = f.read()
        check_all(reader, data, name)
        sizes.add((reader.width, reader.height))
    # chroma width 2 -> 3 (the triangle filter starts, its middle loop empty at 3), odd heights, one and two MCUs
    assert {w for w, _ in sizes} >= {1, 2, 4, 5, 6, 15, 16, 17, 31, 32, 33}
    assert {h for _, h in sizes} >= {1, 2, 7, 8, 9, 16, 17}


def test_t3_arithmetic_beyond_32_bits(reader):
    data = F.with_16bit_quant_of_65535(F.golden("base_420.jpg"))
    g = S.image_decode(data)
    assert g.shape == (37, 53) and g.min() == 0 and g.max() == 255
    check_all(reader, data, "base_420 with 16-bit quantisation tables of 65535")


def test_t4_rgb_files(reader):
    data = F.as_rgb_file(F.golden("base_420.jpg"))
    # (the host decoder skips the conversion: not the YCbCr file's colours)
    assert (S.image_decode(data, color=True) != S.image_decode(F.golden("base_420.jpg"), color=True)).any()
    check_all(reader, data, "base_420 as an R G B file")
    with open(os.path.join(F.EDGES, "rgb_444_23x19.jpg"), "rb") as f:
        data = f.read()
    sof = data.index(b"\xff\xc0")
    assert [data[sof + 10 + 3 * i] for i in range(3)] == [82, 71, 66]
    check_all(reader, data, "rgb_444_23x19.jpg")


def test_t5_other_formats(reader):
    rng = np.random.Generator(np.random.PCG64(3))
    files = {n: F.golden(n) for n in ("rgb.png", "rgba.png", "gray.png", "palette.png", "gray_alpha.png")}
    files["made.pgm"] = b"P5\n13 7\n255\n" + rng.integers(0, 256, 13 * 7, dtype=np.uint8).tobytes()
    files["made.ppm"] = b"P6\n# a comment\n9 11 255\n" + rng.integers(0, 256, 9 * 11 * 3, dtype=np.uint8).tobytes()
    for name, data in files.items():
        check_all(reader, data, name)


def test_t6_refusals(reader):
    good = F.golden("gray_base.jpg")
    want = host_images(good)
    assert reader.decode(good, ALL) == (17, 33)
    sof = F.golden("base_420.jpg").index(b"\xff\xc0")
    arithmetic = bytearray(F.golden("base_420.jpg"))
    arithmetic[sof + 1] = 0xC9
    for bad in (F.golden("base_420.jpg")[:sof + 7], bytes(arithmetic), b"not a picture at all, by any reading"):
        with pytest.raises(capi.SfmlocError) as host:
            S.image_decode(bad)
        assert host.value.message.startswith("sfmloc_image_decode: ")
        for mask in (GRAY, ALL):
            with pytest.raises(capi.SfmlocError) as dev:
                reader.decode(bad, mask)
            assert dev.value.code == host.value.code == capi.EIO
            assert dev.value.message == "sfmloc_imread_decode: " + host.value.message[len("sfmloc_image_decode: "):]
        # the previous decode's images still stand
        for which in (GRAY, BGR, BGR2GRAY):
            np.testing.assert_array_equal(reader.read(which), want[which])
    small = capi.DeviceImread(32, 40)
    try:
        for data in (F.golden("base_444_rst.jpg"), F.golden("rgb.png")):      # 64 x 48; 30 x 21 fits
            if data[:2] == b"\xff\xd8":
                with pytest.raises(capi.SfmlocError) as e:
                    small.decode(data, GRAY)
                assert e.value.code == capi.ECAP
            else:
                assert small.decode(data, GRAY) == (30, 21)
        with pytest.raises(capi.SfmlocError) as e:
            small.decode(F.golden("prog_420.jpg"), GRAY)                     # 35 x 45: too tall
        assert e.value.code == capi.ECAP
    finally:
        small.close()


def test_t7_one_reader_many_frames():
    r = capi.DeviceImread(64, 48)
    try:
        for name in ("base_444_rst.jpg", "gray_base.jpg", "narrow_420.jpg", "base_444_rst.jpg"):
            data = F.golden(name)
            want = host_images(data)
            r.decode(data, ALL)
            for which in (GRAY, BGR, BGR2GRAY):       # (nothing of an earlier, larger frame shows through)
                np.testing.assert_array_equal(r.read(which), want[which], err_msg=name)
    finally:
        r.close()


def test_t8_extractors_on_the_resident_images(model):
    bow_file, pca_file, _, _ = model
    with open(os.path.join(F.EDGES, "query_420.jpg"), "rb") as f:
        frame = f.read()
    # base_444_rst.jpg is 64 x 48, above AKAZE's 16 x 16 minimum, and too smooth for keypoints (the count that must be
    # equal is 0); the textured 160 x 120 frame is there so that keypoint records and descriptor rows are compared too
    for data, (w, h), textured in ((F.golden("base_444_rst.jpg"), (64, 48), False), (frame, (160, 120), True)):
        want = host_images(data)
        r = capi.DeviceImread(w, h)
        ak = capi.Akaze(w, h)
        ib = S.ImgBow.from_files(bow_file, pca_file, w, h, 3)
        try:
            for which in (GRAY, BGR2GRAY):
                kp_h, desc_h = ak.detect_and_compute(want[which])
                assert (len(kp_h) > 20) == textured
                r.decode(data, which | BGR)                 # (no host read between the decode and the extraction)
                kp_d, desc_d = ak.detect_and_compute_dev(r, which)
                assert len(kp_d) == len(kp_h)
                np.testing.assert_array_equal(kp_d.view(np.uint32), kp_h.view(np.uint32))
                np.testing.assert_array_equal(desc_d, desc_h)
                r.decode(data, which)
                assert ak.detect_resident_dev(r, which) == len(kp_h)
            bow_h = ib.compute(want[BGR])
            r.decode(data, GRAY | BGR)
            np.testing.assert_array_equal(bits(ib.compute_dev(r, BGR)), bits(bow_h))
            # what is not there, or not the extractor's size, is refused
            r.decode(data, GRAY)
            for call in (lambda: ak.detect_and_compute_dev(r, BGR2GRAY), lambda: ak.detect_and_compute_dev(r, BGR),
                         lambda: ib.compute_dev(r, BGR), lambda: ib.compute_dev(r, GRAY)):
                with pytest.raises(capi.SfmlocError) as e:
                    call()
                assert e.value.code == capi.EINVAL
            r.decode(F.golden("gray_base.jpg"), GRAY)
            with pytest.raises(capi.SfmlocError) as e:
                ak.detect_and_compute_dev(r, GRAY)
            assert e.value.code == capi.EINVAL and "17 x 33" in e.value.message
        finally:
            ib.close()
            ak.close()
            r.close()


CLI_BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfmlocalization_amd", "bin",
                       "OpenMVGLocalization_AKAZE")


def test_t9_the_tools_write_the_same_files_with_device_decode(model, tmp_path):
    import imageworld
    import synthdata as synth
    bow_file, pca_file, _, _ = model
    # the world of tests/golden/make_imread_dev_fixtures.py (WORLD), whose two query frames look at its first view
    dense = engine.DenseBow(bow_file, pca_file)
    iw = imageworld.build(S, 5, 6, 1, tiles=1, tile_px=800, px_per_m=20.0, focal=200.0, width=160, height=120,
                          dense_bow=dense, extract_batch=6, atlas_kw=dict(smin=1.0, smax=3.0, blobs_per_tile=40000))
    dense.close()
    synth.write_map_to_disk(iw.m, str(tmp_path / "sfm"), str(tmp_path / "matches"), with_bow=iw.bow)
    qdir = tmp_path / "queries"
    qdir.mkdir()
    for name in ("query_420.jpg", "query_444.jpg"):
        shutil.copy(os.path.join(F.EDGES, name), qdir / name)
    bow_args = ["-k=5", f"-a={bow_file}", f"-p={pca_file}"]
    localised = 0
    for tool in ("py", "cc"):
        for label, extra in (("plain", []), ("bow", bow_args)):
            outs = []
            for switch in ([], ["--device-decode"]):
                out = tmp_path / f"out_{tool}_{label}_{len(switch)}"
                args = [str(qdir), str(tmp_path / "sfm"), str(tmp_path / "matches"), str(out), "-r=25"] + extra + switch
                if tool == "py":
                    assert engine.main(args) == 0
                else:
                    res = subprocess.run([CLI_BIN] + args, capture_output=True, text=True, timeout=300)
                    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
                outs.append(out)
            names = sorted(os.listdir(outs[0]))
            assert names == sorted(os.listdir(outs[1])) == ["query_420.json", "query_444.json"]
            for n in names:
                a, b = (outs[0] / n).read_bytes(), (outs[1] / n).read_bytes()
                assert a == b, f"{tool} {label} {n}"
                localised += b'"t"' in a
    assert localised > 0        # (the comparison is not one of failure forms alone)
    # the engines' file entry points, Python and C++: device_decode gives the result of the host decode
    files = [str(qdir / n) for n in ("query_420.jpg", "query_444.jpg")]
    eng = engine.LocalizeEngine(str(tmp_path / "sfm"), str(tmp_path / "matches"), None, 0.6, 25, 4.0, False, 0, 0)
    try:
        for f in files:
            res_h, ex_h = eng.localize_file(f)
            res_d, ex_d = eng.localize_file(f, device_decode=True)
            assert len(res_h) == 12 and res_d == res_h and ex_d["pairs"] == ex_h["pairs"]
            assert ex_d["n_features"] == ex_h["n_features"] > 20
    finally:
        eng.close()
    driver = os.path.join(os.path.dirname(CLI_BIN), "engine_file_decode")
    res = subprocess.run([driver, str(tmp_path / "sfm"), str(tmp_path / "matches")] + files, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert [line.split()[:2] for line in res.stdout.splitlines()] == [["SAME", "12"], ["SAME", "12"]]
