"""Writes tests/golden/imread_dev/: small JPEG files at the MCU and filter edges of the device image reader
(sfmloc_imread, sfmlocalization_amd/csrc/imread_dev.hip), and two query frames for the localisation tools.

    python tests/golden/make_imread_dev_fixtures.py

No expected arrays: the yardstick of tests/test_gpu_imread.py is the library's own host decoder (sfmloc_image_decode) on
the same bytes, which tests/test_image_io.py pins against libjpeg-turbo.  Needs Pillow (and torch on the CPU for the two
frames); the fixtures are committed so the tests do not.

  e420_<w>x<h>.jpg, e422_<w>x<h>.jpg   4:2:0 / 4:2:2 at widths 1 2 4 5 6 15 16 17 31 32 33 and heights 1 2 7 8 9 16 17
                                       (a subset of the grid: every width twice, every height, the corners): chroma
                                       width 2 -> 3 is where the triangle filter starts (its middle loop is empty at 3),
                                       odd heights clamp the h2v2 neighbour row, 15 / 16 / 17 and 31 / 32 / 33 straddle
                                       one and two MCUs
  prog_420_17x9.jpg, rst_420_17x9.jpg  progressive; a restart marker after every MCU
  rgb_444_23x19.jpg                    stored as R G B (component ids 82 71 66, no colour conversion)
  query_420.jpg, query_444.jpg         160 x 120 frames of the imageworld the tools' test builds its map from
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "imread_dev")

WIDTHS = [1, 2, 4, 5, 6, 15, 16, 17, 31, 32, 33]
HEIGHTS = [1, 2, 7, 8, 9, 16, 17]

# the world of the tools' test (tests/test_gpu_imread.py builds the map with the same numbers)
# (a texel per pixel at the cameras' height, and blobs fine enough that a 160 x 120 view has some 60 keypoints)
WORLD = dict(seed=5, tiles=1, tile_px=800, px_per_m=20.0, focal=200.0, width=160, height=120,
             atlas_kw=dict(smin=1.0, smax=3.0, blobs_per_tile=40000))


def picture(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([128 + 100 * np.sin(x / 3.0) * np.cos(y / 2.5), 128 + 90 * np.cos((x + y) / 2.0), 60 + 9.0 * y + 2.0 * x], -1)
    img += rng.normal(0, 12, img.shape)
    if h >= 4 and w >= 4:
        img[h // 3: h // 2 + 1, w // 4: w // 2 + 1] = (250, 10, 30)     # a saturated patch: exercises the range limits
    return np.clip(img, 0, 255).astype(np.uint8)


def grid():
    sizes = []
    for i, w in enumerate(WIDTHS):
        for h in (HEIGHTS[i % 7], HEIGHTS[(i + 3) % 7]):
            sizes.append((w, h))
    for wh in ((1, 1), (33, 17), (6, 17), (5, 1), (2, 9), (4, 9)):
        if wh not in sizes:
            sizes.append(wh)
    return sizes


def save(name, img, **opts):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **opts)
    with open(os.path.join(OUT, name), "wb") as f:
        f.write(b.getvalue())
    return len(b.getvalue())


def query_frames(W=None):
    sys.path.insert(0, ROOT)
    import torch

    import imageworld
    import synthdata as synth
    W = W or WORLD
    atlas = imageworld.make_atlas(W["seed"], W["tiles"], W["tile_px"], torch.device("cpu"), **W.get("atlas_kw", {}))
    rng = np.random.Generator(np.random.PCG64(W["seed"]))          # imageworld.build's first draws: the first view's pose
    tile_m = W["tile_px"] / W["px_per_m"]
    _, C0 = imageworld.cameras(rng, 1, (0.0, 0.0), tile_m)
    rq = np.random.Generator(np.random.PCG64(1005))
    Rs, Cs = [], []
    for _ in range(2):                                              # new poses within half a metre of that view
        R, C = synth.plane_camera(rq, (C0[0][0] + rq.uniform(-0.5, 0.5), C0[0][1] + rq.uniform(-0.5, 0.5)),
                                  rq.uniform(9.5, 10.5), tilt=0.05)
        Rs.append(R)
        Cs.append(C)
    return imageworld.render(atlas, W["px_per_m"], np.stack(Rs), np.stack(Cs), W["focal"], W["width"], W["height"])


def main():
    os.makedirs(OUT, exist_ok=True)
    total, n = 0, 0
    for k, (w, h) in enumerate(grid()):
        img = picture(h, w, 100 + k)
        total += save(f"e420_{w}x{h}.jpg", img, quality=90, subsampling=2)
        total += save(f"e422_{w}x{h}.jpg", img, quality=90, subsampling=1)
        n += 2
    img = picture(9, 17, 7)
    total += save("prog_420_17x9.jpg", img, quality=85, subsampling=2, progressive=True)
    total += save("rst_420_17x9.jpg", img, quality=85, subsampling=2, restart_marker_blocks=1)
    total += save("rgb_444_23x19.jpg", picture(19, 23, 8), quality=90, subsampling=0, keep_rgb=True)
    n += 3
    frames = query_frames()
    for name, g, sub in (("query_420.jpg", frames[0], 2), ("query_444.jpg", frames[1], 0)):
        total += save(name, np.stack([g, g, g], 2), quality=90, subsampling=sub)
        n += 1
    print("wrote", n, "files,", total, "bytes")


if __name__ == "__main__":
    main()
