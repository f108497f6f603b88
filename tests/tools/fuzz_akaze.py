#!/usr/bin/env python3
"""Randomised AKAZE + M-LDB parity campaign: random textures at random sizes from 16 x 16 up (odd widths, tile edges of
the fused kernels, frames below one segment), random thresholds and octave / sub-level counts within the limits of
sfmloc_akaze_create, GPU against the CPU restatement -- scale space, determinant response, keypoints and descriptors bit
for bit.  usage: fuzz_akaze.py [n_images] [first_seed]
SFMLOC_FUZZ_BATCH=1: every seed is a BATCH of 2..6 textures of one random size taken by
sfmloc_akaze_detect_and_compute_batch (one launch per kernel for the batch), each frame against the oracle."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402
from oracle import oracle_c  # noqa: E402


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def draw(rng, seed, n_images=1):
    """-> (w, h, n_octaves, n_sublevels, threshold, [images]): a request sfmloc_akaze_create accepts.  (The FED cycle of a
    level stays within 64 steps: octave 5 would need a frame of 2560 x 1280.)"""
    h = int(rng.integers(16, 420))
    w = int(rng.integers(16, 560))
    omax = int(rng.integers(1, 9))
    nsub = int(rng.integers(1, 32 // omax + 1))
    thres = float(10.0 ** rng.uniform(-5.0, -2.0))
    imgs = []
    for j in range(n_images):
        if min(h, w) < 40:  # (texture_image places rectangles of up to 40 pixels) two-level random blocks
            block = int(rng.integers(2, 7))
            small = rng.integers(0, 2, ((h + block - 1) // block, (w + block - 1) // block))
            g = (30 + 195 * np.kron(small, np.ones((block, block), np.int64))[:h, :w]).astype(np.uint8)
        else:
            g = synth.texture_image(seed * 8 + j, h, w, n_blobs=int(rng.integers(20, 400)), n_rects=int(rng.integers(5, 80)))
        if rng.uniform() < 0.3:
            g = np.clip(g.astype(np.int32) + rng.integers(-12, 13, g.shape), 0, 255).astype(np.uint8)
        imgs.append(g)
    return w, h, omax, nsub, thres, imgs


def one(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    w, h, omax, nsub, thres, (g,) = draw(rng, seed)
    ekp, edesc, eldet, elt = oracle_c.akaze_detect_and_compute(g, thres, omax, nsub, cap=65536, want_levels=True)
    ak = S.Akaze(w, h, n_octaves=omax, n_sublevels=nsub, threshold=thres)
    try:
        assert [tuple(x) for x in oracle_c.akaze_levels(w, h, omax, nsub)] == ak.levels, "level sizes"
        kp, desc = ak.detect_and_compute(g)
        ldet, lt = ak.read_levels()
        assert np.array_equal(bits32(lt), bits32(elt)), "scale space"
        assert np.array_equal(bits32(ldet), bits32(eldet)), "determinant response"
        assert len(kp) == len(ekp) and np.array_equal(bits32(kp), bits32(ekp)), "keypoints"
        assert np.array_equal(desc[:, :61], edesc), "descriptors"
    finally:
        ak.close()
    return len(kp)


def one_batch(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    k = int(rng.integers(2, 7))
    w, h, omax, nsub, thres, imgs = draw(rng, seed, k)
    exs = [S.Akaze(w, h, n_octaves=omax, n_sublevels=nsub, threshold=thres) for _ in range(k)]
    try:
        got = S.Akaze.detect_and_compute_batch(exs, imgs)
        total = 0
        for j, (g, e, (kp, desc)) in enumerate(zip(imgs, exs, got)):
            ekp, edesc, eldet, elt = oracle_c.akaze_detect_and_compute(g, thres, omax, nsub, cap=65536, want_levels=True)
            ldet, lt = e.read_levels()
            assert np.array_equal(bits32(lt), bits32(elt)), f"scale space (frame {j} of {k})"
            assert np.array_equal(bits32(ldet), bits32(eldet)), f"determinant response (frame {j} of {k})"
            assert len(kp) == len(ekp) and np.array_equal(bits32(kp), bits32(ekp)), f"keypoints (frame {j} of {k})"
            assert np.array_equal(desc[:, :61], edesc), f"descriptors (frame {j} of {k})"
            total += len(kp)
    finally:
        for e in exs:
            e.close()
    return total


def main():
    global one
    if os.environ.get("SFMLOC_FUZZ_BATCH") == "1":
        one = one_batch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    oracle_c.build()
    t0 = time.time()
    total = 0
    for s in range(first, first + n):
        try:
            total += one(s)
        except AssertionError as e:
            w, h, omax, nsub, thres, _ = draw(np.random.Generator(np.random.PCG64(s)), s)
            print(f"seed {s} ({w} x {h}, nOct {omax}, nOctLay {nsub}, thres {thres:.3g}): PARITY FAILURE: {e}", flush=True)
            raise
        if (s - first) % 10 == 9:
            print(f"{s - first + 1} images, {total} keypoints compared, {time.time() - t0:.0f} s", flush=True)
    print(f"OK: {n} images, {total} keypoints, every stage bit-exact ({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
