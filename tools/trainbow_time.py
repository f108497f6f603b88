"""Stage timings of the vocabulary trainer (sfmloc_bowtrain_*, sfmlocalization_amd.trainbow) at the reference's sizes
(TrainBoW.cpp:46-54: 3 000 draws x 100 rows, PCA 61 -> 32, K = 100, 3 attempts, 100 iterations), next to the NumPy
restatement's Lloyd step on the host cores.

    python tools/trainbow_time.py [--images 200] [--views 200] [--out profiles/trainbow_time.json]

Images are synthetic textured VGA frames (synthdata.texture_image); the rows drawn from them are real dense descriptors.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synthdata as synth  # noqa: E402
import trainbow_np as tnp  # noqa: E402
from sfmlocalization_amd import capi, fileio, trainbow  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    imgs = []
    for k in range(a.images):
        g = synth.texture_image(5000 + k, 480, 640, n_blobs=400, n_rects=60)
        imgs.append(np.stack([g, g, g], 2))
    res = {"images": a.images, "rows": trainbow.PCA_TRAIN_FEATURE_NUM, "K": trainbow.K}
    with capi.BowTrainer(61, trainbow.PCA_TRAIN_FEATURE_NUM) as tr:
        rng = trainbow.CvRng()
        t0 = time.perf_counter()
        for _ in range(trainbow.PCA_TRAIN_FEATURE_NUM // trainbow.PCA_TRAIN_FEATURE_NUM_PER_IMAGE):
            k = trainbow.draw_index(len(imgs), rng.uniform01())
            rng.state = tr.add_image(imgs[k], trainbow.PCA_TRAIN_FEATURE_NUM_PER_IMAGE, rng.state)
        res["sampling_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        mean, evec, evals = tr.pca()
        res["pca_s"] = time.perf_counter() - t0
        x61 = tr.read()
        t0 = time.perf_counter()
        tr.project(mean, evec, evals, trainbow.PCA_DIM)
        res["project_s"] = time.perf_counter() - t0
        y = tr.read()
        for attempts, iters, key in ((1, 2, "kmeans_seed_plus_1_iter"), (1, 100, "kmeans_1_attempt"),
                                     (3, 100, "kmeans_3_attempts")):
            st = {}
            t0 = time.perf_counter()
            tr.kmeans(trainbow.K, attempts, iters, trainbow.FLT_EPSILON, trainbow.KMEANS_SEED, want_labels=False, stats=st)
            res[key + "_s"] = time.perf_counter() - t0
            res[key + "_assignments"] = st["iterations"]
        # (an attempt stops early once no centre moves by more than FLT_EPSILON: divide by the assignments it ran)
        extra = res["kmeans_1_attempt_assignments"] - res["kmeans_seed_plus_1_iter_assignments"]
        res["kmeans_per_iteration_ms"] = (1e3 * (res["kmeans_1_attempt_s"] - res["kmeans_seed_plus_1_iter_s"]) / extra
                                          if extra > 0 else None)
    # the host restatement: one assignment + centre update on the same projected rows
    cen = y[:trainbow.K].copy()
    t0 = time.perf_counter()
    lab = np.argmin(tnp.dist_f32(y, cen), 1)
    tnp.center_sums(y, lab, trainbow.K)
    res["numpy_lloyd_iteration_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    tnp.pca_moments(x61)
    res["numpy_pca_moments_s"] = time.perf_counter() - t0
    # the .bow pass
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        fileio.write_cv_yaml(os.path.join(td, "P.yml"), {"DimPCA": 32, "EigenVectorsPCA": evec, "EigenValuesPCA": evals,
                                                          "MeanPCA": mean})
        fileio.write_cv_yaml(os.path.join(td, "B.yml"), {"K": 100, "ResizedImageSize": 300, "NormBofFeatureType": "L1",
                                                          "UseSpatialPyramid": 1, "PyramidLevel": 2, "Centers": y[:100]})
        exs = [capi.ImgBow.from_files(os.path.join(td, "B.yml"), os.path.join(td, "P.yml"), 640, 480) for _ in range(8)]
        t0 = time.perf_counter()
        for v0 in range(0, a.views, 8):
            batch = [imgs[(v0 + i) % len(imgs)] for i in range(min(8, a.views - v0))]
            capi.ImgBow.compute_batch(exs[:len(batch)], batch)
            for e in exs[:len(batch)]:
                e.vector_read()
        res["bow_views_per_s"] = a.views / (time.perf_counter() - t0)
        for e in exs:
            e.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
