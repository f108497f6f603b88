"""TrainBoW (TrainBoW/src/TrainBoW.cpp) over the C ABI:

    python -m sfmlocalization_amd.trainbow <inputDir> <bowFile> [-p=pcaFile] [--device=0]

Finds every matches/sfm_data.json below inputDir (readSfmDataFiles, :60-93), draws the training rows of the map images'
dense descriptors (getRandomTrainFeatures, :95-131), trains PCA (with -p) and the k-means vocabulary
(BoFSpatialPyramids::trainKMeans), writes BOWfile.yml / PCAfile.yml as cv::FileStorage does, and one <view>.bow per map
view next to its sfm_data.json (saveMatBin).  Sampling, PCA moments, projection, k-means and the .bow vectors run on the
GPU (sfmloc_bowtrain_*, sfmloc_imgbow_*).

Differences from the reference, all without effect on the output:
  - the reference shares one cv::RNG across an OpenMP loop (racy draws); the draws here are those of a single-threaded
    run of it;
  - with -p the reference draws the k-means sample with a fresh cv::RNG, i.e. the same rows as the PCA sample: the
    sample is kept on the device and projected instead of being drawn again;
  - directories are listed in sorted order (the reference takes readdir's order).
"""
import os
import sys

import numpy as np

from . import capi, engine, fileio

PCA_TRAIN_FEATURE_NUM = 300000          # TrainBoW.cpp:46-54
PCA_TRAIN_FEATURE_NUM_PER_IMAGE = 100
KMEANS_TRAIN_FEATURE_NUM = 300000
KMEANS_TRAIN_FEATURE_NUM_PER_IMAGE = 100
K = 100
PCA_DIM = 32
NORM_BOF_FEATURE_TYPE = "L1"            # L1_NORM_SQUARE_ROOT
USE_SPATIAL_PYRAMID = True
PYRAMID_LEVEL = 2
RESIZED_IMAGE_SIZE = 300                # BowDenseFeatureSettings.h
KMEANS_ITERATION = 100                  # BoFSpatialPyramids.cpp:29
KMEANS_ATTEMPTS = 3
FLT_EPSILON = float(np.finfo(np.float32).eps)
KMEANS_SEED = 0xFFFFFFFF                # cv::theRNG() of a fresh process
BATCH = 8                               # views per sfmloc_imgbow_compute_batch

KEYS = [(("p", "pcaFile"), "", str), (("device",), "0", int), (("h", "help"), "false", engine._b)]


class CvRng:
    """cv::RNG (multiply-with-carry; include/sfmloc.h states it)"""

    def __init__(self, state=0xFFFFFFFF):
        self.state = int(state) or 0xFFFFFFFF

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform01(self):
        return np.float32(np.float32(self.next()) * np.float32(2.3283064365386962890625e-10))


def draw_index(n, r):
    """images.size() * randImage / descriptors.rows * randFeature: a float32 product, truncated, clamped below n"""
    return min(int(np.float32(np.float32(n) * np.float32(r))), n - 1)


def read_sfm_data_files(d, out=None):
    """readSfmDataFiles (TrainBoW.cpp:60-93): matches/sfm_data.json files below d"""
    out = [] if out is None else out
    if not os.path.isdir(d):
        return out
    last = os.path.basename(os.path.normpath(d))
    names = sorted(os.listdir(d))
    if last == "matches":
        out += [os.path.join(d, f) for f in names if f == "sfm_data.json" and os.path.isfile(os.path.join(d, f))]
    else:
        for f in names:
            if os.path.isdir(os.path.join(d, f)):
                read_sfm_data_files(os.path.join(d, f), out)
    return out


def sfm_images(sfm_data_file):
    """-> [(image path, .bow path)] in view-id order (TrainBoW.cpp:164-166, 246-253)"""
    sd = fileio.read_sfm_data(sfm_data_file)
    root = sd.get("root_path", "")
    out = []
    for v in sorted(sd["views"], key=lambda v: int(v["key"])):
        fn = os.path.basename(v["value"]["ptr_wrapper"]["data"]["filename"])
        out.append((os.path.join(root, fn), os.path.join(os.path.dirname(sfm_data_file), os.path.splitext(fn)[0] + ".bow")))
    return out


def _read_bgr(path):
    try:
        return capi.image_read(path, color=True)
    except (capi.SfmlocError, OSError):
        return None          # imread failed: the image has no descriptors


def random_train_features(trainer, images, feature_num, per_image, log=None):
    """getRandomTrainFeatures (TrainBoW.cpp:95-131) into the trainer's sample; an image drawn again is decoded again,
    except right after itself"""
    rng = CvRng()
    trainer.reset()
    last_k, img = -1, None
    for i in range(feature_num // per_image):
        k = draw_index(len(images), rng.uniform01())
        if k != last_k:            # (only the last decoded image is kept: a map's images need not fit host memory)
            img, last_k = _read_bgr(images[k]), k
        if log:
            log(f"extract feature from {images[k]}")
        rng.state = trainer.add_image(img, per_image, rng.state)
    return trainer.size()


def write_bow_vectors(bow_file, pca_file, views, device=0, log=None):
    """calcDenseLocalFeature -> calcPcaProject -> calcBoF -> saveMatBin for every view (TrainBoW.cpp:238-272),
    sfmloc_imgbow batches of one image size"""
    pools = {}
    pending = {}

    def flush(key):
        items = pending.pop(key, [])
        if not items:
            return
        exs = pools[key]
        if pca_file:
            capi.ImgBow.compute_batch(exs[:len(items)], [img for img, _ in items])
            vecs = [e.vector_read() for e in exs[:len(items)]]
        else:   # (61-dimensional words do not fit the batched assignment's LDS layout: one chain per image)
            vecs = [exs[0].compute(img) for img, _ in items]
        for v, (_, out) in zip(vecs, items):
            fileio.write_mat_bin(out, v.reshape(-1, 1))
            if log:
                log(f"Saved BoW feature : {out}")

    try:
        for img_path, out in views:
            img = _read_bgr(img_path)
            if img is None:
                raise IOError(f"cannot read {img_path}")
            key = img.shape[:2]
            if key not in pools:
                pools[key] = [capi.ImgBow.from_files(bow_file, pca_file or None, key[1], key[0], 3, device=device)
                              for _ in range(BATCH)]
            pending.setdefault(key, []).append((img, out))
            if len(pending[key]) == BATCH:
                flush(key)
        for key in list(pending):
            flush(key)
    finally:
        for exs in pools.values():
            for e in exs:
                e.close()


def train(input_dir, bow_file, pca_file="", device=0, log=print):
    sfm_files = read_sfm_data_files(input_dir)
    log(f"number of sfm data files found : {len(sfm_files)}")
    views = [v for f in sfm_files for v in sfm_images(f)]
    images = [p for p, _ in views]
    log(f"number of image files found : {len(images)}")
    if not images:
        raise IOError(f"no map images below {input_dir}")
    with capi.BowTrainer(61, max(PCA_TRAIN_FEATURE_NUM, KMEANS_TRAIN_FEATURE_NUM), device=device) as tr:
        if pca_file:
            n, d = random_train_features(tr, images, PCA_TRAIN_FEATURE_NUM, PCA_TRAIN_FEATURE_NUM_PER_IMAGE)
            log(f"End getting features to train PCA. Training feature matrix size is ({n} x {d})")
            mean, evec, evals = tr.pca()
            fileio.write_cv_yaml(pca_file, {"DimPCA": PCA_DIM, "EigenVectorsPCA": evec, "EigenValuesPCA": evals,
                                            "MeanPCA": mean})
            p = fileio.read_cv_yaml(pca_file)    # the reference reloads the model from the file (TrainBoW.cpp:196-203)
            tr.project(p["MeanPCA"], p["EigenVectorsPCA"], p["EigenValuesPCA"], int(p["DimPCA"]))
        else:
            n, d = random_train_features(tr, images, KMEANS_TRAIN_FEATURE_NUM, KMEANS_TRAIN_FEATURE_NUM_PER_IMAGE)
            log(f"End getting features to train k-means. Training feature matrix size is ({n} x {d})")
        centers, _, compactness = tr.kmeans(K, KMEANS_ATTEMPTS, KMEANS_ITERATION, FLT_EPSILON, KMEANS_SEED,
                                            want_labels=False)
        log(f"End train kmeans. Number of cluster is {K} (compactness {compactness:.6g})")
    fileio.write_cv_yaml(bow_file, {"K": K, "ResizedImageSize": RESIZED_IMAGE_SIZE,
                                    "NormBofFeatureType": NORM_BOF_FEATURE_TYPE, "UseSpatialPyramid": int(USE_SPATIAL_PYRAMID),
                                    "PyramidLevel": PYRAMID_LEVEL, "Centers": centers})
    write_bow_vectors(bow_file, pca_file, views, device=device)
    log("End calculate BoF feature for all images.")
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    pos, o = engine.parse_cv_args(argv, KEYS)
    if len(pos) < 2 or o["help"] or not pos[0] or not pos[1]:
        print("usage: python -m sfmlocalization_amd.trainbow <inputDir> <bowFile> [-p=pcaFile] [--device=0]")
        return 1
    return train(pos[0], pos[1], o["pcaFile"], o["device"])


if __name__ == "__main__":
    sys.exit(main())
