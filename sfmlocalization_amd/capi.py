"""ctypes mirror of include/sfmloc.h (one Python method per C entry point, same names and meaning)."""
import ctypes as C
import os
import weakref

import numpy as np

from . import _abi, _lib

NOMATCH, COLOR_CHUNK = _abi.constants("NOMATCH", "COLOR_CHUNK")
K_HAMMING, K_COMPACT, K_FMATRIX, K_MATCHSET, K_P3P, K_BOW, K_COUNT = _abi.constants(
    "K_HAMMING", "K_COMPACT", "K_FMATRIX", "K_MATCHSET", "K_P3P", "K_BOW", "K_COUNT")
OK, EINVAL, ENODEV, EHIP, EIO, ECAP, ENOMEM = _abi.constants("OK", "EINVAL", "ENODEV", "EHIP", "EIO", "ECAP", "ENOMEM")
BA_ROTATION, BA_TRANSLATION, BA_INTRINSICS, BA_STRUCTURE = _abi.constants(
    "BA_ROTATION", "BA_TRANSLATION", "BA_INTRINSICS", "BA_STRUCTURE")
TRI_ROBUST, TRI_BLIND = _abi.constants("TRI_ROBUST", "TRI_BLIND")
MERGE_SIMILARITY, MERGE_AFFINE = _abi.constants("MERGE_SIMILARITY", "MERGE_AFFINE")
MERGE_MODELS = {"similarity": MERGE_SIMILARITY, "affine": MERGE_AFFINE}


class SfmlocError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sfmloc error {code}: {msg}")
        self.code = code
        self.message = msg  # the library's text alone (sfmloc_last_error)


# the structs of include/sfmloc.h, fields by the header's names
Params = _abi.struct("sfmloc_params")
MapDesc = _abi.struct("sfmloc_map_desc")
MapInfo = _abi.struct("sfmloc_map_info")
Pose = _abi.struct("sfmloc_pose")
BofDesc = _abi.struct("sfmloc_bof_desc")
ScanInfo = _abi.struct("sfmloc_scan_info")
SfmDesc = _abi.struct("sfmloc_sfm_desc")
SfmViewResult = _abi.struct("sfmloc_sfm_view_result")
BaReport = _abi.struct("sfmloc_ba_report")
BaJointOptions = _abi.struct("sfmloc_ba_joint_options")
BaJointReport = _abi.struct("sfmloc_ba_joint_report")
TriangulateOptions = _abi.struct("sfmloc_triangulate_options")
TriangulateReport = _abi.struct("sfmloc_triangulate_report")
RegisterOptions = _abi.struct("sfmloc_register_options")
RegisterReport = _abi.struct("sfmloc_register_report")
RelposeOptions = _abi.struct("sfmloc_relpose_options")
RelposeResult = _abi.struct("sfmloc_relpose_result")
RelrefineOptions = _abi.struct("sfmloc_relrefine_options")
RelrefineResult = _abi.struct("sfmloc_relrefine_result")
WscalesOptions = _abi.struct("sfmloc_wscales_options")
Wscale = _abi.struct("sfmloc_wscale")
WscalesReport = _abi.struct("sfmloc_wscales_report")
SeedOptions = _abi.struct("sfmloc_seed_options")
SeedScore = _abi.struct("sfmloc_seed_score")
GpscaleOptions = _abi.struct("sfmloc_gpscale_options")
GpscaleReport = _abi.struct("sfmloc_gpscale_report")
GposesOptions = _abi.struct("sfmloc_gposes_options")
GposesPair = _abi.struct("sfmloc_gposes_pair")
GposesReport = _abi.struct("sfmloc_gposes_report")
MergeParams = _abi.struct("sfmloc_merge_params")
MergeResult = _abi.struct("sfmloc_merge_result")
ReduceResult = _abi.struct("sfmloc_reduce_result")
BowknnOptions = _abi.struct("sfmloc_bowknn_options")
KernelStats = _abi.struct("sfmloc_kernel_stats")

# every entry point include/sfmloc.h declares (tests check the library exports each one)
SYMBOLS = list(_abi.PROTOTYPES)

_bound = False

GANG_MAX = 32


class gang:
    """`with gang(ctxs):` -- sfmloc_gang_begin / _end: the asynchronous calls made on these contexts (<= GANG_MAX, one
    map) inside the block record their launches, and leaving it issues them as ONE launch per kernel for all members."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        self._arr = (C.c_void_p * len(self.ctxs))(*[c._h for c in self.ctxs])

    def __enter__(self):
        _check(_L().sfmloc_gang_begin(self._arr, len(self.ctxs)))
        return self

    def __exit__(self, *exc):
        _check(_L().sfmloc_gang_end(self._arr, len(self.ctxs)))
        return False


def result_fingerprint(pose, pair_qfeat, pair_landmark, view_counts=True):
    """Every bit of a query's result -- ok, status, counts, iterations, NFA, error_max, P, K, R, t, centre and the
    inlier pairs (localization.cpp:504-547: what the result file is written from) -- except the stage timings, as 8
    bytes.  Two runs of a query agree bit for bit iff their fingerprints do (bench.py `identical_to_single_flight`,
    tests/test_gpu_load.py).  view_counts=False leaves out n_putative_views / n_geometric_views, which a shard of a
    sharded map counts for its own views only."""
    import hashlib
    h = hashlib.blake2b(digest_size=8)
    raw = C.string_at(C.addressof(pose), Pose.stage_seconds.offset)
    if not view_counts:
        o = Pose.n_putative_views.offset
        raw = raw[:o] + raw[o + 8:]
    h.update(raw)
    h.update(np.ascontiguousarray(pair_qfeat).tobytes())
    h.update(np.ascontiguousarray(pair_landmark).tobytes())
    return h.digest()


def _handles(objs):
    return (C.c_void_p * len(objs))(*[o._h for o in objs])


def shard_batch_bow_keys(ctxs, gang, queries, knn, keys_dev_ptr):
    """sfmloc_shard_batch_bow_keys: every query's knn best views of this shard -> keys [len(queries)][knn] on the device"""
    _check(_L().sfmloc_shard_batch_bow_keys(_handles(ctxs), len(ctxs), gang, _handles(queries), len(queries), knn,
                                            C.c_void_p(keys_dev_ptr)))


def shard_batch_begin_bow(ctxs, gang, queries, keys_all_dev_ptr, n_parts, knn, packed_dev_ptr, budget):
    """sfmloc_shard_batch_begin_bow: stage 1 of a batch on the global shortlist + the packed export, one call"""
    _check(_L().sfmloc_shard_batch_begin_bow(_handles(ctxs), len(ctxs), gang, _handles(queries), len(queries),
                                             C.c_void_p(keys_all_dev_ptr), n_parts, knn, C.c_void_p(packed_dev_ptr), budget))


def shard_batch_begin(ctxs, gang, queries, packed_dev_ptr, budget):
    _check(_L().sfmloc_shard_batch_begin(_handles(ctxs), len(ctxs), gang, _handles(queries), len(queries),
                                         C.c_void_p(packed_dev_ptr), budget))


def merge_batch_begin(ctxs, queries, query_index, packed_all_dev_ptr, n_parts, part_stride, n_queries, budget):
    """sfmloc_merge_batch_begin: stage 2 of len(ctxs) queries in one session (finish each with Context.end)"""
    qi = np.ascontiguousarray(query_index, np.uint32)
    _check(_L().sfmloc_merge_batch_begin(_handles(ctxs), len(ctxs), _handles(queries), _ptr(qi, C.c_uint32),
                                         C.c_void_p(packed_all_dev_ptr), n_parts, part_stride, n_queries, budget))


def feat_round_trip(kpt_xy):
    """sfmloc_feat_round_trip: the keypoints after the reference's `.feat` text round trip (6 significant digits)."""
    k = np.ascontiguousarray(kpt_xy, dtype=np.float32)
    out = np.empty_like(k)
    _L().sfmloc_feat_round_trip(_ptr(k, C.c_float), k.size, _ptr(out, C.c_float))
    return out


def gang_counters(lead_ctx):
    """(launches issued by this leader's sessions, of which gang launches with more than one member)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(_L().sfmloc_gang_counters(lead_ctx._h, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def _L():
    global _bound
    L = _lib.load()
    if not _bound:
        for name, (restype, argtypes) in _abi.PROTOTYPES.items():   # the header's signatures, every one of them
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _bound = True
    return L


def _check(rc):
    if rc != 0:
        raise SfmlocError(rc, _L().sfmloc_last_error().decode("utf-8", "replace"))


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _sel(view_sel):
    """view selection -> (pointer, count, keep-alive).  An EMPTY selection must stay a non-null pointer with count 0
    (NULL means "all views" in the C ABI), so it is backed by a one-element dummy."""
    sel = np.ascontiguousarray(view_sel, dtype=np.uint32).ravel()
    back = sel if sel.shape[0] else np.zeros(1, np.uint32)
    return _ptr(back, C.c_uint32), int(sel.shape[0]), back


def device_count():
    return int(_L().sfmloc_device_count())


def packed_bytes(n_queries, budget):
    return int(_L().sfmloc_packed_bytes(n_queries, budget))


def part_bytes(cap):
    return int(_L().sfmloc_part_bytes(cap))


def scan(sfm_dir, match_dir):
    """sfmloc_scan: parse <sfm_dir>/sfm_data.json + <match_dir>/*.desc|feat|bow on the host, no GPU."""
    info = ScanInfo()
    _check(_L().sfmloc_scan(os.fsencode(sfm_dir), os.fsencode(match_dir), C.byref(info)))
    return {f: getattr(info, f) for f, _ in ScanInfo._fields_}


def pack(sfm_dir, match_dir, out_path):
    """sfmloc_pack: the map's files -> one packed binary (host only)."""
    _check(_L().sfmloc_pack(os.fsencode(sfm_dir), os.fsencode(match_dir), os.fsencode(out_path)))


def scan_packed(path):
    """sfmloc_scan_packed: the fields of scan() from a packed map file, no GPU."""
    info = ScanInfo()
    _check(_L().sfmloc_scan_packed(os.fsencode(path), C.byref(info)))
    return {f: getattr(info, f) for f, _ in ScanInfo._fields_}


def default_params(**overrides):
    p = Params()
    _L().sfmloc_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def dense_gray(bgr, size=300, device=0):
    """sfmloc_dense_gray: BGR u8 [h, w, 3] -> the size x size gray image the dense AKAZE describes
    (DenseLocalFeatureWrapper.cpp:89-99)."""
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w, c = bgr.shape
    if c != 3:
        raise ValueError("dense_gray: expected an h x w x 3 BGR image")
    out = np.zeros((size, size), np.uint8)
    _check(_L().sfmloc_dense_gray(device, _ptr(bgr, C.c_uint8), w, h, size, _ptr(out, C.c_uint8)))
    return out


def image_decode(data, color=False):
    """sfmloc_image_decode: the bytes of a JPEG / PNG / PGM / PPM file -> what cv::imread returns for it: u8 [h, w]
    (IMREAD_GRAYSCALE, AKAZEOpenCV.cpp:60) or u8 [h, w, 3] in B G R order (IMREAD_COLOR,
    DenseLocalFeatureWrapper.cpp:85).  Host code; raises SfmlocError (SFMLOC_EIO) for an undecodable file."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    w, h = C.c_int32(0), C.c_int32(0)
    L = _L()
    _check(L.sfmloc_image_decode(_ptr(raw, C.c_uint8), raw.size, int(bool(color)), None, 0, C.byref(w), C.byref(h)))
    out = np.zeros((h.value, w.value, 3) if color else (h.value, w.value), np.uint8)
    _check(L.sfmloc_image_decode(_ptr(raw, C.c_uint8), raw.size, int(bool(color)), _ptr(out, C.c_uint8), out.size,
                                 C.byref(w), C.byref(h)))
    return out


def image_size(path):
    """(width, height) of an image file from its header (sfmloc_image_read with a NULL buffer)."""
    w, h = C.c_int32(0), C.c_int32(0)
    L = _L()
    _check(L.sfmloc_image_read(os.fsencode(path), 0, None, 0, C.byref(w), C.byref(h)))
    return w.value, h.value


def image_read(path, color=False):
    """sfmloc_image_read: cv::imread(path, IMREAD_GRAYSCALE | IMREAD_COLOR) as the reference's tools call it."""
    w, h = C.c_int32(0), C.c_int32(0)
    L = _L()
    bpath = os.fsencode(path)
    _check(L.sfmloc_image_read(bpath, int(bool(color)), None, 0, C.byref(w), C.byref(h)))
    out = np.zeros((h.value, w.value, 3) if color else (h.value, w.value), np.uint8)
    _check(L.sfmloc_image_read(bpath, int(bool(color)), _ptr(out, C.c_uint8), out.size, C.byref(w), C.byref(h)))
    return out


IMREAD_GRAY, IMREAD_BGR, IMREAD_BGR2GRAY = _abi.constants("IMREAD_GRAY", "IMREAD_BGR", "IMREAD_BGR2GRAY")


class DeviceImread:
    """sfmloc_imread: cv::imread whose pixels are born on the device.  A JPEG is entropy-decoded once on the host and
    reconstructed by two kernels; the images asked for (a mask of IMREAD_GRAY, IMREAD_BGR, IMREAD_BGR2GRAY) stay resident
    for Akaze.detect_and_compute_dev / detect_resident_dev and ImgBow.compute_dev.  Every pixel equals image_decode's."""

    def __init__(self, max_width, max_height, device=0):
        self._h = None
        h = C.c_void_p()
        _check(_L().sfmloc_imread_create(device, int(max_width), int(max_height), C.byref(h)))
        self._h = h
        self.max_width, self.max_height = int(max_width), int(max_height)
        self.width = self.height = 0

    def decode(self, data, want=IMREAD_GRAY):
        """the bytes of a JPEG / PNG / PGM / PPM file -> (width, height); asynchronous on the reader's stream"""
        raw = np.frombuffer(bytes(data), dtype=np.uint8)
        w, h = C.c_int32(0), C.c_int32(0)
        _check(_L().sfmloc_imread_decode(self._h, _ptr(raw, C.c_uint8), raw.size, int(want), C.byref(w), C.byref(h)))
        self.width, self.height = w.value, h.value
        return w.value, h.value

    def file(self, path, want=IMREAD_GRAY):
        w, h = C.c_int32(0), C.c_int32(0)
        _check(_L().sfmloc_imread_file(self._h, os.fsencode(path), int(want), C.byref(w), C.byref(h)))
        self.width, self.height = w.value, h.value
        return w.value, h.value

    def read(self, which):
        """one image of the last decode as u8 [h, w] (or [h, w, 3] for IMREAD_BGR); waits for it"""
        out = np.zeros((self.height, self.width, 3) if which == IMREAD_BGR else (self.height, self.width), np.uint8)
        _check(_L().sfmloc_imread_read(self._h, int(which), _ptr(out, C.c_uint8), out.size))
        return out

    def dev(self, which):
        """device address of one image of the last decode (0 when it did not leave that image)"""
        return int(_L().sfmloc_imread_dev(self._h, int(which)) or 0)

    def share_stream(self, ctx):
        _check(_L().sfmloc_imread_share_stream(self._h, None if ctx is None else ctx._h))

    def timing(self, enable=True, read=False):
        """sfmloc_imread_timing: switch event timing of JPEG decodes; read=True -> (host ms, upload ms, IDCT ms,
        upsampling + colour ms) of the last timed decode"""
        out = np.zeros(4, np.float64) if read else None
        _check(_L().sfmloc_imread_timing(self._h, int(bool(enable)), _ptr(out, C.c_double)))
        return None if out is None else tuple(float(v) for v in out)

    def close(self):
        if self._h is not None:
            _L().sfmloc_imread_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Undistorter:
    """sfmloc_undistorter: the server's per-user undistortion (localizeImage.cc:149-177).  new_camera (3x3) and roi
    (x, y, w, h) are what getOptimalNewCameraMatrix(K, dist, size, 1.0, size, &validRoi) returns; apply() is
    cv::undistort + the crop to validRoi, on the GPU."""

    def __init__(self, K, dist, width, height, device=0):
        L = _L()
        Kc = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        d = np.ascontiguousarray(dist, dtype=np.float64).ravel()
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        _check(L.sfmloc_undistorter_create(device, _ptr(Kc, C.c_double), _ptr(d, C.c_double) if d.size else None,
                                           d.size, self.width, self.height, C.byref(self._h)))
        P = np.zeros(9, np.float64)
        roi = np.zeros(4, np.int32)
        _check(L.sfmloc_undistorter_info(self._h, _ptr(P, C.c_double), _ptr(roi, C.c_int32)))
        self.new_camera = P.reshape(3, 3)
        self.roi = tuple(int(v) for v in roi)

    def maps(self):
        xy = np.zeros((self.height, self.width, 2), np.int16)
        fr = np.zeros((self.height, self.width), np.uint16)
        _check(_L().sfmloc_undistorter_maps(self._h, _ptr(xy, C.c_int16), _ptr(fr, C.c_uint16)))
        return xy, fr

    def apply(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        ch = 1 if img.ndim == 2 else img.shape[2]
        if img.shape[0] != self.height or img.shape[1] != self.width:
            raise ValueError("Undistorter.apply: image size differs from the plan's")
        out = np.zeros((self.roi[3], self.roi[2]) if img.ndim == 2 else (self.roi[3], self.roi[2], ch), np.uint8)
        _check(_L().sfmloc_undistorter_apply(self._h, _ptr(img, C.c_uint8), ch, _ptr(out, C.c_uint8), out.size))
        return out

    def close(self):
        if self._h:
            _L().sfmloc_undistorter_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def debug_fail_p3p_alloc(k):
    """sfmloc_debug_fail_p3p_alloc: allocation k of the next P3P workspace regrowth fails (one shot; -1 disarms)."""
    _L().sfmloc_debug_fail_p3p_alloc(int(k))


def debug_fail_next_alloc(k):
    """sfmloc_debug_fail_next_alloc: this thread's k-th device allocation from now fails once (-1 disarms)."""
    _L().sfmloc_debug_fail_next_alloc(int(k))


def k3_list_counts(reset=False, device=0):
    """sfmloc_debug_k3_list_counts: (inlier lists K3's register forms copied from the evaluating wave's segment, lists a
    wave evaluated the model again for) on `device` since the last reset; reset=True clears both after reading."""
    out = np.zeros(2, np.uint64)
    _check(_L().sfmloc_debug_k3_list_counts(int(device), _ptr(out, C.c_uint64), int(bool(reset))))
    return int(out[0]), int(out[1])


def k5_round_counts(reset=False, device=0):
    """sfmloc_debug_k5_round_counts: the P3P rounds queued in the (small, plain, wide) launch form by every context of
    the process since the last reset; reset=True clears the three after reading."""
    out = np.zeros(3, np.uint64)
    _check(_L().sfmloc_debug_k5_round_counts(int(device), _ptr(out, C.c_uint64), int(bool(reset))))
    return int(out[0]), int(out[1]), int(out[2])


def debug_math(op, x, out_stride, device=0):
    """sfmloc_debug_math: run an f64 device building block over the rows of x."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    out = np.zeros((x.shape[0], out_stride), np.float64)
    _check(_L().sfmloc_debug_math(device, op, _ptr(x, C.c_double), x.shape[0], x.shape[1], _ptr(out, C.c_double),
                                  out_stride))
    return out


class Map:
    """Owns a sfmloc_map handle: the reconstruction's descriptor bank (and, later, its keypoints,
    landmarks and BoW vectors) resident in HBM -- what localization.cpp:238-280 loads once."""

    def __init__(self, view_id, view_off, desc, params=None, view_wh=None, kpt_xy=None, row_landmark=None,
                 landmark_id=None, landmark_X=None, intrinsic=None, bow=None):
        self._h = None
        self._children = weakref.WeakSet()
        self.view_id = np.ascontiguousarray(view_id, dtype=np.uint32)
        self.view_off = np.ascontiguousarray(view_off, dtype=np.uint32)
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 64)
        self.n_rows = desc.shape[0]
        self.n_views = self.view_id.shape[0]
        keep = [self.view_id, self.view_off, desc]
        d = MapDesc()
        d.n_views = self.n_views
        d.view_id = _ptr(self.view_id, C.c_uint32)
        d.view_off = _ptr(self.view_off, C.c_uint32)
        d.n_rows = self.n_rows
        d.desc = _ptr(desc, C.c_uint8)
        if view_wh is not None:
            view_wh = np.ascontiguousarray(view_wh, dtype=np.uint32).reshape(-1, 2)
            keep.append(view_wh)
            d.view_wh = _ptr(view_wh, C.c_uint32)
        if kpt_xy is not None:
            kpt_xy = np.ascontiguousarray(kpt_xy, dtype=np.float32).reshape(-1, 2)
            keep.append(kpt_xy)
            d.kpt_xy = _ptr(kpt_xy, C.c_float)
        if row_landmark is not None:
            row_landmark = np.ascontiguousarray(row_landmark, dtype=np.int32)
            landmark_id = np.ascontiguousarray(landmark_id, dtype=np.uint32)
            landmark_X = np.ascontiguousarray(landmark_X, dtype=np.float64).reshape(-1, 3)
            keep += [row_landmark, landmark_id, landmark_X]
            d.row_landmark = _ptr(row_landmark, C.c_int32)
            d.n_landmarks = landmark_id.shape[0]
            d.landmark_id = _ptr(landmark_id, C.c_uint32)
            d.landmark_X = _ptr(landmark_X, C.c_double)
        if intrinsic is not None:
            d.focal, d.ppx, d.ppy = intrinsic[:3]
            if len(intrinsic) >= 6:           # (f, ppx, ppy, k1, k2, k3) = pinhole_radial_k3
                d.k1, d.k2, d.k3 = intrinsic[3:6]
                d.intrinsic_type = 3
        if bow is not None:
            bow = np.ascontiguousarray(bow, dtype=np.float32).reshape(self.n_views, -1)
            keep.append(bow)
            d.bow_dim = bow.shape[1]
            d.bow = _ptr(bow, C.c_float)
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        _check(_L().sfmloc_map_create(C.byref(d), C.byref(self.params), C.byref(h)))
        self._h = h
        del keep

    @classmethod
    def open(cls, sfm_dir, match_dir, params=None):
        """sfmloc_open: load the reference's on-disk map (sfm_data.json + .desc/.feat[/.bow])."""
        self = cls.__new__(cls)
        self._h = None
        self._children = weakref.WeakSet()
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        _check(_L().sfmloc_open(os.fsencode(sfm_dir), os.fsencode(match_dir), C.byref(self.params), C.byref(h)))
        self._h = h
        i = self.info()
        self.n_rows, self.n_views = i["n_rows"], i["n_views"]
        self.view_id = np.zeros(self.n_views, np.uint32)
        self.view_off = np.zeros(self.n_views + 1, np.uint32)
        self.view_center = np.zeros((self.n_views, 3), np.float64)
        _check(_L().sfmloc_map_views(self._h, _ptr(self.view_id, C.c_uint32), _ptr(self.view_off, C.c_uint32),
                                     _ptr(self.view_center, C.c_double)))
        return self

    @classmethod
    def open_packed(cls, path, params=None):
        """sfmloc_open_packed: the map written by pack(); equal to open() on the files it was packed from."""
        self = cls.__new__(cls)
        self._h = None
        self._children = weakref.WeakSet()
        self.params = params if params is not None else default_params()
        h = C.c_void_p()
        _check(_L().sfmloc_open_packed(os.fsencode(path), C.byref(self.params), C.byref(h)))
        self._h = h
        i = self.info()
        self.n_rows, self.n_views = i["n_rows"], i["n_views"]
        self.view_id = np.zeros(self.n_views, np.uint32)
        self.view_off = np.zeros(self.n_views + 1, np.uint32)
        self.view_center = np.zeros((self.n_views, 3), np.float64)
        _check(_L().sfmloc_map_views(self._h, _ptr(self.view_id, C.c_uint32), _ptr(self.view_off, C.c_uint32),
                                     _ptr(self.view_center, C.c_double)))
        return self

    def close(self):
        if self._h is not None:
            # queries and contexts hold pointers into the map: release them first, whatever order the
            # garbage collector would have chosen
            for ch in list(self._children):
                try:
                    ch.close()
                except Exception:
                    pass
            _L().sfmloc_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        i = MapInfo()
        _check(_L().sfmloc_map_get_info(self._h, C.byref(i)))
        return {"n_rows": i.n_rows, "n_views": i.n_views, "n_landmarks": i.n_landmarks,
                "hbm_bytes": i.hbm_bytes, "device": i.device}

    def query(self, desc, kpt_xy=None, width=0, height=0):
        return Query(self, desc, kpt_xy, width, height)

    def match_putative(self, q, view_sel=None):
        """sfmloc_match_putative: asynchronous; results stay on the device."""
        if view_sel is None:
            _check(_L().sfmloc_match_putative(self._h, q._h, None, 0))
        else:
            p, n, keep = _sel(view_sel)
            _check(_L().sfmloc_match_putative(self._h, q._h, p, n))

    def putative_read(self):
        """-> view_count[V], match_i, match_j, match_d (each [n_rows]; view v's list at view_off[v])."""
        cnt = np.zeros(self.n_views, np.uint32)
        mi = np.full(self.n_rows, NOMATCH, np.uint32)
        mj = np.full(self.n_rows, NOMATCH, np.uint32)
        md = np.full(self.n_rows, NOMATCH, np.uint32)
        _check(_L().sfmloc_putative_read(self._h, _ptr(cnt, C.c_uint32), _ptr(mi, C.c_uint32),
                                         _ptr(mj, C.c_uint32), _ptr(md, C.c_uint32), self.n_rows))
        return cnt, mi, mj, md

    def putative_read_rows(self):
        b0 = np.empty(self.n_rows, np.uint32)
        b1 = np.empty(self.n_rows, np.uint32)
        _check(_L().sfmloc_putative_read_rows(self._h, _ptr(b0, C.c_uint32), _ptr(b1, C.c_uint32)))
        return b0, b1

    def sync(self):
        _check(_L().sfmloc_sync(self._h))

    # ----- map-side matching (matchAKAZE / trackAKAZE, MatchUtils.cpp:73-277) -----
    def query_view(self, desc_ptr, kpt_ptr, kpt6_ptr, bow_ptr, n, width, height):
        """sfmloc_query_create_view: a query over device arrays that stay the caller's (integers = device pointers)."""
        return Query._over_device_arrays(self, desc_ptr, kpt_ptr, kpt6_ptr, bow_ptr, n, width, height)

    def query_from_view(self, view_index):
        """sfmloc_query_from_view: one map image's descriptors as a Query (rebuilt from the bank on the device)."""
        return Query._from_view(self, int(view_index))

    def match_one_to_one(self, q, view_sel=None):
        """sfmloc_match_one_to_one: putative matching + matchAKAZE's one-to-one filter; read with putative_read()."""
        if view_sel is None:
            _check(_L().sfmloc_match_one_to_one(self._h, q._h, None, 0))
        else:
            p, n, keep = _sel(view_sel)
            _check(_L().sfmloc_match_one_to_one(self._h, q._h, p, n))

    @staticmethod
    def _take_matches(h):
        out = {}
        try:
            for k in range(_L().sfmloc_matches_pairs(h)):
                vi, vj, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
                _check(_L().sfmloc_matches_pair(h, k, C.byref(vi), C.byref(vj), C.byref(n)))
                mi = np.zeros(n.value, np.uint32)
                mj = np.zeros(n.value, np.uint32)
                _check(_L().sfmloc_matches_read(h, k, _ptr(mi, C.c_uint32), _ptr(mj, C.c_uint32), n.value))
                out[(vi.value, vj.value)] = (mi, mj)
        finally:
            _L().sfmloc_matches_destroy(h)
        return out

    def match_pairs(self, pairs):
        """sfmloc_match_pairs (hulo::matchAKAZE): pairs = [(first, second) view indices] ->
        {(first, second): (i[], j[])} in std::map order."""
        arr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        _check(_L().sfmloc_match_pairs(self._h, _ptr(arr, C.c_uint32), arr.shape[0], C.byref(h)))
        return self._take_matches(h)

    def track(self, max_frame_dist):
        """sfmloc_track (hulo::trackAKAZE) over the views in table order."""
        h = C.c_void_p()
        _check(_L().sfmloc_track(self._h, int(max_frame_dist), C.byref(h)))
        return self._take_matches(h)

    def geometric_pairs(self, matches):
        """sfmloc_geometric_pairs (hulo::geometricMatch): {(I, J): (i[], j[])} -> the same for the pairs that pass the
        F-matrix AC-RANSAC, matches in its inlier order."""
        keys = sorted(matches)
        pairs = np.array(keys, np.uint32).reshape(-1, 2)
        off = np.zeros(len(keys) + 1, np.uint64)
        off[1:] = np.cumsum([len(matches[k][0]) for k in keys])
        mi = np.concatenate([np.asarray(matches[k][0], np.uint32) for k in keys]) if keys else np.zeros(0, np.uint32)
        mj = np.concatenate([np.asarray(matches[k][1], np.uint32) for k in keys]) if keys else np.zeros(0, np.uint32)
        mi, mj = np.ascontiguousarray(mi, np.uint32), np.ascontiguousarray(mj, np.uint32)
        h = C.c_void_p()
        _check(_L().sfmloc_geometric_pairs(self._h, _ptr(pairs, C.c_uint32), len(keys), _ptr(off, C.c_uint64),
                                           _ptr(mi, C.c_uint32), _ptr(mj, C.c_uint32), C.byref(h)))
        return self._take_matches(h)

    def geometric_filter(self, q):
        _check(_L().sfmloc_geometric_filter(self._h, q._h))

    def geometric_read(self):
        """-> geo_count[V], geo_idx[n_rows] (indices into each view's putative list, AC-RANSAC inlier order)."""
        cnt = np.zeros(self.n_views, np.uint32)
        idx = np.full(self.n_rows, NOMATCH, np.uint32)
        _check(_L().sfmloc_geometric_read(self._h, _ptr(cnt, C.c_uint32), _ptr(idx, C.c_uint32), self.n_rows))
        return cnt, idx

    def geometric_read_pairs(self):
        """-> geo_count[V], geo_i[n_rows], geo_j[n_rows]: each view's geometric matches as (map feature, query feature),
        view v's list at view_off[v] -- the guided matches with params.guided_matching, else the putative matches the
        inlier indices name."""
        cnt = np.zeros(self.n_views, np.uint32)
        gi = np.full(self.n_rows, NOMATCH, np.uint32)
        gj = np.full(self.n_rows, NOMATCH, np.uint32)
        _check(_L().sfmloc_geometric_read_pairs(self._h, _ptr(cnt, C.c_uint32), _ptr(gi, C.c_uint32),
                                                _ptr(gj, C.c_uint32), self.n_rows))
        return cnt, gi, gj

    def match_set(self, q):
        _check(_L().sfmloc_match_set(self._h, q._h))

    def match_set_read(self, cap=65536):
        n = C.c_uint32()
        qf = np.zeros(cap, np.uint32)
        lm = np.zeros(cap, np.uint32)
        p2 = np.zeros((cap, 2), np.float64)
        p3 = np.zeros((cap, 3), np.float64)
        _check(_L().sfmloc_match_set_read(self._h, C.byref(n), _ptr(qf, C.c_uint32), _ptr(lm, C.c_uint32),
                                          _ptr(p2, C.c_double), _ptr(p3, C.c_double), cap))
        k = n.value
        return qf[:k].copy(), lm[:k].copy(), p2[:k].copy(), p3[:k].copy()

    def resection(self, q):
        _check(_L().sfmloc_resection(self._h, q._h))

    def debug_resect6(self, pt2d, pt3d, width, height):
        """sfmloc_debug_resect6: the uncalibrated query's resection stage on given 2D-3D correspondences;
        -> (Pose, inlier indices in AC-RANSAC's order)."""
        p2 = np.ascontiguousarray(pt2d, dtype=np.float64).reshape(-1, 2)
        p3 = np.ascontiguousarray(pt3d, dtype=np.float64).reshape(-1, 3)
        assert p2.shape[0] == p3.shape[0]
        pose = Pose()
        ii = np.zeros(max(p2.shape[0], 1), np.uint32)
        _check(_L().sfmloc_debug_resect6(self._h, _ptr(p2, C.c_double), _ptr(p3, C.c_double), p2.shape[0], int(width),
                                         int(height), C.byref(pose), _ptr(ii, C.c_uint32), ii.size))
        k = pose.n_inliers if pose.ok else 0
        return pose, ii[:k].copy()

    def pose_read(self, cap=65536):
        pose = Pose()
        pq = np.zeros(cap, np.uint32)
        pl = np.zeros(cap, np.uint32)
        ii = np.zeros(cap, np.uint32)
        _check(_L().sfmloc_pose_read(self._h, C.byref(pose), _ptr(pq, C.c_uint32), _ptr(pl, C.c_uint32),
                                     _ptr(ii, C.c_uint32), cap))
        k = pose.n_inliers if pose.ok else 0
        return pose, pq[:k].copy(), pl[:k].copy(), ii[:k].copy()

    def localize(self, q, view_sel=None, cap=65536):
        """sfmloc_localize: the whole per-query path; -> (Pose, pair_qfeat, pair_landmark)."""
        pose = Pose()
        pq = np.zeros(cap, np.uint32)
        pl = np.zeros(cap, np.uint32)
        if view_sel is None:
            sel_p, n_sel = None, 0
        else:
            sel_p, n_sel, keep = _sel(view_sel)
        _check(_L().sfmloc_localize(self._h, q._h, sel_p, n_sel, C.byref(pose), _ptr(pq, C.c_uint32),
                                    _ptr(pl, C.c_uint32), cap))
        k = pose.n_inliers if pose.ok else 0
        return pose, pq[:k].copy(), pl[:k].copy()

    def view_sizes(self):
        """sfmloc_map_view_sizes: (width, height) of every view, [n_views, 2]."""
        wh = np.zeros((self.n_views, 2), np.uint32)
        _check(_L().sfmloc_map_view_sizes(self._h, _ptr(wh, C.c_uint32)))
        return wh

    def localize_bow(self, q, query_bow, knn, cand_views=None, cap=65536):
        """sfmloc_localize_bow: BoW shortlist (when more than knn candidates remain) + the whole path in one call on
        the map's own context; -> (Pose, pair_qfeat, pair_landmark)."""
        pose = Pose()
        pq = np.zeros(cap, np.uint32)
        pl = np.zeros(cap, np.uint32)
        b = np.ascontiguousarray(query_bow, dtype=np.float32).ravel()
        if cand_views is None:
            sel_p, n_sel = None, 0
        else:
            sel_p, n_sel, keep = _sel(cand_views)
        _check(_L().sfmloc_localize_bow(self._h, q._h, _ptr(b, C.c_float), int(knn), sel_p, n_sel, C.byref(pose),
                                        _ptr(pq, C.c_uint32), _ptr(pl, C.c_uint32), cap))
        k = pose.n_inliers if pose.ok else 0
        return pose, pq[:k].copy(), pl[:k].copy()

    def context(self, share=None, merge_only=False):
        return Context(self, share, merge_only)

    def bow_select(self, query_bow, k, cand_views=None):
        """sfmloc_bow_select (selectViewByBoF): -> ascending view-table indices of the k nearest .bow vectors."""
        qb = np.ascontiguousarray(query_bow, dtype=np.float32).ravel()
        out = np.zeros(max(k, 1), np.uint32)
        n = C.c_uint32()
        if cand_views is None:
            cp, nc = None, 0
        else:
            cv = np.ascontiguousarray(cand_views, dtype=np.uint32)
            cp, nc = _ptr(cv, C.c_uint32), cv.shape[0]
        _check(_L().sfmloc_bow_select(self._h, _ptr(qb, C.c_float), cp, nc, k, _ptr(out, C.c_uint32), C.byref(n)))
        return out[:n.value].copy()

    def bow_distances(self, query_bow):
        """sfmloc_bow_distances: float32 L2 distance of every view's .bow vector to the query's (what bow_select ranks)."""
        qb = np.ascontiguousarray(query_bow, dtype=np.float32).ravel()
        out = np.zeros(self.n_views, np.float32)
        _check(_L().sfmloc_bow_distances(self._h, _ptr(qb, C.c_float), _ptr(out, C.c_float)))
        return out

    def localize_batch(self, queries, n_contexts=4, cap=0):
        """sfmloc_localize_batch: queries pipelined over n_contexts streams; -> list of Pose (+ pairs if cap)."""
        n = len(queries)
        arr = (C.c_void_p * n)(*[q._h for q in queries])
        poses = (Pose * n)()
        pq = np.zeros((n, cap), np.uint32) if cap else None
        pl = np.zeros((n, cap), np.uint32) if cap else None
        _check(_L().sfmloc_localize_batch(self._h, arr, n, n_contexts, poses, _ptr(pq, C.c_uint32),
                                          _ptr(pl, C.c_uint32), cap))
        if cap:
            return list(poses), pq, pl
        return list(poses)

    def stats(self):
        s = KernelStats()
        _check(_L().sfmloc_stats_read(self._h, C.byref(s)))
        return s

    def stats_reset(self):
        _check(_L().sfmloc_stats_reset(self._h))

    def set_profile(self, level):
        """sfmloc_set_profile: 0 off, 1 every stage, 2 the Hamming scan only."""
        _check(_L().sfmloc_set_profile(self._h, int(level)))


NORM_TYPES = {"NONE": 0, "L2": 1, "L1": 2}


def _bof_desc(centers, in_dim, resized=300, use_pyramid=True, pyramid_level=2, norm="L1", pca_mean=None,
              pca_eigvec=None, pca_eigval=None, n_pca=0):
    """-> (BofDesc, the arrays it points into)"""
    centers = np.ascontiguousarray(centers, np.float32)
    d = BofDesc()
    d.K, d.in_dim = centers.shape[0], int(in_dim)
    d.centers = _ptr(centers, C.c_float)
    d.resized_image_size, d.use_spatial_pyramid, d.pyramid_level = int(resized), int(bool(use_pyramid)), int(pyramid_level)
    d.norm_type = NORM_TYPES[norm] if isinstance(norm, str) else int(norm)
    keep = [centers]
    if n_pca:
        pm = np.ascontiguousarray(pca_mean, np.float32).ravel()
        pe = np.ascontiguousarray(np.asarray(pca_eigvec, np.float32)[:n_pca])
        pv = np.ascontiguousarray(np.asarray(pca_eigval, np.float32).ravel()[:n_pca])
        keep += [pm, pe, pv]
        d.n_pca, d.pca_mean, d.pca_eigvec, d.pca_eigval = int(n_pca), _ptr(pm, C.c_float), _ptr(pe, C.c_float), _ptr(pv, C.c_float)
    return d, keep


def _bof_desc_from_files(bow_file, pca_file=None, in_dim=61):
    from . import fileio
    b = fileio.read_cv_yaml(bow_file)
    kw = {}
    if pca_file:
        p = fileio.read_cv_yaml(pca_file)
        kw = dict(pca_mean=p["MeanPCA"], pca_eigvec=p["EigenVectorsPCA"], pca_eigval=p["EigenValuesPCA"],
                  n_pca=int(p["DimPCA"]))
    return dict(centers=b["Centers"], in_dim=in_dim, resized=int(b["ResizedImageSize"]),
                use_pyramid=bool(b["UseSpatialPyramid"]), pyramid_level=int(b["PyramidLevel"]),
                norm=b["NormBofFeatureType"], **kw)


class ImgBow:
    """sfmloc_imgbow: the query-side BoW vector from the image as one resident, asynchronous chain
    (DenseLocalFeatureWrapper::calcDenseLocalFeature -> PcaWrapper::calcPcaProject -> BoFSpatialPyramids::calcBoF)."""

    def __init__(self, width, height, channels=3, device=0, **model):
        self._h = None
        d, keep = _bof_desc(**model)
        h = C.c_void_p()
        _check(_L().sfmloc_imgbow_create(C.byref(d), device, int(width), int(height), int(channels), C.byref(h)))
        self._h = h
        self.width, self.height, self.channels = int(width), int(height), int(channels)
        self.dim = int(_L().sfmloc_imgbow_dim(h))

    @classmethod
    def from_files(cls, bow_file, pca_file, width, height, channels=3, device=0):
        return cls(width, height, channels, device, **_bof_desc_from_files(bow_file, pca_file))

    def share_stream(self, ctx):
        _check(_L().sfmloc_imgbow_share_stream(self._h, None if ctx is None else ctx._h))

    def order_before(self, ctx):
        """the context's stream waits for what this extractor has queued (an extractor on a stream of its own)"""
        _check(_L().sfmloc_imgbow_order_before(self._h, ctx._h))

    def vector_dev(self):
        """device address of the float32 vector a compute() without a query writes (a query view's bow_dev)"""
        return int(_L().sfmloc_imgbow_vector_dev(self._h) or 0)

    def compute(self, image, query=None, want_vector=None):
        """image [h, w, channels] (or [h, w] for channels = 1) u8.  query: its resident BoW slot is filled
        (asynchronously: share the stream with the context that localises it).  want_vector (default: when no query is
        given): also return the float64 vector, which synchronises."""
        img = np.ascontiguousarray(image, np.uint8)
        assert img.size == self.width * self.height * self.channels, img.shape
        want = (query is None) if want_vector is None else want_vector
        out = np.zeros(self.dim, np.float64) if want else None
        _check(_L().sfmloc_imgbow_compute(self._h, _ptr(img, C.c_uint8), None if query is None else query._h,
                                          _ptr(out, C.c_double)))
        return out

    def compute_dev(self, reader, which=IMREAD_BGR, query=None, want_vector=None):
        """sfmloc_imgbow_compute_dev: compute() on a DeviceImread's resident image (nothing crosses PCIe)"""
        want = (query is None) if want_vector is None else want_vector
        out = np.zeros(self.dim, np.float64) if want else None
        _check(_L().sfmloc_imgbow_compute_dev(self._h, reader._h, int(which), None if query is None else query._h,
                                              _ptr(out, C.c_double)))
        return out

    def vector_read(self):
        """the float64 vector of the last compute() / compute_batch() this extractor took part in (synchronises)"""
        out = np.zeros(self.dim, np.float64)
        _check(_L().sfmloc_imgbow_vector_read(self._h, _ptr(out, C.c_double)))
        return out

    @staticmethod
    def compute_batch(extractors, images):
        """sfmloc_imgbow_compute_batch: the vectors of len(images) frames (one extractor each, same image size) in one gang
        session on the first extractor's stream -- one launch per kernel for all of them.  The float32 vectors stay on the
        device (vector_dev of each extractor); asynchronous."""
        n = len(images)
        assert 1 <= n <= len(extractors) and n <= GANG_MAX
        imgs = [np.ascontiguousarray(g, np.uint8) for g in images]
        for e, g in zip(extractors, imgs):
            assert g.size == e.width * e.height * e.channels, g.shape
        hs = (C.c_void_p * n)(*[e._h for e in extractors[:n]])
        ps = (C.POINTER(C.c_uint8) * n)(*[_ptr(g, C.c_uint8) for g in imgs])
        _check(_L().sfmloc_imgbow_compute_batch(hs, ps, n))

    def close(self):
        if self._h is not None:
            _L().sfmloc_imgbow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BofModel:
    """sfmloc_bof: BOWfile.yml (+ PCAfile.yml) on the GPU; compute() = calcPcaProject + calcBoF."""

    def __init__(self, centers, in_dim, resized=300, use_pyramid=True, pyramid_level=2, norm="L1", pca_mean=None,
                 pca_eigvec=None, pca_eigval=None, n_pca=0, device=0):
        self._h = None
        d, keep = _bof_desc(centers, in_dim, resized, use_pyramid, pyramid_level, norm, pca_mean, pca_eigvec, pca_eigval, n_pca)
        centers = keep[0]
        h = C.c_void_p()
        _check(_L().sfmloc_bof_create(C.byref(d), device, C.byref(h)))
        self._h = h
        self.dim = int(_L().sfmloc_bof_dim(h))
        self.resized = int(resized)
        self.K = int(centers.shape[0])

    @classmethod
    def from_files(cls, bow_file, pca_file=None, in_dim=61, device=0):
        return cls(device=device, **_bof_desc_from_files(bow_file, pca_file, in_dim))

    def compute(self, desc, kpt_xy):
        desc = np.ascontiguousarray(desc, np.float32)
        kpt_xy = np.ascontiguousarray(kpt_xy, np.float32).reshape(-1, 2)
        out = np.zeros(self.dim, np.float64)
        _check(_L().sfmloc_bof_compute(self._h, _ptr(desc, C.c_float), _ptr(kpt_xy, C.c_float), desc.shape[0],
                                       _ptr(out, C.c_double)))
        return out

    def close(self):
        if self._h is not None:
            _L().sfmloc_bof_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sfm_default_params(**overrides):
    """sfmloc_sfm_default_params: the re-resection's gates (min_resection_points 10, min_inliers 7, 4 096 iterations)"""
    p = Params()
    _L().sfmloc_sfm_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


# COLOR_CHUNK (SFMLOC_COLOR_CHUNK, above): iterations of the colouring plan enqueued per host read
COLOR_UNSET = 0xFFFFFFFF        # lm_iter of a landmark without observations


def sfm_color_last_ms():
    """device milliseconds of this thread's last Sfm.color_plan"""
    return float(_L().sfmloc_sfm_color_last_ms())


def ba_joint_default_options():
    """sfmloc_ba_joint_default_options -> BaJointOptions"""
    o = BaJointOptions()
    _L().sfmloc_ba_joint_default_options(C.byref(o))
    return o


def sfm_json_rewrite(in_path, out_path):
    """sfmloc_sfm_json_rewrite (host only): the C++ JSON writer of OpenMVG_BA on a parsed file"""
    _check(_L().sfmloc_sfm_json_rewrite(os.fsencode(in_path), os.fsencode(out_path)))


class Sfm:
    """sfmloc_sfm: OpenMVG_BA's re-resection and structure cleanup on a device-resident sfm_data (include/sfmloc.h states
    the semantics).  Arrays as sfmloc_sfm_desc: views ascending, a pose table (ascending pose id), landmarks ascending
    with their observations in CSR (obs_off, obs_view = view index, obs_x)."""

    def __init__(self, view_id, view_intrinsic, view_pose, intrinsic_type, intrinsic, pose_valid, pose_R, pose_C,
                 landmark_id, landmark_X, obs_off, obs_view, obs_x, params=None):
        self._h = None
        a = self._keep = dict(
            view_id=np.ascontiguousarray(view_id, np.uint32), view_intrinsic=np.ascontiguousarray(view_intrinsic, np.uint32),
            view_pose=np.ascontiguousarray(view_pose, np.uint32), intrinsic_type=np.ascontiguousarray(intrinsic_type, np.uint32),
            intrinsic=np.ascontiguousarray(intrinsic, np.float64).reshape(-1, 6),
            pose_valid=np.ascontiguousarray(pose_valid, np.uint8), pose_R=np.ascontiguousarray(pose_R, np.float64).reshape(-1, 9),
            pose_C=np.ascontiguousarray(pose_C, np.float64).reshape(-1, 3),
            landmark_id=np.ascontiguousarray(landmark_id, np.uint32),
            landmark_X=np.ascontiguousarray(landmark_X, np.float64).reshape(-1, 3),
            obs_off=np.ascontiguousarray(obs_off, np.uint64), obs_view=np.ascontiguousarray(obs_view, np.uint32),
            obs_x=np.ascontiguousarray(obs_x, np.float64).reshape(-1, 2))
        d = SfmDesc()
        d.n_views, d.n_intrinsics = len(a["view_id"]), len(a["intrinsic_type"])
        d.n_poses, d.n_landmarks = len(a["pose_valid"]), len(a["landmark_id"])
        for f, t in (("view_id", C.c_uint32), ("view_intrinsic", C.c_uint32), ("view_pose", C.c_uint32),
                     ("intrinsic_type", C.c_uint32), ("intrinsic", C.c_double), ("pose_valid", C.c_uint8),
                     ("pose_R", C.c_double), ("pose_C", C.c_double), ("landmark_id", C.c_uint32),
                     ("landmark_X", C.c_double), ("obs_off", C.c_uint64), ("obs_view", C.c_uint32), ("obs_x", C.c_double)):
            setattr(d, f, _ptr(a[f].reshape(-1) if a[f].size else np.zeros(1, a[f].dtype), t))
        self.n_views, self.n_poses, self.n_landmarks = d.n_views, d.n_poses, d.n_landmarks
        self.n_obs = int(a["obs_off"][-1])
        h = C.c_void_p()
        _check(_L().sfmloc_sfm_create(C.byref(d), C.byref(params if params is not None else sfm_default_params()),
                                      C.byref(h)))
        self._h = h

    def resect(self):
        """-> (views resected, views whose pose was replaced)"""
        ran, ok = C.c_uint32(0), C.c_uint32(0)
        _check(_L().sfmloc_sfm_resect(self._h, C.byref(ran), C.byref(ok)))
        return int(ran.value), int(ok.value)

    def resect_read(self):
        """-> list of SfmViewResult, one per view"""
        out = (SfmViewResult * self.n_views)()
        _check(_L().sfmloc_sfm_resect_read(self._h, out))
        return list(out)

    def resect_inliers(self, k):
        n = C.c_uint32(0)
        _check(_L().sfmloc_sfm_resect_inliers(self._h, int(k), None, 0, C.byref(n)))
        idx = np.zeros(max(1, n.value), np.uint32)
        _check(_L().sfmloc_sfm_resect_inliers(self._h, int(k), _ptr(idx, C.c_uint32), idx.size, C.byref(n)))
        return idx[:n.value].copy()

    def clean(self, residual_px=4.0, angle_deg=2.0, rm_unstable=False):
        """-> the four landmark counts: before, after the residual filter, after the angle filter, after cleanup"""
        counts = (C.c_uint64 * 4)()
        _check(_L().sfmloc_sfm_clean(self._h, float(residual_px), float(angle_deg), 1 if rm_unstable else 0, counts))
        return [int(c) for c in counts]

    def read(self, masks=True):
        """-> dict(pose_valid, pose_R [n,3,3], pose_C [n,3], obs_keep, landmark_keep) (masks after clean())"""
        pv = np.zeros(max(1, self.n_poses), np.uint8)
        R = np.zeros((max(1, self.n_poses), 9))
        Cc = np.zeros((max(1, self.n_poses), 3))
        ok_ = np.zeros(max(1, self.n_obs), np.uint8) if masks else None
        lk = np.zeros(max(1, self.n_landmarks), np.uint8) if masks else None
        _check(_L().sfmloc_sfm_read(self._h, _ptr(pv, C.c_uint8), _ptr(R, C.c_double), _ptr(Cc, C.c_double),
                                    _ptr(ok_, C.c_uint8), _ptr(lk, C.c_uint8)))
        out = {"pose_valid": pv[:self.n_poses].astype(bool), "pose_R": R[:self.n_poses].reshape(-1, 3, 3),
               "pose_C": Cc[:self.n_poses]}
        if masks:
            out["obs_keep"] = ok_[:self.n_obs].astype(bool)
            out["landmark_keep"] = lk[:self.n_landmarks].astype(bool)
        return out

    def adjust(self, what):
        """sfmloc_sfm_adjust: the separable bundle adjustment -- what = BA_STRUCTURE, BA_ROTATION, BA_TRANSLATION or
        BA_ROTATION | BA_TRANSLATION (0: nothing) -> BaReport"""
        rep = BaReport()
        _check(_L().sfmloc_sfm_adjust(self._h, int(what), C.byref(rep)))
        return rep

    def adjust_joint(self, what, **options):
        """sfmloc_sfm_adjust_joint: poses, intrinsics and structure in one Levenberg-Marquardt problem -- what = any
        non-zero combination of the BA_ bits; options = fields of BaJointOptions over the defaults -> BaJointReport"""
        opt = ba_joint_default_options()
        for k, val in options.items():
            if k not in ("max_steps", "max_pcg", "function_tolerance", "pcg_tolerance"):
                raise TypeError(f"adjust_joint: unknown option {k}")
            setattr(opt, k, val)
        rep = BaJointReport()
        _check(_L().sfmloc_sfm_adjust_joint(self._h, int(what), C.byref(opt), C.byref(rep)))
        return rep

    def triangulate(self, **options):
        """sfmloc_sfm_triangulate: X and the keep masks rebuilt from the poses -- options = fields of TriangulateOptions
        over the defaults (mode TRI_ROBUST / TRI_BLIND, min_inliers, allow_pairs, residual_px) -> TriangulateReport"""
        opt = triangulate_default_options()
        for k, val in options.items():
            if k not in ("mode", "min_inliers", "allow_pairs", "residual_px"):
                raise TypeError(f"triangulate: unknown option {k}")
            setattr(opt, k, val)
        rep = TriangulateReport()
        _check(_L().sfmloc_sfm_triangulate(self._h, C.byref(opt), C.byref(rep)))
        return rep

    def register(self, **options):
        """sfmloc_sfm_register: the views without a pose resected against the kept structure, the structure extended,
        round after round -- options = fields of RegisterOptions over the defaults (max_rounds, min_points, min_inliers,
        tri_min_inliers, tri_allow_pairs, residual_px) -> RegisterReport"""
        opt = register_default_options()
        for k, val in options.items():
            if k not in ("max_rounds", "min_points", "min_inliers", "tri_min_inliers", "tri_allow_pairs", "residual_px"):
                raise TypeError(f"register: unknown option {k}")
            setattr(opt, k, val)
        rep = RegisterReport()
        _check(_L().sfmloc_sfm_register(self._h, C.byref(opt), C.byref(rep)))
        return rep

    def register_read(self):
        """-> (list of SfmViewResult, one per view: the last round that tried it; round [n_views], -1 = never tried)"""
        out = (SfmViewResult * self.n_views)()
        rnd = np.full(max(1, self.n_views), -1, np.int32)
        _check(_L().sfmloc_sfm_register_read(self._h, out, _ptr(rnd, C.c_int32)))
        return list(out), rnd[:self.n_views]

    def register_counts(self):
        """sfmloc_sfm_register_counts -> [n_views] uint32: per view the observations whose landmark is kept, as a
        registration round would count them now; nothing on the handle changes"""
        c = np.zeros(max(1, self.n_views), np.uint32)
        _check(_L().sfmloc_sfm_register_counts(self._h, _ptr(c, C.c_uint32)))
        return c[:self.n_views]

    def register_inliers(self, k):
        n = C.c_uint32(0)
        _check(_L().sfmloc_sfm_register_inliers(self._h, int(k), None, 0, C.byref(n)))
        idx = np.zeros(max(1, n.value), np.uint32)
        _check(_L().sfmloc_sfm_register_inliers(self._h, int(k), _ptr(idx, C.c_uint32), idx.size, C.byref(n)))
        return idx[:n.value].copy()

    def read_intrinsics(self):
        """-> the intrinsics [n_intrinsics, 6] (f, ppx, ppy, k1, k2, k3) as they are now"""
        K = np.zeros((len(self._keep["intrinsic_type"]), 6))
        _check(_L().sfmloc_sfm_read_intrinsics(self._h, _ptr(K, C.c_double)))
        return K

    def read_structure(self):
        """-> the landmarks' X [n_landmarks, 3] as they are now"""
        X = np.zeros((max(1, self.n_landmarks), 3))
        _check(_L().sfmloc_sfm_read_structure(self._h, _ptr(X, C.c_double)))
        return X[:self.n_landmarks]

    def debug_read(self):
        """-> (residual norm per observation, minimum clamped cosine per landmark); NaN where not evaluated"""
        res = np.zeros(max(1, self.n_obs))
        mc = np.zeros(max(1, self.n_landmarks))
        _check(_L().sfmloc_sfm_debug_read(self._h, _ptr(res, C.c_double), _ptr(mc, C.c_double)))
        return res[:self.n_obs], mc[:self.n_landmarks]

    def color_plan(self):
        """sfmloc_sfm_color_plan -> (order [n_order] view indices, lm_iter [n_landmarks] (COLOR_UNSET without
        observations), lm_obs [n_landmarks] observation index): which view each landmark takes its colour from"""
        order = np.zeros(max(1, self.n_views), np.uint32)
        it = np.full(max(1, self.n_landmarks), COLOR_UNSET, np.uint32)
        ob = np.zeros(max(1, self.n_landmarks), np.uint64)
        n = C.c_uint32(0)
        _check(_L().sfmloc_sfm_color_plan(self._h, _ptr(order, C.c_uint32), C.byref(n), _ptr(it, C.c_uint32),
                                          _ptr(ob, C.c_uint64)))
        return order[:n.value].copy(), it[:self.n_landmarks], ob[:self.n_landmarks]

    def close(self):
        if self._h:
            _L().sfmloc_sfm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def triangulate_default_options():
    """sfmloc_triangulate_default_options -> TriangulateOptions (robust, 3 inliers, pairs allowed, 4 px)"""
    o = TriangulateOptions()
    _L().sfmloc_triangulate_default_options(C.byref(o))
    return o


def register_default_options():
    """sfmloc_register_default_options -> RegisterOptions (16 rounds, more than 10 points, 4 px)"""
    o = RegisterOptions()
    _L().sfmloc_register_default_options(C.byref(o))
    return o


def pair_arrays(matches, view_index=None):
    """{(I, J): (i[], j[])} -> (pairs [n, 2] uint32, offsets [n + 1] uint64, match_i, match_j): the pair list layout of
    sfmloc_geometric_pairs and sfmloc_tracks_build, pairs in ascending (I, J); view_index maps a key to a view index"""
    keys = sorted(matches)
    ix = (lambda k: k) if view_index is None else (lambda k: view_index[k])
    pairs = np.array([[ix(a), ix(b)] for a, b in keys], np.uint32).reshape(-1, 2)
    off = np.zeros(len(keys) + 1, np.uint64)
    for k, key in enumerate(keys):
        off[k + 1] = off[k] + np.uint64(len(matches[key][0]))
    cat = (lambda c: np.concatenate([np.asarray(matches[k][c], np.uint32) for k in keys]) if keys
           else np.zeros(0, np.uint32))
    return pairs, off, cat(0), cat(1)


def _options(struct, default_fn, overrides):
    """a fresh `struct` filled by the library's default_fn, then the caller's fields; an unknown field is an error"""
    o = struct()
    getattr(_L(), default_fn)(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _pair_list(pairs, offsets, match_i, match_j):
    """the pair list of pair_arrays, coerced and length-checked -> (pairs [P, 2], offsets, match_i, match_j)"""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    match_i, match_j = np.ascontiguousarray(match_i, np.uint32), np.ascontiguousarray(match_j, np.uint32)
    if len(offsets) != len(pairs) + 1 or len(match_i) != len(match_j) or \
            (len(pairs) and int(offsets[-1]) != len(match_i)):
        raise ValueError("pair list arrays differ in length")
    return pairs, offsets, match_i, match_j


def _pair_scene(view_off, kpt_xy, view_wh, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j):
    """the two-view scene of RelPoses, RelRefine and WedgeScales, coerced and length-checked -> (the arrays, which the
    caller keeps alive over the call; the C arguments from view_off to match_j, with view_wh where it is not None)"""
    view_off = np.ascontiguousarray(view_off, np.uint64)
    kpt_xy = np.ascontiguousarray(kpt_xy, np.float32).reshape(-1, 2)
    view_intrinsic = np.ascontiguousarray(view_intrinsic, np.uint32)
    intrinsics = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 6)
    intrinsic_type = np.ascontiguousarray(intrinsic_type, np.uint32)
    n_views = len(view_off) - 1
    wh = () if view_wh is None else (np.ascontiguousarray(view_wh, np.uint32).reshape(-1, 2),)
    if any(len(a) != n_views for a in wh) or len(view_intrinsic) != n_views or len(intrinsic_type) != len(intrinsics) or \
            (n_views >= 0 and len(kpt_xy) != int(view_off[-1])):
        raise ValueError("view arrays differ in length")
    pairs, offsets, match_i, match_j = _pair_list(pairs, offsets, match_i, match_j)
    args = (_ptr(view_off, C.c_uint64), n_views, _ptr(kpt_xy, C.c_float), *(_ptr(a, C.c_uint32) for a in wh),
            _ptr(view_intrinsic, C.c_uint32), _ptr(intrinsics, C.c_double), _ptr(intrinsic_type, C.c_uint32),
            len(intrinsics), _ptr(pairs, C.c_uint32), len(pairs), _ptr(offsets, C.c_uint64), _ptr(match_i, C.c_uint32),
            _ptr(match_j, C.c_uint32))
    return (view_off, kpt_xy, wh, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j), args


def _pair_poses(P, rel_R, rel_t, inl_off, inl_idx, use_pair):
    """the results of RelPoses for P pairs that RelRefine and WedgeScales take, coerced and length-checked -> (the
    arrays, the C arguments from rel_R to use_pair)"""
    rel_R = np.ascontiguousarray(rel_R, np.float64).reshape(-1, 9)
    rel_t = np.ascontiguousarray(rel_t, np.float64).reshape(-1, 3)
    inl_off, inl_idx = np.ascontiguousarray(inl_off, np.uint64), np.ascontiguousarray(inl_idx, np.uint32)
    if use_pair is not None:
        use_pair = np.ascontiguousarray(np.asarray(use_pair) != 0, np.uint8)
    if len(rel_R) != P or len(rel_t) != P or len(inl_off) != P + 1 or (use_pair is not None and len(use_pair) != P) \
            or (P and int(inl_off[-1]) > len(inl_idx)):
        raise ValueError("pose or inlier arrays differ in length")
    args = (_ptr(rel_R, C.c_double), _ptr(rel_t, C.c_double), _ptr(inl_off, C.c_uint64), _ptr(inl_idx, C.c_uint32),
            None if use_pair is None else _ptr(use_pair, C.c_uint8))
    return (rel_R, rel_t, inl_off, inl_idx, use_pair), args


def tracks_last_ms():
    """device milliseconds of this thread's last Tracks()"""
    return float(_L().sfmloc_tracks_last_ms())


class Tracks:
    """sfmloc_tracks: feature tracks of a pair list (include/sfmloc.h states the semantics).  view_off [n_views + 1]
    feature rows per view; pairs [n, 2] view indices, offsets [n + 1], match_i / match_j as pair_arrays returns them;
    view_use [n_views] masks views out.  -> counts (components, dropped for conflict, dropped for length, kept),
    off [n_tracks + 1], view, feat."""

    def __init__(self, view_off, pairs, offsets, match_i, match_j, view_use=None, min_length=2, device=0):
        view_off = np.ascontiguousarray(view_off, np.uint64)
        if view_use is not None:
            view_use = np.ascontiguousarray(view_use, np.uint8)
            if len(view_use) != len(view_off) - 1:
                raise ValueError("view_use must have one entry per view")
        pairs, offsets, match_i, match_j = _pair_list(pairs, offsets, match_i, match_j)
        h = C.c_void_p()
        _check(_L().sfmloc_tracks_build(int(device), _ptr(view_off, C.c_uint64), len(view_off) - 1,
                                        _ptr(view_use, C.c_uint8), _ptr(pairs.reshape(-1), C.c_uint32), len(pairs),
                                        _ptr(offsets, C.c_uint64), _ptr(match_i, C.c_uint32), _ptr(match_j, C.c_uint32),
                                        int(min_length), C.byref(h)))
        try:
            counts = (C.c_uint64 * 4)()
            _check(_L().sfmloc_tracks_counts(h, counts))
            self.counts = [int(c) for c in counts]
            self.off = np.zeros(self.counts[3] + 1, np.uint64)
            _check(_L().sfmloc_tracks_read(h, _ptr(self.off, C.c_uint64), None, None))
            n = int(self.off[-1])
            self.view, self.feat = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint32)
            _check(_L().sfmloc_tracks_read(h, None, _ptr(self.view, C.c_uint32), _ptr(self.feat, C.c_uint32)))
            self.view, self.feat = self.view[:n], self.feat[:n]
            self.ms = tracks_last_ms()
        finally:
            _L().sfmloc_tracks_destroy(h)

    @property
    def n_tracks(self):
        return self.counts[3]


# sfmloc_relpose_result as a NumPy record (align=True gives the C layout: 13 uint32, 4 bytes of padding, 23 doubles)
RELPOSE_RESULT = np.dtype([("ok", np.uint32), ("n_matches", np.uint32), ("n_inliers", np.uint32),
                           ("sample", np.uint32, 5), ("front", np.uint32, 4), ("choice", np.uint32),
                           ("E", np.float64, 9), ("R", np.float64, 9), ("t", np.float64, 3),
                           ("error_max_px", np.float64), ("nfa", np.float64)], align=True)


def relpose_default_options(**overrides):
    """sfmloc_relpose_default_options -> RelposeOptions (256 iterations, 2.5 px, the default seed)"""
    return _options(RelposeOptions, "sfmloc_relpose_default_options", overrides)


def relpose_last_ms():
    """device milliseconds of this thread's last RelPoses()"""
    return float(_L().sfmloc_relpose_last_ms())


class RelPoses:
    """sfmloc_relative_poses: the relative pose of every pair of a pair list (include/sfmloc.h states the semantics).
    view_off [n_views + 1] feature rows per view, kpt_xy [rows, 2] float32, view_wh [n_views, 2], view_intrinsic
    [n_views], intrinsics [n, 6] (f, ppx, ppy, k1, k2, k3), intrinsic_type [n] (0 or 3); pairs, offsets, match_i,
    match_j as pair_arrays returns them; options: the fields of sfmloc_relpose_options.  -> results (RELPOSE_RESULT
    [n_pairs]), inl_off [n_pairs + 1], inl_idx (positions in each pair's match list, AC-RANSAC's order), ms."""

    def __init__(self, view_off, kpt_xy, view_wh, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i,
                 match_j, device=0, **options):
        keep, scene = _pair_scene(view_off, kpt_xy, view_wh, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets,
                                  match_i, match_j)
        pairs = keep[6]
        opt = relpose_default_options(**options)
        h = C.c_void_p()
        _check(_L().sfmloc_relative_poses(int(device), *scene, C.byref(opt), C.byref(h)))
        try:
            self.results = np.zeros(len(pairs), RELPOSE_RESULT)
            _check(_L().sfmloc_relpose_results(h, _ptr(self.results, RelposeResult) if len(pairs) else None))
            self.inl_off = np.zeros(len(pairs) + 1, np.uint64)
            _check(_L().sfmloc_relpose_inliers(h, _ptr(self.inl_off, C.c_uint64), None))
            n = int(self.inl_off[-1])
            idx = np.zeros(max(1, n), np.uint32)
            _check(_L().sfmloc_relpose_inliers(h, None, _ptr(idx, C.c_uint32)))
            self.inl_idx = idx[:n]
            self.ms = relpose_last_ms()
        finally:
            _L().sfmloc_relpose_destroy(h)

    def inliers(self, k):
        """the inlier positions of pair k"""
        return self.inl_idx[int(self.inl_off[k]):int(self.inl_off[k + 1])]


# sfmloc_relrefine_result as a NumPy record (four uint32, 23 doubles: no padding)
RELREFINE_RESULT = np.dtype([("status", np.uint32), ("n_used", np.uint32), ("steps", np.uint32), ("reserved", np.uint32),
                             ("R", np.float64, 9), ("t", np.float64, 3), ("E", np.float64, 9),
                             ("cost_initial", np.float64), ("cost", np.float64)], align=True)


def relrefine_default_options(**overrides):
    """sfmloc_relrefine_default_options -> RelrefineOptions (max_steps 100, min_points 13)"""
    return _options(RelrefineOptions, "sfmloc_relrefine_default_options", overrides)


def relrefine_last_ms():
    """device milliseconds of the calling thread's last sfmloc_refine_relative_poses"""
    return float(_L().sfmloc_relrefine_last_ms())


class RelRefine:
    """sfmloc_refine_relative_poses: every relative pose adjusted on its inliers (include/sfmloc.h "Two-view refinement"
    states the semantics).  The arguments are WedgeScales': the view and pair arrays of RelPoses (without view_wh), rel_R
    [P, 3, 3], rel_t [P, 3], inl_off [P + 1], inl_idx its results; use_pair [P] or None (all); options: the fields of
    sfmloc_relrefine_options.  -> results (RELREFINE_RESULT [P]; status 1 or 3: a refined pose), ms."""

    def __init__(self, view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j,
                 rel_R, rel_t, inl_off, inl_idx, use_pair=None, device=0, **options):
        keep, scene = _pair_scene(view_off, kpt_xy, None, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets,
                                  match_i, match_j)
        P = len(keep[6])
        keep_poses, poses = _pair_poses(P, rel_R, rel_t, inl_off, inl_idx, use_pair)
        opt = relrefine_default_options(**options)
        h = C.c_void_p()
        _check(_L().sfmloc_refine_relative_poses(int(device), *scene, *poses, C.byref(opt), C.byref(h)))
        try:
            self.results = np.zeros(P, RELREFINE_RESULT)
            _check(_L().sfmloc_relrefine_results(h, _ptr(self.results, RelrefineResult) if P else None))
            self.ms = relrefine_last_ms()
        finally:
            _L().sfmloc_relrefine_destroy(h)

    @property
    def refined(self):
        """[P] bool: the pairs whose R, t and E are the refinement's (status 1 or 3)"""
        return np.isin(self.results["status"], (1, 3))


# sfmloc_wscale as a NumPy record (four uint32, one double: no padding)
WSCALE = np.dtype([("view", np.uint32), ("k", np.uint32), ("l", np.uint32), ("n_shared", np.uint32),
                   ("ratio", np.float64)], align=True)


def wscales_default_options(**overrides):
    """sfmloc_wscales_default_options -> WscalesOptions (min_shared 8, max_shared 2048)"""
    return _options(WscalesOptions, "sfmloc_wscales_default_options", overrides)


def wscales_last_ms():
    """device milliseconds of the calling thread's last sfmloc_wedge_scales"""
    return float(_L().sfmloc_wscales_last_ms())


class WedgeScales:
    """sfmloc_wedge_scales: the ratio of the baselines of every two pairs that share a view, from the depths of the
    features they share (include/sfmloc.h "Wedge scales" states the semantics).  The view and pair arrays are RelPoses'
    (without view_wh); rel_R [P, 3, 3], rel_t [P, 3], inl_off [P + 1], inl_idx its results; use_pair [P] or None (all);
    options: the fields of sfmloc_wscales_options.  -> records (WSCALE [n_wedges], ordered by (k, l, view)), report
    (WscalesReport), ms."""

    def __init__(self, view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j,
                 rel_R, rel_t, inl_off, inl_idx, use_pair=None, device=0, **options):
        keep, scene = _pair_scene(view_off, kpt_xy, None, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets,
                                  match_i, match_j)
        keep_poses, poses = _pair_poses(len(keep[6]), rel_R, rel_t, inl_off, inl_idx, use_pair)
        opt = wscales_default_options(**options)
        h = C.c_void_p()
        _check(_L().sfmloc_wedge_scales(int(device), *scene, *poses, C.byref(opt), C.byref(h)))
        try:
            n = C.c_uint32()
            _check(_L().sfmloc_wscales_count(h, C.byref(n)))
            self.records = np.zeros(n.value, WSCALE)
            _check(_L().sfmloc_wscales_read(h, _ptr(self.records, Wscale) if n.value else None))
            self.report = WscalesReport()
            _check(_L().sfmloc_wscales_report_read(h, C.byref(self.report)))
            self.ms = wscales_last_ms()
        finally:
            _L().sfmloc_wscales_destroy(h)


# sfmloc_seed_score as a NumPy record (four uint32, one double: no padding)
SEED_SCORE = np.dtype([("n_inliers", np.uint32), ("n_used", np.uint32), ("candidate", np.uint32), ("reserved", np.uint32),
                       ("cos_median", np.float64)], align=True)


def seed_default_options(**overrides):
    """sfmloc_seed_default_options -> SeedOptions (min_used 100, max_cos cos 3 degrees, min_cos cos 60 degrees)"""
    return _options(SeedOptions, "sfmloc_seed_default_options", overrides)


def seed_last_ms():
    """device milliseconds of the calling thread's last sfmloc_seed_scores"""
    return float(_L().sfmloc_seed_last_ms())


def seed_choose(scores, pairs, view_pose):
    """the seed pair among the records (csrc/seed_host.h choose): a candidate whose two views have different id_pose,
    the smallest cos_median, then the larger n_used, then the smaller pair index -> its index, or -1"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    view_pose = np.asarray(view_pose, np.int64)
    best = -1
    for k, s in enumerate(scores):
        if not int(s["candidate"]) or view_pose[pairs[k, 0]] == view_pose[pairs[k, 1]]:
            continue
        if best < 0 or s["cos_median"] < scores[best]["cos_median"] or \
                (s["cos_median"] == scores[best]["cos_median"] and s["n_used"] > scores[best]["n_used"]):
            best = k
    return best


class SeedScores:
    """sfmloc_seed_scores: per pair the median cosine between the two rays of its inlier matches, and whether the pair
    may start an incremental reconstruction (include/sfmloc.h "Seed scores" states the semantics).  The arguments are
    WedgeScales'; options: the fields of sfmloc_seed_options.  -> scores (SEED_SCORE [P]), ms; choose(view_pose) -> the
    seed pair's index or -1."""

    def __init__(self, view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j,
                 rel_R, rel_t, inl_off, inl_idx, use_pair=None, device=0, **options):
        keep, scene = _pair_scene(view_off, kpt_xy, None, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets,
                                  match_i, match_j)
        self.pairs = keep[6]
        P = len(self.pairs)
        keep_poses, poses = _pair_poses(P, rel_R, rel_t, inl_off, inl_idx, use_pair)
        opt = seed_default_options(**options)
        h = C.c_void_p()
        _check(_L().sfmloc_seed_scores(int(device), *scene, *poses, C.byref(opt), C.byref(h)))
        try:
            self.scores = np.zeros(P, SEED_SCORE)
            _check(_L().sfmloc_seed_read(h, _ptr(self.scores, SeedScore) if P else None))
            self.ms = seed_last_ms()
        finally:
            _L().sfmloc_seed_destroy(h)

    def choose(self, view_pose):
        return seed_choose(self.scores, self.pairs, view_pose)


# sfmloc_gposes_pair as a NumPy record (four uint32, two doubles: no padding)
GPOSES_PAIR = np.dtype([("n_triplets", np.uint32), ("n_triplets_ok", np.uint32), ("kept", np.uint32),
                        ("used_t", np.uint32), ("rot_residual", np.float64), ("trans_residual", np.float64)], align=True)


def gposes_default_options(**overrides):
    """sfmloc_gposes_default_options -> GposesOptions (5 degrees, the derived rotation delta, 0.05, 1e-6, 1e-6, 50, 20000)"""
    return _options(GposesOptions, "sfmloc_gposes_default_options", overrides)


def gposes_last_ms():
    """device milliseconds of the calling thread's last sfmloc_global_poses"""
    return float(_L().sfmloc_gposes_last_ms())


def gpscale_default_options(**overrides):
    """sfmloc_gpscale_default_options -> GpscaleOptions (0.1, 1e-6, 1e-6, 50, 20000)"""
    return _options(GpscaleOptions, "sfmloc_gpscale_default_options", overrides)


class GlobalPoses:
    """sfmloc_global_poses: rotation and translation averaging over relative poses (include/sfmloc.h "Global poses"
    states the semantics).  pairs [P, 2] view indices, rel_R [P, 3, 3] and rel_t [P, 3] in sfmloc_relpose_result's
    convention, use_t [P] or None (all); options: the fields of sfmloc_gposes_options.  -> in_component [n] bool,
    R [n, 3, 3], C [n, 3], pairs (GPOSES_PAIR [P]), report (GposesReport), ms.
    wedges (a WSCALE array, or (kl [W, 2], ratio [W])): sfmloc_global_poses_scaled ("Scaled global poses") instead, with
    scale = the fields of sfmloc_gpscale_options; then also baselines [P], wedge_weights [W], scale_report
    (GpscaleReport)."""

    def __init__(self, n_views, pairs, rel_R, rel_t, use_t=None, device=0, wedges=None, scale=None, **options):
        pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        rel_R = np.ascontiguousarray(rel_R, np.float64).reshape(-1, 9)
        rel_t = np.ascontiguousarray(rel_t, np.float64).reshape(-1, 3)
        if use_t is not None:
            use_t = np.ascontiguousarray(np.asarray(use_t) != 0, np.uint8)
        if len(rel_R) != len(pairs) or len(rel_t) != len(pairs) or (use_t is not None and len(use_t) != len(pairs)):
            raise ValueError("pair arrays differ in length")
        n, P = int(n_views), len(pairs)
        opt = gposes_default_options(**options)
        h = C.c_void_p()
        if wedges is None:
            if scale is not None:
                raise ValueError("scale options without wedges")
            _check(_L().sfmloc_global_poses(int(device), n, _ptr(pairs, C.c_uint32), P, _ptr(rel_R, C.c_double),
                                            _ptr(rel_t, C.c_double), None if use_t is None else _ptr(use_t, C.c_uint8),
                                            C.byref(opt), C.byref(h)))
        else:
            if isinstance(wedges, np.ndarray) and wedges.dtype.names:
                wedges = (np.stack([wedges["k"], wedges["l"]], 1), wedges["ratio"])
            kl = np.ascontiguousarray(wedges[0], np.uint32).reshape(-1, 2)
            ratio = np.ascontiguousarray(wedges[1], np.float64).reshape(-1)
            if len(kl) != len(ratio):
                raise ValueError("wedge arrays differ in length")
            sopt = gpscale_default_options(**(scale or {}))
            _check(_L().sfmloc_global_poses_scaled(int(device), n, _ptr(pairs, C.c_uint32), P, _ptr(rel_R, C.c_double),
                                                   _ptr(rel_t, C.c_double),
                                                   None if use_t is None else _ptr(use_t, C.c_uint8), C.byref(opt),
                                                   _ptr(kl, C.c_uint32) if len(kl) else None,
                                                   _ptr(ratio, C.c_double) if len(kl) else None, len(kl), C.byref(sopt),
                                                   C.byref(h)))
        try:
            if wedges is not None:
                self.baselines, self.wedge_weights = np.zeros(P), np.zeros(len(kl))
                _check(_L().sfmloc_gpscale_baselines(h, _ptr(self.baselines, C.c_double) if P else None))
                _check(_L().sfmloc_gpscale_weights(h, _ptr(self.wedge_weights, C.c_double) if len(kl) else None))
                self.scale_report = GpscaleReport()
                _check(_L().sfmloc_gpscale_report_read(h, C.byref(self.scale_report)))
            inc = np.zeros(max(1, n), np.uint8)
            self.R, self.C = np.zeros((max(1, n), 3, 3)), np.zeros((max(1, n), 3))
            _check(_L().sfmloc_gposes_views(h, _ptr(inc, C.c_uint8), _ptr(self.R, C.c_double), _ptr(self.C, C.c_double)))
            self.in_component, self.R, self.C = inc[:n].astype(bool), self.R[:n], self.C[:n]
            self.pairs = np.zeros(P, GPOSES_PAIR)
            _check(_L().sfmloc_gposes_pairs(h, _ptr(self.pairs, GposesPair) if P else None))
            self.report = GposesReport()
            _check(_L().sfmloc_gposes_report_read(h, C.byref(self.report)))
            self.ms = gposes_last_ms()
        finally:
            _L().sfmloc_gposes_destroy(h)


def five_point(rows):
    """sfmloc_debug_five_point: rows [n, 20] (x1[10], x2[10]: five bearing pairs) -> (count [n], E [n, 10, 9])"""
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 20)
    out = np.zeros((len(rows), 91))
    _check(_L().sfmloc_debug_five_point(0, _ptr(rows, C.c_double), len(rows), _ptr(out, C.c_double)))
    return out[:, 0].astype(np.int64), out[:, 1:].reshape(-1, 10, 9)


def merge_default_params(**overrides):
    """sfmloc_merge_default_params: seed as default_params, device 0, rounds_per_launch 0 (the library's choice)"""
    p = MergeParams()
    _L().sfmloc_merge_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _pts(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1, 3)


def merge_ransac(A, B, thres, rounds, svd_ratio=1.75, model=MERGE_SIMILARITY, stream=0, params=None):
    """sfmloc_merge_ransac on matches A[n, 3] ~ M [B[n, 3]; 1] -> dict(M [3, 4] or None, round, count, inliers
    ascending uint32)"""
    A, B = _pts(A), _pts(B)
    if A.shape != B.shape:
        raise ValueError("A and B differ in shape")
    n = A.shape[0]
    res = MergeResult()
    idx = np.empty(max(n, 1), np.uint32)
    _check(_L().sfmloc_merge_ransac(_ptr(A, C.c_double), _ptr(B, C.c_double), n, float(thres), int(rounds), float(svd_ratio),
                                    int(model), int(stream), C.byref(params) if params is not None else None, C.byref(res),
                                    _ptr(idx, C.c_uint32), idx.size))
    return {"M": np.array(res.M, np.float64).reshape(3, 4) if res.has_model else None, "round": int(res.round),
            "count": int(res.count), "inliers": idx[:res.n_inliers].copy()}


def merge_inliers(A, B, M, thres, params=None):
    """sfmloc_merge_inliers: ascending indices of the matches within thres of M"""
    A, B = _pts(A), _pts(B)
    M = np.ascontiguousarray(M, np.float64).reshape(12)
    idx = np.empty(max(A.shape[0], 1), np.uint32)
    n = C.c_uint32(0)
    _check(_L().sfmloc_merge_inliers(_ptr(A, C.c_double), _ptr(B, C.c_double), A.shape[0], _ptr(M, C.c_double), float(thres),
                                     C.byref(params) if params is not None else None, _ptr(idx, C.c_uint32), idx.size,
                                     C.byref(n)))
    return idx[:n.value].copy()


def merge_median_nn(X, params=None):
    """sfmloc_merge_median_nn: the median distance to the nearest other point (0.0 for fewer than 2 points)"""
    X = _pts(X)
    out = C.c_double(0.0)
    _check(_L().sfmloc_merge_median_nn(_ptr(X, C.c_double), X.shape[0], C.byref(params) if params is not None else None,
                                       C.byref(out)))
    return out.value


def merge_transform(M, R=None, X=None, params=None):
    """sfmloc_merge_transform -> (M[:, :3] R for every rotation [k, 3, 3], M [X; 1] for every point [k, 3])"""
    M = np.ascontiguousarray(M, np.float64).reshape(12)
    R = np.array(np.zeros((0, 3, 3)) if R is None else R, np.float64).reshape(-1, 3, 3)
    X = np.array(np.zeros((0, 3)) if X is None else X, np.float64).reshape(-1, 3)
    _check(_L().sfmloc_merge_transform(_ptr(M, C.c_double), _ptr(R, C.c_double), R.shape[0], _ptr(X, C.c_double), X.shape[0],
                                       C.byref(params) if params is not None else None))
    return R, X


def merge_last_ms():
    return float(_L().sfmloc_merge_last_ms())


def reduce_points(X, A=None, thres=0.01, knn=1000, params=None, out=None):
    """sfmloc_reduce_points on landmarks X[n, 3] -> dict(owner uint32 [n], order uint32 [n_absorbed], dist f64 [n],
    n_keep, n_absorbed, n_pairs, rounds).  A: 3 x 4 or None (the identity).  out: (owner, order, dist) arrays to write
    into (each [n]; the tests watch them on a refused call)."""
    X = _pts(X)
    n = X.shape[0]
    A = None if A is None else np.ascontiguousarray(A, np.float64).reshape(12)
    owner, order, dist = out if out is not None else (np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.float64))
    res = ReduceResult()
    _check(_L().sfmloc_reduce_points(_ptr(X, C.c_double), n, None if A is None else _ptr(A, C.c_double), float(thres),
                                     int(knn), C.byref(params) if params is not None else None, _ptr(owner, C.c_uint32),
                                     _ptr(order, C.c_uint32), _ptr(dist, C.c_double), C.byref(res)))
    return {"owner": owner, "order": order[:res.n_absorbed], "dist": dist, "n_keep": int(res.n_keep),
            "n_absorbed": int(res.n_absorbed), "n_pairs": int(res.n_pairs), "rounds": int(res.rounds)}


def reduce_last_ms():
    return float(_L().sfmloc_reduce_last_ms())


def bowknn_default_options(**overrides):
    """sfmloc_bowknn_default_options -> BowknnOptions (k 20, window 0, rows_per_launch 0, profile 0)"""
    return _options(BowknnOptions, "sfmloc_bowknn_default_options", overrides)


def bow_knn(bow, k, window=0, rows_per_launch=0, device=0, profile=False, out=None):
    """sfmloc_bow_knn on the BoW vectors bow[n, dim]: for every view the k views nearest to it among those more than
    `window` places away (include/sfmloc.h "All-views BoW k-NN") -> (nbr uint32 [n, k] ascending per row, padded with
    0xFFFFFFFF; dist float32 [n, k], padded with +inf; count uint32 [n]).  out: (nbr, dist, count) arrays to write into
    (the tests watch them on a refused call)."""
    bow = np.ascontiguousarray(bow, np.float32)
    if bow.ndim != 2:
        raise ValueError("bow: an [n, dim] matrix")
    n, dim = bow.shape
    opt = bowknn_default_options(k=int(k), window=min(int(window), 0xFFFFFFFF), rows_per_launch=int(rows_per_launch), profile=int(bool(profile)))
    kk = max(int(k), 0)
    nbr, dist, count = out if out is not None else (np.empty((n, kk), np.uint32), np.empty((n, kk), np.float32),
                                                   np.empty(n, np.uint32))
    _check(_L().sfmloc_bow_knn(int(device), _ptr(bow, C.c_float), n, dim, C.byref(opt), _ptr(nbr, C.c_uint32),
                               _ptr(dist, C.c_float), _ptr(count, C.c_uint32)))
    return nbr, dist, count


def bowknn_last_ms():
    """device milliseconds of the calling thread's last sfmloc_bow_knn made with profile"""
    return float(_L().sfmloc_bowknn_last_ms())


class BowTrainer:
    """sfmloc_bowtrain: TrainBoW's training (TrainBoW.cpp) on the device -- the resident sample (host rows or the drawn dense
    rows of images), cv::PCA, the projection, cv::kmeans.  The fixed arithmetic is stated in include/sfmloc.h."""

    def __init__(self, dim=61, cap_rows=300000, device=0):
        self._h = None
        h = C.c_void_p()
        _check(_L().sfmloc_bowtrain_create(int(device), int(dim), int(cap_rows), C.byref(h)))
        self._h = h

    def reset(self):
        _check(_L().sfmloc_bowtrain_reset(self._h))

    def size(self):
        """-> (rows, dim) of the sample"""
        n, d = C.c_uint32(0), C.c_uint32(0)
        _check(_L().sfmloc_bowtrain_size(self._h, C.byref(n), C.byref(d)))
        return int(n.value), int(d.value)

    def add_rows(self, rows):
        rows = np.ascontiguousarray(rows, np.float32)
        _check(_L().sfmloc_bowtrain_add_rows(self._h, _ptr(rows.reshape(-1), C.c_float), rows.shape[0]))

    def add_image(self, image, n_pick, rng_state):
        """the dense rows of one image (h x w x 3 BGR or h x w gray; None = no descriptors) at n_pick draws of the cv::RNG
        state -> the state after the draws"""
        st = C.c_uint64(int(rng_state))
        if image is None:
            _check(_L().sfmloc_bowtrain_add_image(self._h, None, 0, 0, 3, int(n_pick), C.byref(st)))
            return int(st.value)
        img = np.ascontiguousarray(image, np.uint8)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        _check(_L().sfmloc_bowtrain_add_image(self._h, _ptr(img.reshape(-1), C.c_uint8), w, h, ch, int(n_pick), C.byref(st)))
        return int(st.value)

    def read(self):
        n, d = self.size()
        out = np.zeros((n, d), np.float32)
        _check(_L().sfmloc_bowtrain_read(self._h, _ptr(out.reshape(-1), C.c_float), out.size))
        return out

    def pca64(self):
        """-> (mean [d], cov [d, d], eigvec [d, d] rows, eigval [d]) in float64"""
        d = self.size()[1]
        m, c, v, e = np.zeros(d), np.zeros((d, d)), np.zeros((d, d)), np.zeros(d)
        _check(_L().sfmloc_bowtrain_pca64(self._h, *[_ptr(a.reshape(-1), C.c_double) for a in (m, c, v, e)]))
        return m, c, v, e

    def pca(self):
        """-> PCAfile.yml's arrays: MeanPCA [1, d], EigenVectorsPCA [d, d], EigenValuesPCA [d, 1] float32"""
        d = self.size()[1]
        m, v, e = np.zeros((1, d), np.float32), np.zeros((d, d), np.float32), np.zeros((d, 1), np.float32)
        _check(_L().sfmloc_bowtrain_pca(self._h, *[_ptr(a.reshape(-1), C.c_float) for a in (m, v, e)]))
        return m, v, e

    def project(self, mean, eigvec, eigval, n_pca):
        """the sample -> its first n_pca PCA coordinates divided by the eigenvalues, in place"""
        d, keep = _bof_desc(np.zeros((1, 1), np.float32), self.size()[1], pca_mean=mean, pca_eigvec=eigvec,
                            pca_eigval=eigval, n_pca=int(n_pca))
        _check(_L().sfmloc_bowtrain_project(self._h, C.byref(d)))

    def kmeans(self, K, attempts=3, max_iter=100, eps=float(np.finfo(np.float32).eps), seed=0xFFFFFFFF, want_labels=True,
               stats=None):
        """-> (centers [min(K, n), d] f32, labels [n] i32 or None, compactness).  stats (a dict): also "min_dist" [n] f32
        (the last assignment's) and "iterations" (assignments run, all attempts together)"""
        n, d = self.size()
        kc = min(int(K), n)
        cen = np.zeros((kc, d), np.float32)
        lab = np.zeros(n, np.int32) if want_labels else None
        mind = np.zeros(n, np.float32) if stats is not None else None
        comp, iters = C.c_double(0.0), C.c_uint32(0)
        _check(_L().sfmloc_bowtrain_kmeans(self._h, int(K), int(attempts), int(max_iter), float(eps), int(seed),
                                           _ptr(cen.reshape(-1), C.c_float), _ptr(lab, C.c_int32), _ptr(mind, C.c_float),
                                           C.byref(comp), C.byref(iters)))
        if stats is not None:
            stats["min_dist"], stats["iterations"] = mind, int(iters.value)
        return cen, lab, float(comp.value)

    def close(self):
        if self._h is not None:
            _L().sfmloc_bowtrain_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Akaze:
    """sfmloc_akaze: AKAZE + M-LDB extractor for one image size (extractAKAZESingleImg's compute part,
    AKAZEOpenCV.cpp:44-46,67; defaults AKAZEOption.h:31-34)."""

    def __init__(self, width, height, n_octaves=4, n_sublevels=4, threshold=0.001, device=0):
        self._h = None
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        _check(_L().sfmloc_akaze_create(device, self.width, self.height, n_octaves, n_sublevels, threshold, C.byref(h)))
        self._h = h
        n = C.c_int()
        wh = (C.c_int * 64)()
        _check(_L().sfmloc_akaze_levels(h, C.byref(n), wh))
        self.levels = [(wh[2 * i], wh[2 * i + 1]) for i in range(n.value)]

    def share_stream(self, ctx):
        """sfmloc_akaze_share_stream: queue the extraction on the context's stream (None: back on its own)."""
        _check(_L().sfmloc_akaze_share_stream(self._h, None if ctx is None else ctx._h))

    def detect_and_compute(self, gray, cap=65536):
        """-> kpts [n x 6] (x, y, size, angle, response, class_id), desc [n x 64] (.desc rows)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        assert gray.shape == (self.height, self.width)
        if getattr(self, "_out_cap", 0) != cap:      # output staging kept between calls (5.8 MB at the default cap)
            self._out_kp = np.zeros((cap, 6), np.float32)
            self._out_desc = np.zeros((cap, 64), np.uint8)
            self._out_cap = cap
        kp, desc = self._out_kp, self._out_desc
        n = C.c_uint32()
        _check(_L().sfmloc_akaze_detect_and_compute(self._h, _ptr(gray, C.c_uint8), _ptr(kp, C.c_float),
                                                    _ptr(desc, C.c_uint8), cap, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def detect_and_compute_dev(self, reader, which=IMREAD_GRAY, cap=65536):
        """sfmloc_akaze_detect_and_compute_dev: detect_and_compute on a DeviceImread's resident gray image"""
        if getattr(self, "_out_cap", 0) != cap:
            self._out_kp = np.zeros((cap, 6), np.float32)
            self._out_desc = np.zeros((cap, 64), np.uint8)
            self._out_cap = cap
        kp, desc = self._out_kp, self._out_desc
        n = C.c_uint32()
        _check(_L().sfmloc_akaze_detect_and_compute_dev(self._h, reader._h, int(which), _ptr(kp, C.c_float),
                                                        _ptr(desc, C.c_uint8), cap, C.byref(n)))
        return kp[:n.value].copy(), desc[:n.value].copy()

    def detect_resident_dev(self, reader, which=IMREAD_GRAY):
        """sfmloc_akaze_detect_resident_dev: detect_resident on a DeviceImread's resident gray image -> keypoints"""
        n = C.c_uint32()
        _check(_L().sfmloc_akaze_detect_resident_dev(self._h, reader._h, int(which), C.byref(n)))
        return int(n.value)

    @staticmethod
    def detect_and_compute_batch(extractors, grays, cap=65536):
        """sfmloc_akaze_detect_and_compute_batch: extractors[i] takes grays[i] (all of one size), the device side of
        detection as ONE launch per kernel for all of them -> [(kpts, desc)] as detect_and_compute gives."""
        n = len(extractors)
        assert n == len(grays) and n >= 1
        imgs = [np.ascontiguousarray(g, np.uint8) for g in grays]
        for e, g in zip(extractors, imgs):
            assert g.shape == (e.height, e.width)
            if getattr(e, "_out_cap", 0) != cap:
                e._out_kp = np.zeros((cap, 6), np.float32)
                e._out_desc = np.zeros((cap, 64), np.uint8)
                e._out_cap = cap
        aks = (C.c_void_p * n)(*[e._h for e in extractors])
        gp = (C.POINTER(C.c_uint8) * n)(*[_ptr(g, C.c_uint8) for g in imgs])
        kp = (C.POINTER(C.c_float) * n)(*[_ptr(e._out_kp, C.c_float) for e in extractors])
        dp = (C.POINTER(C.c_uint8) * n)(*[_ptr(e._out_desc, C.c_uint8) for e in extractors])
        n_out = (C.c_uint32 * n)()
        _check(_L().sfmloc_akaze_detect_and_compute_batch(aks, gp, n, kp, dp, cap, n_out))
        return [(e._out_kp[:n_out[i]].copy(), e._out_desc[:n_out[i]].copy()) for i, e in enumerate(extractors)]

    def resident_arrays(self):
        """sfmloc_akaze_resident_arrays -> device addresses (desc, kpt, kpt6, kp6) of the last resident detection"""
        p = [C.c_void_p() for _ in range(4)]
        _check(_L().sfmloc_akaze_resident_arrays(self._h, *[C.byref(x) for x in p]))
        return tuple(int(x.value or 0) for x in p)

    def detect_resident(self, gray):
        """sfmloc_akaze_detect_resident: outputs stay on the device as a query block -> number of keypoints"""
        gray = np.ascontiguousarray(gray, np.uint8)
        assert gray.shape == (self.height, self.width)
        n = C.c_uint32()
        _check(_L().sfmloc_akaze_detect_resident(self._h, _ptr(gray, C.c_uint8), C.byref(n)))
        return int(n.value)

    @staticmethod
    def detect_resident_batch(extractors, grays):
        n = len(extractors)
        imgs = [np.ascontiguousarray(g, np.uint8) for g in grays]
        aks = (C.c_void_p * n)(*[e._h for e in extractors])
        gp = (C.POINTER(C.c_uint8) * n)(*[_ptr(g, C.c_uint8) for g in imgs])
        n_out = (C.c_uint32 * n)()
        _check(_L().sfmloc_akaze_detect_resident_batch(aks, gp, n, n_out))
        return [int(x) for x in n_out]

    def query_view(self, m, n, bow_dev=0):
        """the last resident detection as a query of map m (sfmloc_query_create_view over the extractor's arrays)"""
        desc, kpt, kpt6, _ = self.resident_arrays()
        return m.query_view(desc, kpt, kpt6, bow_dev, n, self.width, self.height)

    def compute(self, gray, kin):
        gray = np.ascontiguousarray(gray, np.uint8)
        kin = np.ascontiguousarray(kin, np.float32).reshape(-1, 4)
        desc = np.zeros((kin.shape[0], 64), np.uint8)
        ang = np.zeros(kin.shape[0], np.float32)
        _check(_L().sfmloc_akaze_compute(self._h, _ptr(gray, C.c_uint8), _ptr(kin, C.c_float), kin.shape[0],
                                         _ptr(desc, C.c_uint8), _ptr(ang, C.c_float)))
        return desc, ang

    def read_levels(self):
        tot = sum(w * h for w, h in self.levels)
        ldet = np.zeros(tot, np.float32)
        lt = np.zeros(tot, np.float32)
        _check(_L().sfmloc_akaze_read_levels(self._h, _ptr(ldet, C.c_float), _ptr(lt, C.c_float)))
        return ldet, lt

    def suppress_stats(self):
        """The duplicate suppression of the last call (sfmloc_akaze_suppress_stats): counts and in-kernel clocks."""
        out = np.zeros(9, np.uint32)
        _check(_L().sfmloc_akaze_suppress_stats(self._h, _ptr(out, C.c_uint32)))
        names = ("candidates", "keypoints", "rounds", "first_pass_ticks", "second_pass_ticks", "compaction_ticks",
                 "spilled_ap", "spilled_n", "global_levels")
        return dict(zip(names, (int(v) for v in out)))

    def close(self):
        if self._h is not None:
            _L().sfmloc_akaze_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """sfmloc_context: one in-flight query (stream + workspace) on a map; begin() is asynchronous."""

    def __init__(self, m, share=None, merge_only=False):
        self._h = None
        self.map = m
        h = C.c_void_p()
        if merge_only:  # sfmloc_context_create_merge: for merge_begin[_packed] + end only, no matching workspace
            _check(_L().sfmloc_context_create_merge(m._h, None if share is None else share._h, C.byref(h)))
            self._lender = share
        elif share is None:
            _check(_L().sfmloc_context_create(m._h, C.byref(h)))
        else:       # sfmloc_context_create_sharing: no stream of its own, work goes to `share`'s
            _check(_L().sfmloc_context_create_sharing(m._h, share._h, C.byref(h)))
            self._lender = share
        self._h = h
        m._children.add(self)

    def begin(self, q, view_sel=None):
        if view_sel is None:
            _check(_L().sfmloc_localize_begin(self._h, q._h, None, 0))
        else:
            p, n, keep = _sel(view_sel)
            _check(_L().sfmloc_localize_begin(self._h, q._h, p, n))

    def begin_bow(self, q, bow, knn, cand_views=None):
        """sfmloc_localize_bow_begin: BoW shortlist (knn of the candidate views, all views when None) + the whole
        path on it, asynchronous, the shortlist never leaving the device.  Finish with end()."""
        b = None if bow is None else np.ascontiguousarray(bow, dtype=np.float32).ravel()   # None: q.set_bow()'s
        L = _L()
        if cand_views is None:
            _check(L.sfmloc_localize_bow_begin(self._h, q._h, _ptr(b, C.c_float), int(knn), None, 0))
        else:
            p, n, keep = _sel(cand_views)
            _check(L.sfmloc_localize_bow_begin(self._h, q._h, _ptr(b, C.c_float), int(knn), p, n))

    def shard_bow_keys(self, q, knn, keys_dev_ptr, bow=None):
        """sfmloc_shard_bow_keys: this shard's knn best (distance, view id) keys -> device buffer [knn] u64."""
        b = None if bow is None else np.ascontiguousarray(bow, dtype=np.float32).ravel()
        _check(_L().sfmloc_shard_bow_keys(self._h, q._h, _ptr(b, C.c_float), int(knn), C.c_void_p(keys_dev_ptr)))

    def shard_begin_bow(self, q, keys_dev_ptr, n_parts, knn, part_stride_keys=0):
        """sfmloc_shard_begin_bow: global knn best among the gathered key lists -> this shard's views -> K1..K3 +
        candidate emission, all on the device."""
        _check(_L().sfmloc_shard_begin_bow(self._h, q._h, C.c_void_p(keys_dev_ptr), int(n_parts),
                                           int(part_stride_keys), int(knn)))

    def shard_export_packed(self, packed_dev_ptr, n_queries, budget, query_index):
        _check(_L().sfmloc_shard_export_packed(self._h, C.c_void_p(packed_dev_ptr), n_queries, budget, query_index))

    def merge_begin_packed(self, q, packed_dev_ptr, n_parts, n_queries, budget, query_index, part_stride=0):
        _check(_L().sfmloc_merge_begin_packed(self._h, q._h, C.c_void_p(packed_dev_ptr), n_parts, part_stride, n_queries,
                                              budget, query_index))

    def signal(self, hip_stream=0):
        """sfmloc_context_signal: `hip_stream` (a hipStream_t as an integer) waits for this context's queued work."""
        _check(_L().sfmloc_context_signal(self._h, C.c_void_p(hip_stream)))

    def wait(self, hip_stream=0):
        """sfmloc_context_wait: this context waits for the work queued on `hip_stream` so far."""
        _check(_L().sfmloc_context_wait(self._h, C.c_void_p(hip_stream)))

    def shard_begin(self, q, view_sel=None):
        """K1..K3 + candidate emission on this shard (asynchronous)."""
        if view_sel is None:
            _check(_L().sfmloc_shard_begin(self._h, q._h, None, 0))
        else:
            p, n, keep = _sel(view_sel)
            _check(_L().sfmloc_shard_begin(self._h, q._h, p, n))

    def shard_export(self, dst_dev_ptr, cap):
        _check(_L().sfmloc_shard_export(self._h, C.c_void_p(dst_dev_ptr), cap))

    def sync(self):
        _check(_L().sfmloc_context_sync(self._h))

    def debug_views(self):
        """sfmloc_debug_context_views: the view list the last begin worked on (a sharded shortlist's phantom padding,
        index n_views, as written)."""
        n = C.c_uint32()
        out = np.zeros(self.map.n_views + 1, np.uint32)
        _check(_L().sfmloc_debug_context_views(self._h, _ptr(out, C.c_uint32), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def merge_begin(self, q, parts_dev_ptr, n_parts, cap, part_stride=0):
        _check(_L().sfmloc_merge_begin(self._h, q._h, C.c_void_p(parts_dev_ptr), n_parts, cap, part_stride))

    def end(self, cap=65536):
        pose = Pose()
        pq = np.zeros(cap, np.uint32)
        pl = np.zeros(cap, np.uint32)
        _check(_L().sfmloc_localize_end(self._h, C.byref(pose), _ptr(pq, C.c_uint32), _ptr(pl, C.c_uint32), cap))
        k = pose.n_inliers if pose.ok else 0
        return pose, pq[:k].copy(), pl[:k].copy()

    def close(self):
        if self._h is not None and self.map._h is not None:
            _L().sfmloc_context_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Query:
    """A query image's descriptors/keypoints resident in HBM (output of extractAKAZESingleImg,
    AKAZEOpenCV.cpp:37-113)."""

    def __init__(self, m, desc, kpt_xy=None, width=0, height=0):
        self._h = None
        self.map = m
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 64)
        self.n = desc.shape[0]
        if kpt_xy is not None:
            kpt_xy = np.ascontiguousarray(kpt_xy, dtype=np.float32).reshape(-1, 2)
            assert kpt_xy.shape[0] == self.n
        h = C.c_void_p()
        _check(_L().sfmloc_query_create(m._h, _ptr(desc, C.c_uint8), _ptr(kpt_xy, C.c_float), self.n,
                                        int(width), int(height), C.byref(h)))
        self._h = h
        m._children.add(self)

    def set_bow(self, bow):
        """sfmloc_query_set_bow: the query's BoW vector becomes resident with it."""
        b = np.ascontiguousarray(bow, dtype=np.float32).ravel()
        _check(_L().sfmloc_query_set_bow(self._h, _ptr(b, C.c_float)))

    def set_uncalibrated(self, on=True):
        """sfmloc_query_set_uncalibrated: no intrinsic is assumed for this query's camera -- the six-point resection
        instead of P3P, and the pose's K is the recovered one (include/sfmloc.h "Uncalibrated queries")."""
        _check(_L().sfmloc_query_set_uncalibrated(self._h, 1 if on else 0))

    @classmethod
    def _over_device_arrays(cls, m, desc_ptr, kpt_ptr, kpt6_ptr, bow_ptr, n, width, height):
        self = cls.__new__(cls)
        self._h = None
        self.map = m
        self.n = int(n)
        h = C.c_void_p()
        _check(_L().sfmloc_query_create_view(m._h, C.c_void_p(desc_ptr), C.c_void_p(kpt_ptr), C.c_void_p(kpt6_ptr),
                                             C.c_void_p(bow_ptr) if bow_ptr else None, int(n), int(width), int(height),
                                             C.byref(h)))
        self._h = h
        m._children.add(self)
        return self

    @classmethod
    def _from_view(cls, m, view_index):
        self = cls.__new__(cls)
        self._h = None
        self.map = m
        self.n = int(m.view_off[view_index + 1] - m.view_off[view_index])
        h = C.c_void_p()
        _check(_L().sfmloc_query_from_view(m._h, view_index, C.byref(h)))
        self._h = h
        m._children.add(self)
        return self

    def close(self):
        if self._h is not None and self.map._h is not None:
            _L().sfmloc_query_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
