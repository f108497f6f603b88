"""Named AKAZE requests at the sizes and octave settings where csrc/akaze.hip changes form or fills a table: octaves
evolved in LDS (k_octave_resident) and the run length it takes, the level table at 1 and at 32 levels, the octave cut,
the largest and smallest frames sfmloc_akaze_create accepts, the segment scan at its one- / two-launch boundary, the
output paths around their keypoint counts.  No device here: the cases are inputs, what each is for is asserted with the
CPU restatement alone in test_akaze_cases_cpu.py, and test_gpu_akaze_shapes.py runs them on the device.

The form conditions below restate the launch schedule of csrc/akaze_plan.h (what build_scale_space, akaze_detect_enqueue
and sfmloc_akaze_detect_and_compute launch by) over the level sizes the RESTATEMENT plans (oracle_c.akaze_levels): a case
stays on its side of a boundary whatever the library does.  They are the independent side: test_akaze_cases_cpu.py holds
these constants and conditions against the header's own (tests/cpp/akaze_plan.cpp prints them), so that a threshold
moved in the header alone turns the cases red instead of leaving them green off their boundary."""
from collections import namedtuple

import numpy as np

THRESHOLD = 0.001                 # AKAZEOption.h's default
LDS_BYTES = 150 * 1024            # k_octave_resident: three float images of the octave's size
RUN_MAX = 8                       # kOctaveRunMax: levels one k_octave_resident launch evolves
MAX_LEVELS = 32                   # kMaxLevels
SCAN_ONE_LAUNCH = 65536           # akaze_detect_enqueue: n_seg above this takes k_seg_sum + k_seg_write
SPEC_START, SPEC_MAX = 512, 4096  # Akaze::spec_n at creation, kSpecMax
CAND_CAP = 65536                  # kCandCap
STEPS_LARGE, STEPS_SMALL, SMALL_WIDTH = 4, 8, 160  # FED steps per launch of a level evolved by the per-level kernels
NBR_GRID = (384, 256, 4096)       # k_suppress_nbr: a workgroup per so many pixels, at least, at most
DESC_GRID = (96, 1024, 16384)     # k_orient_describe in a detection: the same
MIN_SIDE, MAX_W, MAX_H, MAX_OCTAVES = 16, 16384, 4096, 8  # what sfmloc_akaze_create accepts
# the constants above by the names csrc/akaze_plan.h gives them (test_akaze_cases_cpu.py: equal)
HEADER_NAMES = dict(kResidentLdsBytes=LDS_BYTES, kOctaveRunMax=RUN_MAX, kMaxLevels=MAX_LEVELS,
                    kSegScanOneLaunch=SCAN_ONE_LAUNCH, kSpecStart=SPEC_START, kSpecMax=SPEC_MAX, kCandCap=CAND_CAP,
                    kNldStepsLarge=STEPS_LARGE, kNldStepsSmall=STEPS_SMALL, kNldSmallWidth=SMALL_WIDTH,
                    kNbrPixPerGroup=NBR_GRID[0], kNbrGridMin=NBR_GRID[1], kNbrGridMax=NBR_GRID[2],
                    kDescPixPerGroup=DESC_GRID[0], kDescGridMin=DESC_GRID[1], kDescGridMax=DESC_GRID[2],
                    kMinSide=MIN_SIDE, kMaxWidth=MAX_W, kSupMaxRows=MAX_H + 1, kMaxOctaves=MAX_OCTAVES)


def blocks(seed, w, h, block=5, lo=30, hi=225):
    """Random two-level blocks of a few pixels (any size from 1 x 1 up; synthdata.texture_image needs 40 x 40)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    small = rng.integers(0, 2, ((h + block - 1) // block, (w + block - 1) // block))
    return (lo + (hi - lo) * np.kron(small, np.ones((block, block), np.int64))[:h, :w]).astype(np.uint8)


def sparse_blocks(seed, w, h, block=5, keep=0.1):
    """blocks() with most of the frame flat: few extrema, short CPU runs on large frames."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = blocks(seed + 1, w, h, block)
    cell = 8 * block
    on = rng.random(((h + cell - 1) // cell, (w + cell - 1) // cell)) < keep
    mask = np.kron(on, np.ones((cell, cell), bool))[:h, :w]
    return np.where(mask, g, 128).astype(np.uint8)


def patch(seed, w, h, size=20, x=100, y=80):
    """A flat frame with one small square of blocks(): a handful of keypoints"""
    g = constant(w, h)
    g[y:y + size, x:x + size] = blocks(seed, size, size)
    return g


def constant(w, h, value=128):
    return np.full((h, w), value, np.uint8)


# what a case promises (asserted on the CPU): levels; resident = per octave (run length, evolved in LDS?); seg = which
# side of SCAN_ONE_LAUNCH n_seg is on ("==" exactly on it); kp = (lo, hi) bounds of the keypoint count, inclusive;
# edge = "rows" / "cols": keypoints in the last 64 rows / columns
Case = namedtuple("Case", "name w h n_octaves n_sublevels threshold image what levels resident seg kp edge")


def case(name, w, h, what, levels, resident, kp, n_octaves=4, n_sublevels=4, threshold=THRESHOLD, image=None, seg="<",
         edge=None):
    image = image or (lambda: blocks(5, w, h))
    return Case(name, w, h, n_octaves, n_sublevels, threshold, image, what, levels, resident, seg, kp, edge)


NONE, FEW, SOME, MANY = (0, 0), (1, SPEC_START), (1, SPEC_MAX), (SPEC_MAX + 1, CAND_CAP)

CASES = [
    # ---- frame sizes, default parameters -----------------------------------------------------------------------------
    case("16x16", 16, 16, "the smallest frame: a quarter of one 64-pixel segment, no keypoint", 4, [(3, True)], NONE),
    case("47x33", 47, 33, "odd sizes below one segment", 4, [(3, True)], NONE),
    case("64x64", 64, 64, "exactly one segment per row", 4, [(3, True)], FEW),
    case("128x100", 128, 100, "the largest frame whose octave 0 is evolved in LDS (153 600 bytes exactly)", 4,
         [(3, True)], FEW),
    case("129x100", 129, 100, "one column more: octave 0 by the per-level kernels", 4, [(3, False)], FEW),
    case("160x80", 160, 80, "the smallest frame that keeps octave 1 (80 x 40)", 8, [(3, True), (4, True)], FEW),
    case("159x80", 159, 80, "octave 1 cut by its width (79 < 80)", 4, [(3, True)], FEW),
    case("160x79", 160, 79, "octave 1 cut by its height (39 < 40)", 4, [(3, True)], FEW),
    case("16x4096", 16, 4096, "the tallest frame at the smallest width: the row tables of k_suppress full, no keypoint", 4,
         [(3, False)], NONE),
    case("80x4096", 80, 4096, "the tallest frame: keypoints in the last rows of full row tables", 4, [(3, False)], SOME,
         edge="rows"),
    case("160x4096", 160, 4096, "the tallest frame with two octaves (n_seg = 98 304)", 8, [(3, False), (4, False)], MANY,
         seg=">", edge="rows"),
    case("16384x16", 16384, 16, "the widest frame at the smallest height, no keypoint", 4, [(3, False)], NONE),
    case("16384x64", 16384, 64, "the widest frame: the largest x packed into a candidate; n_seg = 65 536, the last size "
         "of the one-launch scan", 4, [(3, False)], SOME, seg="==", edge="cols"),
    case("16384x65", 16384, 65, "one row more: n_seg = 66 560, the first size of the two-launch scan", 4, [(3, False)],
         SOME, seg=">", edge="cols"),
    case("1024x544", 1024, 544, "four octaves just below the scan boundary (n_seg = 65 280)", 16,
         [(3, False), (4, False), (4, False), (4, True)], MANY, image=lambda: blocks(5, 1024, 544)),
    case("1024x548", 1024, 548, "four octaves just above the scan boundary (n_seg = 65 728)", 16,
         [(3, False), (4, False), (4, False), (4, True)], MANY, seg=">", image=lambda: blocks(5, 1024, 548)),
    # ---- octave settings ---------------------------------------------------------------------------------------------
    case("o1s1", 320, 240, "one level: no evolution at all", 1, [(0, False)], SOME, n_octaves=1, n_sublevels=1),
    case("o1s4", 320, 240, "one octave", 4, [(3, False)], SOME, n_octaves=1),
    case("o2s1", 320, 240, "one sub-level: every level starts with a half-sampling", 2, [(0, False), (1, False)], SOME,
         n_octaves=2, n_sublevels=1),
    case("o3s1", 320, 240, "one sub-level, the last octave (80 x 60) a resident run of one", 3,
         [(0, False), (1, False), (1, True)], SOME, n_octaves=3, n_sublevels=1),
    case("o3s2", 320, 240, "runs of 1 and 2", 6, [(1, False), (2, False), (2, True)], SOME, n_octaves=3, n_sublevels=2),
    case("o2s8", 320, 240, "sixteen levels in two octaves", 16, [(7, False), (8, False)], SOME, n_octaves=2,
         n_sublevels=8),
    case("o2s8_lds", 256, 200, "a later octave (128 x 100) at the longest resident run (8)", 16, [(7, False), (8, True)],
         SOME, n_octaves=2, n_sublevels=8),
    case("o2s9_lds", 256, 200, "a later octave (128 x 100) one past the longest resident run", 18,
         [(8, False), (9, False)], SOME, n_octaves=2, n_sublevels=9),
    case("o2s16", 320, 240, "32 levels in two octaves: every level table full, one-step FED cycles", 32,
         [(15, False), (16, False)], SOME, n_octaves=2, n_sublevels=16),
    case("o1s9", 128, 100, "octave 0 at the longest resident run (8 evolved levels)", 9, [(8, True)], FEW, n_octaves=1,
         n_sublevels=9),
    case("o1s10", 128, 100, "octave 0 one past the longest resident run", 10, [(9, False)], FEW, n_octaves=1,
         n_sublevels=10),
    case("o1s32", 128, 96, "32 levels in one octave", 32, [(31, False)], FEW, n_octaves=1, n_sublevels=32),
    case("o8_small", 200, 100, "eight octaves asked for, the cut leaves two", 4, [(1, False), (2, True)], FEW, n_octaves=8,
         n_sublevels=2),
    case("o5s3", 1280, 640, "five octaves (the smallest frame that has them), sparse content", 15,
         [(2, False), (3, False), (3, False), (3, True), (3, True)], SOME, n_octaves=5, n_sublevels=3, seg=">",
         image=lambda: sparse_blocks(7, 1280, 640)),
    # ---- thresholds --------------------------------------------------------------------------------------------------
    case("thres1e-4", 320, 240, "a low threshold", 12, [(3, False), (4, False), (4, True)], SOME, threshold=1e-4),
    case("thres1e-2", 320, 240, "a high threshold", 12, [(3, False), (4, False), (4, True)], SOME, threshold=1e-2),
    case("thres10", 320, 240, "a threshold nothing passes: candidates none, keypoints none", 12,
         [(3, False), (4, False), (4, True)], NONE, threshold=10.0),
    case("constant", 320, 240, "a constant image: zero gradients, zero candidates", 12, [(3, False), (4, False), (4, True)],
         NONE, image=lambda: constant(320, 240)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# ---- one 320 x 240 extractor across the output paths of sfmloc_akaze_detect_and_compute: the speculative download
# (n <= spec_n; spec_n = 512 at first, then the last count + a quarter in steps of 256, 256 .. 4 096) and the second
# copy.  One octave of 32 sub-levels and a low threshold, so that a frame this small can have more than 4 096 keypoints.
# (name, image, (lo, hi) of the keypoint count); the order is the order of the calls.
PATH_W, PATH_H = 320, 240
PATH_PARAMS = dict(n_octaves=1, n_sublevels=32, threshold=1e-5)
PATH_SEQUENCE = [
    ("none", lambda: constant(PATH_W, PATH_H), NONE),                             # speculative; spec_n 512 -> 256
    ("few", lambda: patch(3, PATH_W, PATH_H), (1, 256)),                         # speculative; spec_n stays 256
    ("some", lambda: sparse_blocks(3, PATH_W, PATH_H, 5, 0.3), (513, SPEC_MAX)),  # n > spec_n: the second copy
    ("many", lambda: blocks(11, PATH_W, PATH_H, 2), (SPEC_MAX + 1, CAND_CAP)),    # n > the cap of spec_n
    ("few again", lambda: patch(3, PATH_W, PATH_H), (1, 256)),                   # spec_n = 4 096: speculative again
]

# ---- more extrema than the candidate workspace holds (ECAP).  Keypoints are a subset of the candidates, so a frame on
# which the restatement alone finds more than CAND_CAP keypoints overflows it for certain.  The restatement's count on
# this frame is OVERFLOW_KEYPOINTS (about 14 s on one CPU core: counted once, by hand, not in the suite); the same
# extractor then takes the ordinary frame.
OVERFLOW_W, OVERFLOW_H = 896, 512
OVERFLOW_KEYPOINTS = 73871
OVERFLOW_PARAMS = dict(n_octaves=1, n_sublevels=32, threshold=1e-5)


def overflow_image():
    return blocks(21, OVERFLOW_W, OVERFLOW_H, 2)


def overflow_ordinary_image():
    return sparse_blocks(22, OVERFLOW_W, OVERFLOW_H, 5, 0.05)


# ---- the form conditions, from level sizes -----------------------------------------------------------------------------

def octaves(levels):
    """[(w, h), ...] of the restatement's levels -> [(w, h, number of levels)] per octave (an octave halves both sides)"""
    out = []
    for w, h in levels:
        if out and out[-1][:2] == (int(w), int(h)):
            out[-1] = (int(w), int(h), out[-1][2] + 1)
        else:
            out.append((int(w), int(h), 1))
    return out


def resident_plan(levels, need=None):
    """-> per octave (run, resident): the levels the evolution loop builds in it (octave 0: all but level 0, which the
    Gaussian gives) and whether build_scale_space hands them to k_octave_resident in one launch.  need: only the levels
    [0, need) are built (a description-only call whose keypoints stop at level need - 1)"""
    out = []
    for i, (w, h, n) in enumerate(octaves(levels[:need])):
        run = n - 1 if i == 0 else n
        out.append((run, run >= 1 and 3 * w * h * 4 <= LDS_BYTES and run <= RUN_MAX))
    return out


def fixed_grid(w, h, grid):
    """the workgroups of a kernel that strides over candidates / keypoints whose number only the device knows"""
    per, lo, hi = grid
    return min(max(w * h // per, lo), hi)


# ---- the description-only path cut short: the schedule's second input is the number of levels a call builds, and a run
# cut short can change form.  (name, frame, octave settings, levels the cut call builds, resident_plan of the cut call
# and of the whole one); test_gpu_akaze_shapes.py describes dense_keypoints on one extractor, cut short and whole.
NeedCase = namedtuple("NeedCase", "name w h n_octaves n_sublevels need cut whole")
NEED_CASES = [
    NeedCase("160x80_levels0-5", 160, 80, 4, 4, 6, [(3, True), (2, True)], [(3, True), (4, True)]),
    NeedCase("128x100_o1s10_levels0-8", 128, 100, 1, 10, 9, [(8, True)], [(9, False)]),
]


def n_seg(levels, w):
    """akaze.hip's n_seg: two 64-pixel segments per 128 columns of the FRAME's width, for every row of every level"""
    return sum(int(h) for _, h in levels) * 2 * ((w + 127) // 128)


def dense_keypoints(levels, w, h, step=6):
    """Keypoints for the description-only path, [n x 4] (x, y, size, class_id): a grid on every level of the plan"""
    xs, ys = np.arange(0, w, step, dtype=np.float32), np.arange(0, h, step, dtype=np.float32)
    kin, size = [], 4.0
    for lvl in range(len(levels)):
        kin += [(x, y, size, lvl) for y in ys for x in xs]
        size *= 1.25
    return np.array(kin, np.float32)
