"""The comparison of one AKAZE extraction with the CPU restatement, shared by test_gpu_akaze.py and
test_gpu_akaze_shapes.py: level sizes, the nonlinear scale space and the determinant response, keypoints (six floats)
and descriptors (61 bytes + 3 zero ones) bit for bit, the keypoint count equal (zero included)."""
import numpy as np


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_outputs_equal(kp, desc, ekp, edesc, what=""):
    assert len(kp) == len(ekp), f"{what}: {len(kp)} keypoints, the restatement has {len(ekp)}"
    assert kp.shape == (len(ekp), 6) and desc.shape == (len(ekp), 64)
    np.testing.assert_array_equal(bits32(kp), bits32(ekp), err_msg=f"{what}: keypoints (x, y, size, angle, response, level)")
    np.testing.assert_array_equal(desc[:, :61], edesc, err_msg=f"{what}: descriptors")
    assert (desc[:, 61:] == 0).all()


def assert_extraction_matches_oracle(oracle_c, ak, g, threshold=0.001, n_octaves=4, n_sublevels=4, what=""):
    """ak (an extractor made with these parameters for g's size) on g -> (kp, desc), everything equal to the restatement's"""
    h, w = g.shape
    ekp, edesc, eldet, elt = oracle_c.akaze_detect_and_compute(g, threshold, n_octaves, n_sublevels, cap=65536, want_levels=True)
    assert [tuple(x) for x in oracle_c.akaze_levels(w, h, n_octaves, n_sublevels)] == ak.levels
    kp, desc = ak.detect_and_compute(g)
    ldet, lt = ak.read_levels()
    np.testing.assert_array_equal(bits32(lt), bits32(elt), err_msg=f"{what}: nonlinear scale space Lt")
    np.testing.assert_array_equal(bits32(ldet), bits32(eldet), err_msg=f"{what}: Hessian determinant response")
    assert_outputs_equal(kp, desc, ekp, edesc, what)
    return kp, desc
