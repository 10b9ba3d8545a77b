"""The row sets the bundle-adjustment tests share (tests/test_ba_ref.py on the CPU, tests/test_ba_gpu.py on the device): not a test module.
A case is dict(prev, nkp, obs, xy, poses, row_cap[, truth]) as ba_ref.ba_rows takes them."""
import numpy as np

import ba_ref as br
import ftrack_ref as fr

CAM = fr.Camera(458.0, 458.0, 376.0, 240.0)                         # the prototype's camera (tests/test_ftrack_ref.py uses the same)


def scene(seed, n, n_pts, noise=0.3, row_cap=None):
    """the planted scene of ba_ref.scene at n cameras (n may be 0 or 1: rows without windows)"""
    if n == 0:
        R = row_cap or 8
        return dict(prev=np.zeros(0, np.int32), nkp=np.zeros(0, np.int32), obs=np.zeros((0, R), fr.OBS_DTYPE), xy=np.zeros((0, R, 2), np.float32),
                    poses=np.zeros((0, 12)), truth=np.zeros((0, 12)), row_cap=R)
    sc = br.scene(seed, CAM, n_cam=n, n_pts=n_pts, noise=noise, span=(min(3, n), min(12, n)))
    if row_cap is not None:
        assert row_cap >= sc["row_cap"]
        pad = row_cap - sc["row_cap"]
        obs = np.zeros((n, row_cap), fr.OBS_DTYPE)
        obs[:] = fr.EMPTY_OBS
        obs[:, :sc["row_cap"]] = sc["obs"]
        sc["obs"], sc["xy"], sc["row_cap"] = obs, np.concatenate([sc["xy"], np.zeros((n, pad, 2), np.float32)], 1), row_cap
    return sc


def chain(seed, n, K, row_cap, noise=0.3):
    """n cameras that all see the same K points, keypoint k of every frame the same point: every frame has exactly K keypoints"""
    sc = br.scene(seed, CAM, n_cam=n, n_pts=max(K, 1), noise=noise, span=(n, n))
    obs = np.zeros((n, row_cap), fr.OBS_DTYPE)
    obs[:] = fr.EMPTY_OBS
    xy = np.zeros((n, row_cap, 2), np.float32)
    obs[:, :K], xy[:, :K] = sc["obs"][:, :K], sc["xy"][:, :K]
    sc["obs"], sc["xy"], sc["row_cap"], sc["nkp"] = obs, xy, row_cap, np.full(n, K, np.int32)
    return sc


def pivot_case():
    """one window of 8 free frames of which frame 5 has a pose and no keypoint: its 6 x 6 block is zero, the camera pivot fails in every linearisation"""
    sc = scene(11, 9, 150)
    sc["nkp"] = sc["nkp"].copy()
    sc["nkp"][5] = 0
    return sc


HOSTILE = ("nan_anchor", "nan_inside", "nan_shared", "zero_anchor", "zero_inside", "zero_shared", "pixels", "tree", "prev_kp")


def hostile(kind):
    """9 frames, stride 4: windows 0 (frames 0 ... 4) and 1 (4 ... 8).  Returns (case, the windows whose own frames were left alone)"""
    sc = scene(21, 9, 160)
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    clean = []
    if kind.startswith(("nan_", "zero_")):
        f = dict(anchor=0, inside=2, shared=4)[kind.split("_")[1]]
        if kind.startswith("nan_"):
            sc["poses"][f, 7] = np.nan
        else:
            sc["poses"][f, :9] = 0.0
        clean = [] if f == 4 else [1]
    elif kind == "pixels":
        sc["xy"][1, 0, 0], sc["xy"][1, 1, 1], sc["xy"][2, 2, 0] = np.nan, np.inf, -np.inf
        sc["xy"][2, 3, 0], sc["xy"][3, 0, 1], sc["xy"][3, 1] = 3e38, -3e38, (3e38, 3e38)
        clean = [1]
    elif kind == "tree":
        sc["prev"][3] = 1                                           # frames 2 and 3 both continue frame 1
        clean = [1]
    elif kind == "prev_kp":
        sc["obs"]["prev_kp"][2, 0], sc["obs"]["prev_kp"][2, 1], sc["obs"]["prev_kp"][3, 0] = 10 ** 6, -5, int(sc["nkp"][2])
        clean = [1]
    return sc, clean


def all_finite(poses_in, out, windows, points):
    """no NaN or infinity in any record; a frame whose input pose is finite has a finite output pose (a frame without a pose keeps its bytes)"""
    posed = np.isfinite(poses_in).all(1) if len(poses_in) else np.zeros(0, bool)
    return bool(np.isfinite(out[posed]).all() and all(np.isfinite(windows[f]).all() for f in ("cost0", "cost1", "lambda_", "scale")) and
                np.isfinite(points["X"]).all() and np.isfinite(points["rms0_px"]).all() and np.isfinite(points["rms1_px"]).all())
