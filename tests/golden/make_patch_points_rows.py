"""Records tests/golden/patch_points_rows.npz: orc_patch_points' rows on two keypoint lists inside [-2^20, 2^20], written with the oracle
library of the commit BEFORE the candidate window was given a rule for every float (VIS_ORACLE_LIB names that build; the loop it ran ends
on these lists).  tests/test_align_hostile_ref.py compares today's oracle with these bytes.

    VIS_ORACLE_LIB=/path/to/the/parent/libvis_oracle.so python tests/golden/make_patch_points_rows.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "vi-slam_amd"))
import oracle_bind as orc  # noqa: E402
import vislam  # noqa: E402


def lists():
    rng = np.random.default_rng(0)                      # tests/test_align_gpu.py::test_align_batch_explicit_points_and_init, pair 1
    pts = np.zeros((3, 230, 2), np.float32)
    pts[..., 0] = rng.uniform(-2, 320 + 2, (3, 230)); pts[..., 1] = rng.uniform(-2, 240 + 2, (3, 230))
    out = {"uniform320": (pts[1], 320, 240)}
    # windows clipped on each side of each level of 160 x 120: coordinates from 12 px outside to 12 px inside every border (on level l a
    # window is 2^l * patch wide), at integer, .5 and arbitrary positions, against both coordinates in the middle
    w, h = 160, 120
    edge = np.concatenate([np.arange(-12, 13, 1.5), np.arange(-90, -12, 13.0), [0.25, -0.5, 0.5, -1.0]]).astype(np.float32)
    xy = [(x, h / 2) for x in edge] + [(w - 1 - x, h / 2 + 0.5) for x in edge] + [(w / 2, y) for y in edge] + [(w / 2 + 0.5, h - 1 - y) for y in edge]
    xy += [(x, y) for x in (-3.0, 2.5, w - 3.5, w + 2.0) for y in (-3.0, 2.5, h - 3.5, h + 2.0)]
    out["clipped160"] = (np.array(xy[:200], np.float32), w, h)
    return out


if __name__ == "__main__":
    assert os.environ.get("VIS_ORACLE_LIB"), __doc__
    arrays = {}
    for name, (xy, w, h) in lists().items():
        kp = np.zeros(len(xy), vislam.KEYPOINT_DTYPE)
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        arrays[f"{name}_xy"] = xy
        arrays[f"{name}_wh"] = np.array([w, h], np.int32)
        for l in range(5):
            arrays[f"{name}_L{l}"] = orc.patch_points(kp, w, h, l)
            print(name, l, arrays[f"{name}_L{l}"].shape)
    np.savez_compressed(os.path.join(HERE, "patch_points_rows.npz"), **arrays)
