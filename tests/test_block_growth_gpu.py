"""GPU: the host-pointer entry points size the context's two grow-only blocks (device scratch, pinned staging) from one buffer list
per call (csrc/vis_internal.h vis_carve).  ONE context runs the pair calls at m = 5, then 700, then 5 again, and an image call at
16 x 16 and 64 x 48: on the way up both blocks are replaced between calls, on the way down a call carves a block larger than it
needs.  Every result must be byte-identical to the same call on a context created fresh for it -- a list that measures differently from
how it binds, or a stage built on a block that was replaced afterwards, reads or writes the wrong bytes."""
import numpy as np
import pytest

import f2f_ref as fr
import homography_ref as hr

pytestmark = pytest.mark.gpu


def _blob(v):
    """any result (arrays, numpy records, ctypes structures, ints, nested tuples) as bytes"""
    if isinstance(v, (tuple, list)):
        return b"|".join(_blob(x) for x in v)
    if isinstance(v, (np.ndarray, np.generic)):
        return np.asarray(v).tobytes()
    if isinstance(v, (int, float)):
        return repr(v).encode()
    return bytes(v)


def _pair_calls(vislam, m):
    """[(name, call(context) -> result)] in the order of the shared context; inputs depend on m alone"""
    x1, x2, R, t = fr.two_view(m, 900 + m, 0.2, 0.5)
    ka, kb = fr.keypoints(vislam.KEYPOINT_DTYPE, x1), fr.keypoints(vislam.KEYPOINT_DTYPE, x2)
    rot, t32 = R.T.astype(np.float32), t.astype(np.float32)
    hdraws = hr.make_draws(m)
    idx = np.random.default_rng(m).integers(0, m, (300, 2)).astype(np.int32)

    def hpose(c):
        rec, mask = c.find_homography(x1, x2, hdraws)
        return c.homography_pose(rec, x1, x2, mask)

    def pose(c):
        E, mask, ninl, iters = c.essential_ransac(x1, x2)
        return (E, mask, ninl, iters) + tuple(c.recover_pose(E, x1, x2))

    return [("filter_keypoints", lambda c: c.filter_keypoints(ka, kb, rot, t32, 500.0)),
            ("find_homography", lambda c: c.find_homography(x1, x2, hdraws)),
            ("homography_pose", hpose),
            ("triangulate", lambda c: c.triangulate(R, t, x1, x2)),
            ("essential_ransac + recover_pose", pose),
            ("f2f_ransac", lambda c: c.f2f_ransac(ka, kb, rot, idx, 0.37))]


def _image_calls(vislam):
    rng = np.random.default_rng(5)
    return [(f"camera_update {w} x {h}", (lambda img: lambda c: c.camera_update(img))(rng.integers(0, 256, (h, w)).astype(np.uint8)))
            for w, h in ((16, 16), (64, 48))]


def test_one_context_through_growing_and_shrinking_calls(vislam):
    fresh = {}

    def want(key, call):
        if key not in fresh:                                       # (m = 5 comes twice: one reference)
            c = vislam.Context(0)
            fresh[key] = _blob(call(c))
            c.close()
        return fresh[key]

    shared = vislam.Context(0)
    for step, m in enumerate((5, 700, 5)):
        for name, call in _pair_calls(vislam, m) + (_image_calls(vislam) if step == 0 else []):
            got = _blob(call(shared))
            assert len(got) > 0 and got == want((name, m), call), (step, m, name)
    shared.close()
    assert len(fresh) == 14
