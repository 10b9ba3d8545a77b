"""CPU: the homography entry points' place in the C ABI -- vis_homography_params (40 bytes) and vis_homography_result (112 bytes) in the C
compiler's layout and in the ctypes / numpy bindings, the defaults, VIS_H_TILE and the model codes, the four symbols exported and listed,
and every refusal that needs no device, in the header's order; VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import homography_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_homography_params", "vis_find_homography", "vis_homography_batch", "vis_batch_homography")
P_FIELDS = ("iters", "min_inliers", "chi2_h", "chi2_e", "sigma_px", "h_ratio")
R_FIELDS = ("H", "score_h", "score_e", "n_inliers", "n_points", "best_iter", "n_degenerate", "n_inliers_e", "model")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_homography_params, f)
#define R(f) (int)offsetof(vis_homography_result, f)
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_homography_params), P(iters), P(min_inliers), P(chi2_h), P(chi2_e), P(sigma_px), P(h_ratio));
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_homography_result), R(H), R(score_h), R(score_e), R(n_inliers), R(n_points),
           R(best_iter), R(n_degenerate), R(n_inliers_e), R(model));
    printf("%d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_H_TILE, (int)VIS_MODEL_NONE, (int)VIS_MODEL_HOMOGRAPHY,
           (int)VIS_MODEL_ESSENTIAL);
    return 0;
}
"""


def test_layout_in_c_and_ctypes(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [40, 0, 4, 8, 16, 24, 32]
    assert rows[1] == [112, 0, 72, 80, 88, 92, 96, 100, 104, 108]
    for S in (vislam.HomographyParams, hr.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    S = vislam.HomographyResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == rows[1]
    for d in (vislam.HOMOGRAPHY_RESULT_DTYPE, hr.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == rows[1]
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2] == vislam.H_TILE == 512
    assert rows[2][3:] == [vislam.MODEL_NONE, vislam.MODEL_HOMOGRAPHY, vislam.MODEL_ESSENTIAL] == [0, 1, 2]


def test_defaults(vislam):
    hp = vislam.default_homography_params()
    want = hr.default_params()
    assert [getattr(hp, f) for f in P_FIELDS] == [getattr(want, f) for f in P_FIELDS] == [200, 8, 5.991, 3.841, 1.0, 0.40]
    vislam.lib.vis_default_homography_params(None)                 # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("find_homography", "homography_batch", "batch_homography"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd = C.c_void_p(64), C.c_void_p(68)                     # never dereferenced: the argument / context checks come first
    hp = vislam.default_homography_params()
    ok = C.byref(hp)
    rec = np.full(1, 0, vislam.HOMOGRAPHY_RESULT_DTYPE)
    rec["best_iter"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    find = lambda hp_=ok, p1=some, p2=some, m=4, dr=some, E=None, mask=None, o=out: L.vis_find_homography(None, hp_, p1, p2, m, dr, E, mask, o)
    batch = lambda hp_=ok, n=1, p1=some, p2=some, npts=some, mx=49, dr=some, E=None, cap=49, mask=None, o=some: \
        L.vis_homography_batch(None, hp_, n, p1, p2, npts, mx, dr, E, cap, mask, o)
    plan = lambda hp_=ok, n=1, dr=some, cap=49, mask=None, o=some: L.vis_batch_homography(None, hp_, n, dr, cap, mask, o)
    # valid arguments, no context -> VIS_E_STATE
    assert find() == -5 and batch() == -5 and plan() == -5
    assert batch(E=some, mask=some) == -5 and plan(mask=some) == -5
    # a mask with a short row_cap: the context check comes first for the device-pointer call (the order of vis_filter_keypoints_batch)
    assert batch(mask=some, cap=48) == -5
    # NULL pointers -> VIS_E_INVALID
    assert find(hp_=None) == -1 and find(p1=None) == -1 and find(p2=None) == -1 and find(dr=None) == -1 and find(o=None) == -1
    assert batch(hp_=None) == -1 and batch(p1=None) == -1 and batch(p2=None) == -1 and batch(npts=None) == -1 and batch(dr=None) == -1 and batch(o=None) == -1
    assert plan(hp_=None) == -1 and plan(dr=None) == -1 and plan(o=None) == -1
    # misaligned pointers (8 bytes for points, E and records)
    assert batch(p1=odd) == -1 and batch(p2=odd) == -1 and batch(E=odd) == -1 and batch(o=odd) == -1 and plan(o=odd) == -1
    # negative sizes
    assert find(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1 and plan(n=-1) == -1 and plan(cap=-1) == -1
    # every parameter, on every call
    nan, inf = float("nan"), float("inf")
    bad = [("iters", -1), ("min_inliers", 3), ("min_inliers", -8)]
    for f in ("chi2_h", "chi2_e", "sigma_px"):
        bad += [(f, 0.0), (f, -1.0), (f, nan), (f, inf), (f, -inf)]
    bad += [("h_ratio", 0.0), ("h_ratio", 1.0), ("h_ratio", -0.1), ("h_ratio", 1.5), ("h_ratio", nan), ("h_ratio", inf)]
    for f, v in bad:
        q = vislam.default_homography_params()
        setattr(q, f, v)
        assert find(hp_=C.byref(q)) == -1 and batch(hp_=C.byref(q)) == -1 and plan(hp_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed
    for f, v in (("iters", 0), ("min_inliers", 4), ("h_ratio", 1e-9), ("h_ratio", 1.0 - 1e-9), ("sigma_px", 1e-300), ("chi2_h", 1e300)):
        q = vislam.default_homography_params()
        setattr(q, f, v)
        assert find(hp_=C.byref(q)) == -5 and batch(hp_=C.byref(q)) == -5 and plan(hp_=C.byref(q)) == -5, (f, v)
    q = vislam.default_homography_params()
    q.iters = 0
    assert find(hp_=C.byref(q), dr=None) == -5                     # no iterations: no table needed
    assert find(m=0, p1=None, p2=None, dr=None) == -5              # no points: no rows needed
    assert int(rec["best_iter"][0]) == 7 and not rec["H"].any()    # a refused call writes nothing
