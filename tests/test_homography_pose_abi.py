"""CPU: the homography-pose entry points' place in the C ABI -- vis_hpose_params (48 bytes) and vis_hpose_result (320 bytes) in the C compiler's
layout and in the ctypes / numpy bindings, the defaults, the kind and flag codes, the four symbols exported and listed, and every refusal that
needs no device, in the header's order; VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import homography_pose_ref as hpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_hpose_params", "vis_homography_pose", "vis_homography_pose_batch", "vis_batch_homography_pose")
P_FIELDS = ("min_t_over_d", "max_cos_parallax", "ambiguity_ratio", "good_share", "parallax_share", "min_good", "reserved_")
R_FIELDS = ("R", "t", "n", "R2", "t2", "n2", "sv", "t_norm", "n_good", "kind", "flags", "solution", "second", "n_tested", "n_parallax", "n_points",
            "reserved_")
P_LAYOUT = [48, 0, 8, 16, 24, 32, 40, 44]
R_LAYOUT = [320, 0, 72, 96, 120, 192, 216, 240, 264, 272, 288, 292, 296, 300, 304, 308, 312, 316]

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_hpose_params, f)
#define R(f) (int)offsetof(vis_hpose_result, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(vis_hpose_params), P(min_t_over_d), P(max_cos_parallax), P(ambiguity_ratio), P(good_share),
           P(parallax_share), P(min_good), P(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_hpose_result), R(R), R(t), R(n), R(R2), R(t2), R(n2), R(sv),
           R(t_norm), R(n_good), R(kind), R(flags), R(solution), R(second), R(n_tested), R(n_parallax), R(n_points), R(reserved_));
    printf("%d %d %d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_HP_NONE, (int)VIS_HP_ROTATION, (int)VIS_HP_PLANE,
           (int)VIS_HPF_AMBIGUOUS, (int)VIS_HPF_HINTED, (int)VIS_HPF_FEW, (int)VIS_HPF_LOW_PARALLAX);
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
    assert rows[0] == P_LAYOUT and rows[1] == R_LAYOUT
    for S in (vislam.HposeParams, hpr.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == P_LAYOUT
    S = vislam.HposeResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == R_LAYOUT
    for d in (vislam.HPOSE_RESULT_DTYPE, hpr.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == R_LAYOUT
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2:5] == [vislam.HP_NONE, vislam.HP_ROTATION, vislam.HP_PLANE] == [hpr.HP_NONE, hpr.HP_ROTATION, hpr.HP_PLANE] == [0, 1, 2]
    assert rows[2][5:] == [vislam.HPF_AMBIGUOUS, vislam.HPF_HINTED, vislam.HPF_FEW, vislam.HPF_LOW_PARALLAX] == [1, 2, 4, 8]
    assert [hpr.HPF_AMBIGUOUS, hpr.HPF_HINTED, hpr.HPF_FEW, hpr.HPF_LOW_PARALLAX] == [1, 2, 4, 8]


def test_defaults(vislam):
    hq = vislam.default_hpose_params()
    want = hpr.default_params()
    assert [getattr(hq, f) for f in P_FIELDS] == [getattr(want, f) for f in P_FIELDS] == [0.05, 0.9998476951563913, 0.75, 0.9, 0.5, 8, 0]
    assert abs(hq.max_cos_parallax - math.cos(math.radians(1.0))) < 1e-15
    vislam.lib.vis_default_hpose_params(None)                      # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("homography_pose", "homography_pose_batch", "batch_homography_pose"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd = C.c_void_p(64), C.c_void_p(68)                     # never dereferenced: the argument / context checks come first
    hq = vislam.default_hpose_params()
    ok = C.byref(hq)
    rec = np.zeros(1, vislam.HPOSE_RESULT_DTYPE)
    rec["solution"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    one = lambda hq_=ok, h=some, p1=some, p2=some, m=4, mask=None, rot=None, o=out: L.vis_homography_pose(None, hq_, h, p1, p2, m, mask, rot, o)
    batch = lambda hq_=ok, n=1, h=some, p1=some, p2=some, npts=some, mx=49, cap=49, mask=None, rot=None, o=some: \
        L.vis_homography_pose_batch(None, hq_, n, h, p1, p2, npts, mx, cap, mask, rot, o)
    plan = lambda hq_=ok, n=1, h=some, cap=49, mask=None, rot=None, o=some: L.vis_batch_homography_pose(None, hq_, n, h, cap, mask, rot, o)
    # valid arguments, no context -> VIS_E_STATE; the mask and the hint may be given or NULL
    assert one() == -5 and batch() == -5 and plan() == -5
    assert one(mask=some, rot=some) == -5 and batch(mask=some, rot=some) == -5 and plan(mask=some, rot=some) == -5
    # a mask with a short row_cap: the context check comes first for the device-pointer call (the order of vis_homography_batch)
    assert batch(mask=some, cap=48) == -5
    # NULL pointers -> VIS_E_INVALID
    assert one(hq_=None) == -1 and one(h=None) == -1 and one(p1=None) == -1 and one(p2=None) == -1 and one(o=None) == -1
    assert batch(hq_=None) == -1 and batch(h=None) == -1 and batch(p1=None) == -1 and batch(p2=None) == -1 and batch(npts=None) == -1 and batch(o=None) == -1
    assert plan(hq_=None) == -1 and plan(h=None) == -1 and plan(o=None) == -1
    # misaligned pointers (8 bytes for records and points)
    assert batch(h=odd) == -1 and batch(p1=odd) == -1 and batch(p2=odd) == -1 and batch(o=odd) == -1 and plan(h=odd) == -1 and plan(o=odd) == -1
    odd4 = C.c_void_p(66)
    assert batch(npts=odd4) == -1 and batch(rot=odd4) == -1 and plan(rot=odd4) == -1     # 4 bytes for d_npts and d_rot
    assert batch(npts=odd, rot=odd) == -5 and plan(rot=odd) == -5
    assert one(h=odd4, p1=odd4, p2=odd4, rot=odd4) == -5              # host pointers are copied: no alignment asked
    # negative sizes
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1 and plan(n=-1) == -1 and plan(cap=-1) == -1
    # every parameter, on every call
    nan, inf = float("nan"), float("inf")
    bad = [("min_t_over_d", -1e-9), ("min_t_over_d", nan), ("min_t_over_d", inf), ("min_t_over_d", -inf), ("min_good", 0), ("min_good", -8)]
    for f in ("max_cos_parallax", "ambiguity_ratio", "good_share", "parallax_share"):
        bad += [(f, 0.0), (f, -0.5), (f, 1.0 + 1e-9), (f, 2.0), (f, nan), (f, inf), (f, -inf)]
    for f, v in bad:
        q = vislam.default_hpose_params()
        setattr(q, f, v)
        assert one(hq_=C.byref(q)) == -1 and batch(hq_=C.byref(q)) == -1 and plan(hq_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed
    for f, v in (("min_t_over_d", 0.0), ("min_t_over_d", 1e300), ("min_good", 1), ("max_cos_parallax", 1.0), ("max_cos_parallax", 1e-300),
                 ("ambiguity_ratio", 1.0), ("good_share", 1.0), ("parallax_share", 1.0), ("parallax_share", 1e-9)):
        q = vislam.default_hpose_params()
        setattr(q, f, v)
        assert one(hq_=C.byref(q)) == -5 and batch(hq_=C.byref(q)) == -5 and plan(hq_=C.byref(q)) == -5, (f, v)
    assert one(m=0, p1=None, p2=None) == -5                        # no points: no rows needed
    assert batch(mx=0, p1=None, p2=None) == -5
    assert int(rec["solution"][0]) == 7 and not rec["R"].any()     # a refused call writes nothing
