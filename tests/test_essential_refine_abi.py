"""CPU: the essential-batch and two-view refinement entry points' place in the C ABI -- vis_eref_params (16 bytes) and vis_eref_result (216 bytes)
in the C compiler's layout and in the ctypes / numpy bindings, the defaults, the flags, the five symbols exported and listed, and every refusal
that needs no device, in the header's order, for all four calls; VIS_ABI_VERSION, vis_params and vis_pose_result unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import essential_refine_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_essential_batch", "vis_default_eref_params", "vis_essential_refine", "vis_essential_refine_batch", "vis_batch_essential_refine")
P_FIELDS = ("refine_iters", "min_inliers", "threshold_px")
R_FIELDS = ("R", "t", "E", "cost0", "cost1", "n_used", "n_points", "n_inliers0", "n_inliers_refined", "best_step", "steps_run", "flags", "reserved_")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_eref_params, f)
#define R(f) (int)offsetof(vis_eref_result, f)
#define Q(f) (int)offsetof(vis_pose_result, f)
int main(void) {
    printf("%d %d %d %d\n", (int)sizeof(vis_eref_params), P(refine_iters), P(min_inliers), P(threshold_px));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_eref_result), R(R), R(t), R(E), R(cost0), R(cost1), R(n_used), R(n_points),
           R(n_inliers0), R(n_inliers_refined), R(best_step), R(steps_run), R(flags), R(reserved_));
    printf("%d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_ER_REFINED, (int)VIS_ER_REJECTED, (int)VIS_ER_FEW, (int)VIS_ER_NO_POSE);
    printf("%d %d %d %d\n", (int)sizeof(vis_pose_result), Q(E), Q(R), Q(t));
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
    assert rows[0] == [16, 0, 4, 8]
    assert rows[1] == [216, 0, 72, 96, 168, 176, 184, 188, 192, 196, 200, 204, 208, 212]
    for S in (vislam.EssentialRefineParams, er.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    S = vislam.EssentialRefineResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == rows[1]
    for d in (vislam.EREF_RESULT_DTYPE, er.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == rows[1]
    assert rows[1][0] % 8 == 0                                     # records in an array stay 8-byte aligned
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2:] == [vislam.ER_REFINED, vislam.ER_REJECTED, vislam.ER_FEW, vislam.ER_NO_POSE] == [er.REFINED, er.REJECTED, er.FEW, er.NO_POSE] == [1, 2, 4, 8]
    # the record the refinement starts from: vis_essential_batch writes it, vis_essential_refine_batch reads R and t at these offsets
    assert rows[3] == [192, 0, 72, 144] == [vislam.POSE_RESULT_DTYPE.itemsize] + [vislam.POSE_RESULT_DTYPE.fields[k][1] for k in ("E", "R", "t")]


def test_defaults(vislam):
    ep = vislam.default_eref_params()
    want = er.default_params()
    assert [getattr(ep, f) for f in P_FIELDS] == [getattr(want, f) for f in P_FIELDS] == [5, 8, 1.0]
    vislam.lib.vis_default_eref_params(None)                       # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("essential_batch", "essential_refine", "essential_refine_batch", "batch_essential_refine"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd8, odd4 = C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)   # never dereferenced: the argument / context checks come first
    ep = vislam.default_eref_params()
    ok = C.byref(ep)
    rec = np.zeros(1, vislam.EREF_RESULT_DTYPE)
    rec["best_step"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    ess = lambda n=1, p1=some, p2=some, npts=some, mx=49, cap=49, mask=None, o=some: L.vis_essential_batch(None, n, p1, p2, npts, mx, cap, mask, o)
    one = lambda ep_=ok, R=some, t=some, p1=some, p2=some, m=8, mask=None, o=out: L.vis_essential_refine(None, ep_, R, t, p1, p2, m, mask, o)
    batch = lambda ep_=ok, n=1, pose=some, p1=some, p2=some, npts=some, mx=49, cap=49, mask=None, o=some: \
        L.vis_essential_refine_batch(None, ep_, n, pose, p1, p2, npts, mx, cap, mask, o)
    plan = lambda ep_=ok, n=1, o=some: L.vis_batch_essential_refine(None, ep_, n, o)
    # valid arguments, no context -> VIS_E_STATE
    assert ess() == -5 and ess(mask=some) == -5 and one() == -5 and one(mask=some) == -5 and batch() == -5 and batch(mask=some) == -5 and plan() == -5
    # what would be VIS_E_CAPACITY with a context: the context check comes first (the order of vis_homography_batch)
    assert ess(mask=some, cap=48) == -5 and ess(mx=8193) == -5 and batch(mask=some, cap=48) == -5
    # NULL pointers -> VIS_E_INVALID
    assert ess(p1=None) == -1 and ess(p2=None) == -1 and ess(npts=None) == -1 and ess(o=None) == -1
    assert one(ep_=None) == -1 and one(R=None) == -1 and one(t=None) == -1 and one(p1=None) == -1 and one(p2=None) == -1 and one(o=None) == -1
    assert batch(ep_=None) == -1 and batch(pose=None) == -1 and batch(p1=None) == -1 and batch(p2=None) == -1 and batch(npts=None) == -1 and batch(o=None) == -1
    assert plan(ep_=None) == -1 and plan(o=None) == -1
    # misaligned device pointers (8 bytes for points and records, 4 for counts)
    assert ess(p1=odd8) == -1 and ess(p2=odd8) == -1 and ess(o=odd8) == -1 and ess(npts=odd4) == -1
    assert batch(pose=odd8) == -1 and batch(p1=odd8) == -1 and batch(p2=odd8) == -1 and batch(o=odd8) == -1 and batch(npts=odd4) == -1
    assert plan(o=odd8) == -1
    # negative sizes
    assert ess(n=-1) == -1 and ess(mx=-1) == -1 and ess(cap=-1) == -1
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1 and plan(n=-1) == -1
    # every parameter, on the three calls that take them
    nan, inf = float("nan"), float("inf")
    bad = [("refine_iters", -1), ("refine_iters", 65), ("min_inliers", 5), ("min_inliers", -8)] + [("threshold_px", v) for v in (0.0, -1.0, nan, inf, -inf)]
    for f, v in bad:
        q = vislam.default_eref_params()
        setattr(q, f, v)
        assert one(ep_=C.byref(q)) == -1 and batch(ep_=C.byref(q)) == -1 and plan(ep_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed
    for f, v in (("refine_iters", 0), ("refine_iters", 64), ("min_inliers", 6), ("threshold_px", 1e-300), ("threshold_px", 1e300)):
        q = vislam.default_eref_params()
        setattr(q, f, v)
        assert one(ep_=C.byref(q)) == -5 and batch(ep_=C.byref(q)) == -5 and plan(ep_=C.byref(q)) == -5, (f, v)
    assert one(m=0, p1=None, p2=None) == -5 and ess(mx=0, p1=None, p2=None) == -5 and batch(mx=0, p1=None, p2=None) == -5      # no points: no rows needed
    assert ess(n=0) == -5 and batch(n=0) == -5 and plan(n=0) == -5
    assert int(rec["best_step"][0]) == 7 and not rec["R"].any()    # a refused call writes nothing
