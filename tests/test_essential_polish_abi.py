"""CPU: the two-view polish's place in the C ABI -- vis_epolish_params (32 bytes) and vis_epolish_result (224 bytes) in the C compiler's layout and
in the ctypes / numpy bindings, the defaults, the flags, the five symbols exported and listed, and every refusal that needs no device, in the
header's order, for all four calls; a refused call writes nothing; VIS_ABI_VERSION, vis_params and vis_pose_result unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import essential_polish_ref as epr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_epolish_params", "vis_essential_polish", "vis_essential_polish_batch", "vis_batch_essential_polish", "vis_batch_triangulate_from")
P_FIELDS = ("rounds", "refine_iters", "min_inliers", "reserved_", "select_px", "reserved2_")
R_FIELDS = ("R", "t", "E", "cost_first", "cost0", "cost1", "n_points", "n_set_first", "n_set_last", "n_changed", "rounds_run", "steps_run", "best_step",
            "flags")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_epolish_params, f)
#define R(f) (int)offsetof(vis_epolish_result, f)
#define Q(f) (int)offsetof(vis_pose_result, f)
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_epolish_params), P(rounds), P(refine_iters), P(min_inliers), P(reserved_), P(select_px), P(reserved2_));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_epolish_result), R(R), R(t), R(E), R(cost_first), R(cost0), R(cost1),
           R(n_points), R(n_set_first), R(n_set_last), R(n_changed), R(rounds_run), R(steps_run), R(best_step), R(flags));
    printf("%d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_EP_POLISHED, (int)VIS_EP_REJECTED, (int)VIS_EP_FEW,
           (int)VIS_EP_NO_POSE, (int)VIS_EP_SHRANK);
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_pose_result), Q(E), Q(R), Q(t), Q(n_inliers), Q(n_points));
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
    assert rows[0] == [32, 0, 4, 8, 12, 16, 24]
    assert rows[1] == [224, 0, 72, 96, 168, 176, 184, 192, 196, 200, 204, 208, 212, 216, 220]
    for S in (vislam.EssentialPolishParams, epr.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    S = vislam.EssentialPolishResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == rows[1]
    for d in (vislam.EPOLISH_RESULT_DTYPE, epr.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == rows[1]
    # no implicit padding: the fields fill the records
    assert sum(C.sizeof(t) for _, t in vislam.EssentialPolishParams._fields_) == 32 and sum(C.sizeof(t) for _, t in S._fields_) == 224
    assert rows[1][0] % 8 == 0                                     # records in an array stay 8-byte aligned
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2:] == [vislam.EP_POLISHED, vislam.EP_REJECTED, vislam.EP_FEW, vislam.EP_NO_POSE, vislam.EP_SHRANK] == \
        [epr.POLISHED, epr.REJECTED, epr.FEW, epr.NO_POSE, epr.SHRANK] == [1, 2, 4, 8, 16]
    # the record the polish starts from and writes
    for d in (vislam.POSE_RESULT_DTYPE, epr.POSE_DTYPE):
        assert rows[3] == [192, 0, 72, 144, 168, 180] == [d.itemsize] + [d.fields[k][1] for k in ("E", "R", "t", "n_inliers", "n_points")]


def test_defaults(vislam):
    ep = vislam.default_epolish_params()
    want = epr.default_params()
    assert [getattr(ep, f) for f in P_FIELDS[:5]] == [getattr(want, f) for f in P_FIELDS[:5]] == [3, 5, 8, 0, 2.0]
    assert list(ep.reserved2_) == list(want.reserved2_) == [0, 0]
    junk = vislam.EssentialPolishParams(-1, -1, -1, -1, -1.0, (C.c_int32 * 2)(-1, -1))
    vislam.lib.vis_default_epolish_params(C.byref(junk))           # every byte is set, the reserved ones to 0
    assert bytes(junk) == bytes(ep)
    vislam.lib.vis_default_epolish_params(None)                    # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("essential_polish", "essential_polish_batch", "batch_essential_polish", "batch_triangulate_from"):
        assert callable(getattr(vislam.Context, name)), name
    hdr = open(os.path.join(ROOT, "include", "vislam_hip.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr, s


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd8, odd4 = C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)   # never dereferenced: the argument / context checks come first
    far = C.c_void_p(1 << 20)
    ep = vislam.default_epolish_params()
    ok = C.byref(ep)
    rec = np.zeros(1, vislam.EPOLISH_RESULT_DTYPE)
    rec["best_step"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    mo = np.full(8, 0xEE, np.uint8)
    po = np.zeros(1, vislam.POSE_RESULT_DTYPE)
    po["n_models"] = 9
    tp = vislam.default_tri_params()
    one = lambda ep_=ok, R=some, t=some, p1=some, p2=some, m=8, mask=None, o=out, mk=mo.ctypes.data_as(C.c_void_p), q=po.ctypes.data_as(C.c_void_p): \
        L.vis_essential_polish(None, ep_, R, t, p1, p2, m, mask, o, mk, q)
    batch = lambda ep_=ok, n=1, pose=some, p1=some, p2=some, npts=some, mx=49, cap=49, mask=None, mk=far, o=some, q=None: \
        L.vis_essential_polish_batch(None, ep_, n, pose, p1, p2, npts, mx, cap, mask, mk, o, q)
    plan = lambda ep_=ok, n=1, cap=49, mk=some, o=some, q=None: L.vis_batch_essential_polish(None, ep_, n, cap, mk, o, q)
    tri = lambda tp_=C.byref(tp), n=1, pose=some, mcap=49, mask=None, cap=49, pts=some, fl=some, sm=some: \
        L.vis_batch_triangulate_from(None, tp_, n, pose, mcap, mask, cap, pts, fl, sm)
    # valid arguments, no context -> VIS_E_STATE
    assert one() == -5 and one(mask=some) == -5 and one(q=None) == -5 and batch() == -5 and batch(mask=some) == -5 and batch(q=far) == -5
    assert plan() == -5 and plan(q=some) == -5 and tri() == -5 and tri(mask=some) == -5
    # what would be VIS_E_CAPACITY with a context: the context check comes first
    assert batch(cap=48) == -5 and tri(mask=some, mcap=48) == -5 and tri(cap=1) == -5
    # NULL pointers -> VIS_E_INVALID
    assert one(ep_=None) == -1 and one(R=None) == -1 and one(t=None) == -1 and one(p1=None) == -1 and one(p2=None) == -1 and one(o=None) == -1 and one(mk=None) == -1
    assert batch(ep_=None) == -1 and batch(pose=None) == -1 and batch(p1=None) == -1 and batch(p2=None) == -1 and batch(npts=None) == -1
    assert batch(o=None) == -1 and batch(mk=None) == -1
    assert plan(ep_=None) == -1 and plan(o=None) == -1 and plan(mk=None) == -1
    assert tri(tp_=None) == -1 and tri(pose=None) == -1 and tri(pts=None) == -1 and tri(fl=None) == -1 and tri(sm=None) == -1
    # misaligned device pointers (8 bytes for points and records, 4 for counts; 16 for map points)
    assert batch(pose=odd8) == -1 and batch(p1=odd8) == -1 and batch(p2=odd8) == -1 and batch(o=odd8) == -1 and batch(q=odd8) == -1 and batch(npts=odd4) == -1
    assert plan(o=odd8) == -1 and plan(q=odd8) == -1
    assert tri(pose=odd8) == -1 and tri(pts=C.c_void_p(72)) == -1 and tri(sm=odd4) == -1
    # negative sizes
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1 and plan(n=-1) == -1 and plan(cap=-1) == -1 and tri(mcap=-1) == -1
    # overlapping input and output: the mask rows (n x row_cap bytes each), the pose records
    assert batch(mask=some, mk=some) == -1 and batch(mask=some, mk=C.c_void_p(64 + 48)) == -1 and batch(mask=some, mk=C.c_void_p(64 + 49)) == -5
    assert batch(mask=C.c_void_p(64 + 48), mk=some) == -1
    assert batch(q=some) == -1 and batch(q=C.c_void_p(64 + 184)) == -1 and batch(q=C.c_void_p(64 + 192)) == -5
    # every parameter, on the three calls that take them
    nan, inf = float("nan"), float("inf")
    bad = [("rounds", -1), ("rounds", 9), ("refine_iters", 0), ("refine_iters", -1), ("refine_iters", 65), ("min_inliers", 5), ("min_inliers", -8),
           ("reserved_", 1)] + [("select_px", v) for v in (0.0, -1.0, nan, inf, -inf)]
    for f, v in bad:
        q = vislam.default_epolish_params()
        setattr(q, f, v)
        assert one(ep_=C.byref(q)) == -1 and batch(ep_=C.byref(q)) == -1 and plan(ep_=C.byref(q)) == -1, (f, v)
    for k in (0, 1):
        q = vislam.default_epolish_params()
        q.reserved2_[k] = 1
        assert one(ep_=C.byref(q)) == -1 and batch(ep_=C.byref(q)) == -1 and plan(ep_=C.byref(q)) == -1, k
    # the edges that are allowed
    for f, v in (("rounds", 0), ("rounds", 8), ("refine_iters", 1), ("refine_iters", 64), ("min_inliers", 6), ("select_px", 1e-300), ("select_px", 1e300)):
        q = vislam.default_epolish_params()
        setattr(q, f, v)
        assert one(ep_=C.byref(q)) == -5 and batch(ep_=C.byref(q)) == -5 and plan(ep_=C.byref(q)) == -5, (f, v)
    assert one(m=0, p1=None, p2=None, mk=None) == -5 and batch(mx=0, p1=None, p2=None) == -5      # no points: no rows needed
    assert batch(n=0) == -5 and plan(n=0) == -5 and tri(n=0) == -5
    # a refused call writes nothing
    assert int(rec["best_step"][0]) == 7 and not rec["R"].any() and (mo == 0xEE).all() and int(po["n_models"][0]) == 9 and not po["R"].any()
