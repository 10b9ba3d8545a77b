"""CPU: the KLT entry points' place in the C ABI -- vis_klt_params (56 bytes), vis_klt_point and vis_klt_pair (32 bytes each) in the C
compiler's layout and in the ctypes / numpy bindings, the defaults, the flags, the four symbols exported and listed, and every refusal that
needs no device, in the header's order; VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import klt_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_klt_params", "vis_klt_track", "vis_klt_batch", "vis_batch_klt")
PT_FIELDS = ("x", "y", "fb", "min_eig", "sad", "flags", "iters", "levels", "pad_")
PR_FIELDS = ("n_points", "n_tracked", "n_oob", "n_flat", "n_err", "n_fb", "n_invalid", "flags")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_klt_params, f)
#define T(f) (int)offsetof(vis_klt_point, f)
#define R(f) (int)offsetof(vis_klt_pair, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_klt_params), P(win_radius), P(first_level), P(last_level), P(max_iters), P(epsilon),
           P(min_eig), P(max_err), P(fb_max_px), P(scharr_scale), P(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_klt_point), T(x), T(y), T(fb), T(min_eig), T(sad), T(flags), T(iters), T(levels), T(pad_));
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_klt_pair), R(n_points), R(n_tracked), R(n_oob), R(n_flat), R(n_err), R(n_fb), R(n_invalid),
           R(flags));
    printf("%d %d %d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_KLT_TRACKED, (int)VIS_KLT_OOB, (int)VIS_KLT_FLAT,
           (int)VIS_KLT_ERR, (int)VIS_KLT_FB, (int)VIS_KLT_INVALID, (int)VIS_KLT_NO_PAIR);
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
    assert rows[0] == [56, 0, 4, 8, 12, 16, 24, 32, 40, 48, 52]
    assert rows[1] == [32, 0, 4, 8, 12, 16, 20, 24, 26, 27]
    assert rows[2] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    for S in (vislam.KltParams, kr.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in kr.P_FIELDS] == rows[0]
    for d in (vislam.KLT_POINT_DTYPE, kr.POINT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in PT_FIELDS] == rows[1]
    for d in (vislam.KLT_PAIR_DTYPE, kr.PAIR_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in PR_FIELDS] == rows[2]
    assert rows[3][0] == 5                                         # VIS_ABI_VERSION: only new symbols and three new structs
    assert rows[3][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[3][2:8] == [vislam.KLT_TRACKED, vislam.KLT_OOB, vislam.KLT_FLAT, vislam.KLT_ERR, vislam.KLT_FB, vislam.KLT_INVALID] \
        == [kr.TRACKED, kr.OOB, kr.FLAT, kr.ERR, kr.FB, kr.INVALID] == [1, 2, 4, 8, 16, 32]
    assert rows[3][8] == vislam.KLT_NO_PAIR == kr.NO_PAIR == 1


def test_defaults(vislam):
    kp = vislam.default_klt_params()
    want = kr.default_params()
    assert [getattr(kp, f) for f in kr.P_FIELDS] == [getattr(want, f) for f in kr.P_FIELDS] == [7, 3, 0, 10, 0.01, 0.1, 0.0, 0.0, 3, 0]
    vislam.lib.vis_default_klt_params(None)                        # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("klt_track", "klt_batch", "batch_klt", "keypoint_capacity"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd8, odd4 = C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)   # never dereferenced: the argument / context checks come first
    kp = vislam.default_klt_params()
    ok = C.byref(kp)
    lv = (C.c_void_p * 5)(*[64] * 5)
    top = (C.c_void_p * 5)(64, 64, 64, 64, None)                   # the default levels are 0 ... 3: level 4 may be NULL
    hole = (C.c_void_p * 5)(64, None, 64, 64, 64)
    rec = np.full(2, 0, vislam.KLT_POINT_DTYPE)
    rec["sad"] = 7
    pr = np.zeros(1, vislam.KLT_PAIR_DTYPE)
    pr["n_points"] = 9
    out, pair = rec.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p)
    one = lambda kp_=ok, w=160, h=120, g1=lv, x1=lv, y1=lv, g2=lv, x2=None, y2=None, pts=some, gs=None, m=2, o=out, p=pair: \
        L.vis_klt_track(None, kp_, w, h, g1, x1, y1, g2, x2, y2, pts, gs, m, o, p)
    batch = lambda kp_=ok, fr=some, w=160, h=120, st=160, n=2, gr=some, gx=some, gy=some, pts=some, npts=some, mx=8, gs=None, o=some, p=some, \
        p1=None, p2=None, nt=None: L.vis_klt_batch(None, kp_, fr, w, h, st, n, gr, gx, gy, pts, npts, mx, gs, o, p, p1, p2, nt)
    plan = lambda kp_=ok, fr=some, n=2, gs=None, cap=512, o=some, p=some, p1=None, p2=None, nt=None: \
        L.vis_batch_klt(None, kp_, fr, n, gs, cap, o, p, p1, p2, nt)
    # valid arguments, no context -> VIS_E_STATE
    assert one() == -5 and one(g1=top, x1=top, y1=top, g2=top) == -5 and one(gs=some) == -5 and one(m=0, pts=None, o=None) == -5
    assert batch() == -5 and batch(gs=some) == -5 and batch(p1=some, p2=some, nt=some) == -5 and batch(st=200) == -5 and batch(mx=0, pts=None, o=None) == -5
    assert batch(n=0) == -5 and batch(w=16, h=16, st=16) == -5 and batch(w=4095, h=4095, st=4095) == -5
    assert plan() == -5 and plan(gs=some) == -5 and plan(p1=some, p2=some, nt=some) == -5 and plan(cap=0) == -5
    # NULL pointers -> VIS_E_INVALID
    assert one(kp_=None) == -1 and one(g1=None) == -1 and one(x1=None) == -1 and one(y1=None) == -1 and one(g2=None) == -1
    assert one(pts=None) == -1 and one(o=None) == -1 and one(p=None) == -1
    assert one(g1=hole) == -1 and one(x1=hole) == -1 and one(y1=hole) == -1 and one(g2=hole) == -1     # a level inside [last, first]
    for name in ("kp_", "fr", "gr", "gx", "gy", "pts", "npts", "o", "p"):
        assert batch(**{name: None}) == -1, name
    assert plan(kp_=None) == -1 and plan(fr=None) == -1 and plan(o=None) == -1 and plan(p=None) == -1
    # the compacted rows: all three or none
    for call in (batch, plan):
        assert call(p1=some) == -1 and call(p2=some, nt=some) == -1 and call(p1=some, p2=some) == -1
    # forward-backward reads frame 2's gradients
    fbp = vislam.default_klt_params()
    fbp.fb_max_px = 1.0
    assert one(kp_=C.byref(fbp)) == -1 and one(kp_=C.byref(fbp), x2=lv) == -1 and one(kp_=C.byref(fbp), x2=lv, y2=hole) == -1
    assert one(kp_=C.byref(fbp), x2=lv, y2=top) == -5
    # misaligned device pointers (8 bytes for records, 4 for points, guesses and counts)
    assert batch(o=odd8) == -1 and batch(p=odd8) == -1 and batch(pts=odd4) == -1 and batch(gs=odd4) == -1 and batch(npts=odd4) == -1
    assert batch(p1=odd4, p2=some, nt=some) == -1 and batch(p1=some, p2=odd4, nt=some) == -1 and batch(p1=some, p2=some, nt=odd4) == -1
    assert plan(o=odd8) == -1 and plan(p=odd8) == -1 and plan(gs=odd4) == -1 and plan(p1=odd4, p2=some, nt=some) == -1
    # sizes
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and plan(n=-1) == -1 and plan(cap=-1) == -1
    for w, h, st in ((15, 120, 160), (160, 15, 160), (4096, 120, 4096), (160, 4096, 160), (160, 120, 159)):
        assert batch(w=w, h=h, st=st) == -1, (w, h, st)
    assert one(w=15) == -1 and one(h=4096) == -1
    # every parameter, on all three calls
    nan, inf = float("nan"), float("inf")
    bad = [("win_radius", 1), ("win_radius", 11), ("win_radius", -7), ("first_level", 5), ("last_level", -1), ("last_level", 4), ("max_iters", 0),
           ("max_iters", 31), ("scharr_scale", 0), ("scharr_scale", 9), ("reserved_", 1)]
    bad += [(f, v) for f in ("epsilon", "min_eig", "max_err", "fb_max_px") for v in (-1.0, nan, inf, -inf)]
    for f, v in bad:
        q = vislam.default_klt_params()
        setattr(q, f, v)
        assert one(kp_=C.byref(q), x2=lv, y2=lv) == -1 and batch(kp_=C.byref(q)) == -1 and plan(kp_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed (the plan's gradients are made with scale 3: vis_batch_klt takes no other)
    for f, v in (("win_radius", 2), ("win_radius", 10), ("first_level", 4), ("first_level", 0), ("max_iters", 1), ("max_iters", 30), ("epsilon", 0.0),
                 ("min_eig", 0.0), ("max_err", 1e300), ("fb_max_px", 1e-300), ("scharr_scale", 1), ("scharr_scale", 8)):
        q = vislam.default_klt_params()
        setattr(q, f, v)
        assert one(kp_=C.byref(q), x2=lv, y2=lv) == -5 and batch(kp_=C.byref(q)) == -5, (f, v)
        assert plan(kp_=C.byref(q)) == (-1 if f == "scharr_scale" else -5), (f, v)
    q = vislam.default_klt_params()
    q.first_level = q.last_level = 2
    only2 = (C.c_void_p * 5)(None, None, 64, None, None)
    assert one(kp_=C.byref(q), g1=only2, x1=only2, y1=only2, g2=only2) == -5
    assert (rec["sad"] == 7).all() and int(pr["n_points"][0]) == 9   # a refused call writes nothing
