"""CPU: the PnP entry points' place in the C ABI -- vis_pnp_params (24 bytes) and vis_pnp_result (240 bytes) in the C compiler's layout and in
the ctypes / numpy bindings, the defaults, VIS_PNP_TILE and the flags, the four symbols exported and listed, and every refusal that needs
no device, in the header's order; VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_pnp_params", "vis_pnp_ransac", "vis_pnp_batch", "vis_batch_pnp")
L_FIELDS = ("R_rel", "t_rel", "scale", "n_linked", "q", "p", "flags")
P_FIELDS = ("iters", "min_inliers", "threshold_px", "refine_iters", "reserved_")
R_FIELDS = ("R", "t", "R_ransac", "t_ransac", "cost0", "cost1", "n_inliers", "n_points", "best_iter", "best_root", "n_degenerate", "n_solutions",
            "n_inliers_refined", "flags")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_pnp_params, f)
#define R(f) (int)offsetof(vis_pnp_result, f)
#define L(f) (int)offsetof(vis_pnp_link, f)
int main(void) {
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_pnp_params), P(iters), P(min_inliers), P(threshold_px), P(refine_iters), P(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_pnp_result), R(R), R(t), R(R_ransac), R(t_ransac), R(cost0), R(cost1),
           R(n_inliers), R(n_points), R(best_iter), R(best_root), R(n_degenerate), R(n_solutions), R(n_inliers_refined), R(flags));
    printf("%d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_PNP_TILE, (int)VIS_PNP_REFINED, (int)VIS_PNP_REFINE_REJECTED,
           (int)VIS_PNP_FEW);
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_pnp_link), L(R_rel), L(t_rel), L(scale), L(n_linked), L(q), L(p), L(flags), (int)VIS_PNPL_NO_MAP);
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
    assert rows[0] == [24, 0, 4, 8, 16, 20]
    assert rows[1] == [240, 0, 72, 96, 168, 192, 200, 208, 212, 216, 220, 224, 228, 232, 236]
    for S in (vislam.PnpParams, pr.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    S = vislam.PnpResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == rows[1]
    for d in (vislam.PNP_RESULT_DTYPE, pr.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == rows[1]
    assert rows[3] == [120, 0, 72, 96, 104, 108, 112, 116, 1] and vislam.PNPL_NO_MAP == pr.NO_MAP == 1
    assert [C.sizeof(vislam.PnpLink)] + [getattr(vislam.PnpLink, f).offset for f in L_FIELDS] == rows[3][:-1]
    for d in (vislam.PNP_LINK_DTYPE, pr.LINK_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in L_FIELDS] == rows[3][:-1]
    assert rows[1][0] % 8 == 0 and rows[3][0] % 8 == 0                                     # records in an array stay 8-byte aligned
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2] == vislam.PNP_TILE == 512
    assert rows[2][3:] == [vislam.PNP_REFINED, vislam.PNP_REFINE_REJECTED, vislam.PNP_FEW] == [pr.REFINED, pr.REFINE_REJECTED, pr.FEW] == [1, 2, 4]


def test_defaults(vislam):
    pp = vislam.default_pnp_params()
    want = pr.default_params()
    assert [getattr(pp, f) for f in P_FIELDS] == [getattr(want, f) for f in P_FIELDS] == [200, 8, 2.0, 5, 0]
    vislam.lib.vis_default_pnp_params(None)                        # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("pnp_ransac", "pnp_batch", "batch_pnp"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd8, odd4 = C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)   # never dereferenced: the argument / context checks come first
    pp = vislam.default_pnp_params()
    ok = C.byref(pp)
    rec = np.full(1, 0, vislam.PNP_RESULT_DTYPE)
    rec["best_iter"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    one = lambda pp_=ok, X=some, xy=some, m=4, dr=some, mask=None, o=out: L.vis_pnp_ransac(None, pp_, X, xy, m, dr, mask, o)
    batch = lambda pp_=ok, n=1, X=some, xs=3, xy=some, npts=some, mx=49, dr=some, cap=49, mask=None, o=some: \
        L.vis_pnp_batch(None, pp_, n, X, xs, xy, npts, mx, dr, cap, mask, o)
    pts16 = C.c_void_p(80)
    plan = lambda pp_=ok, n=1, dr=some, pts=pts16, fl=some, cap=49, req=16, mcap=0, mask=None, o=some, l=some: \
        L.vis_batch_pnp(None, pp_, n, dr, pts, fl, cap, req, mcap, mask, o, l)
    assert plan() == -5 and plan(mask=some, mcap=49) == -5 and plan(req=0) == -5 and plan(req=255) == -5
    assert plan(pp_=None) == -1 and plan(dr=None) == -1 and plan(pts=None) == -1 and plan(fl=None) == -1 and plan(o=None) == -1 and plan(l=None) == -1
    assert plan(pts=C.c_void_p(72)) == -1 and plan(o=odd8) == -1 and plan(l=odd8) == -1 and plan(dr=odd4) == -1
    assert plan(n=-1) == -1 and plan(cap=-1) == -1 and plan(mcap=-1) == -1 and plan(req=-1) == -1 and plan(req=256) == -1
    # valid arguments, no context -> VIS_E_STATE
    assert one() == -5 and batch() == -5 and batch(xs=4) == -5 and batch(mask=some) == -5
    # a mask with a short row_cap: the context check comes first (the order of vis_homography_batch)
    assert batch(mask=some, cap=48) == -5
    # NULL pointers -> VIS_E_INVALID
    assert one(pp_=None) == -1 and one(X=None) == -1 and one(xy=None) == -1 and one(dr=None) == -1 and one(o=None) == -1
    assert batch(pp_=None) == -1 and batch(X=None) == -1 and batch(xy=None) == -1 and batch(npts=None) == -1 and batch(dr=None) == -1 and batch(o=None) == -1
    # misaligned device pointers (8 bytes for points, pixels and records, 4 for counts and draws)
    assert batch(X=odd8) == -1 and batch(xy=odd8) == -1 and batch(o=odd8) == -1 and batch(npts=odd4) == -1 and batch(dr=odd4) == -1
    # negative sizes, a point stride below three doubles
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1 and batch(xs=2) == -1 and batch(xs=-3) == -1
    # every parameter, on both calls
    nan, inf = float("nan"), float("inf")
    bad = [("iters", -1), ("iters", (1 << 29) + 1), ("min_inliers", 3), ("min_inliers", -8), ("refine_iters", -1)]
    bad += [("threshold_px", v) for v in (0.0, -1.0, nan, inf, -inf)]
    for f, v in bad:
        q = vislam.default_pnp_params()
        setattr(q, f, v)
        assert one(pp_=C.byref(q)) == -1 and batch(pp_=C.byref(q)) == -1 and plan(pp_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed
    for f, v in (("iters", 0), ("iters", 1 << 29), ("min_inliers", 4), ("refine_iters", 0), ("threshold_px", 1e-300), ("threshold_px", 1e300)):
        q = vislam.default_pnp_params()
        setattr(q, f, v)
        assert one(pp_=C.byref(q)) == -5 and batch(pp_=C.byref(q)) == -5 and plan(pp_=C.byref(q)) == -5, (f, v)
    q = vislam.default_pnp_params()
    q.iters = 0
    assert one(pp_=C.byref(q), dr=None) == -5                      # no samples: no table needed
    assert one(m=0, X=None, xy=None, dr=None) == -5                # no points: no rows needed
    assert int(rec["best_iter"][0]) == 7 and not rec["R"].any()    # a refused call writes nothing
