"""CPU: the homography polish's place in the C ABI -- vis_hpolish_params (32 bytes) and vis_hpolish_result (128 bytes) in the C compiler's layout
and in the ctypes / numpy bindings, the defaults, the flags, the four symbols exported and listed, and every refusal that needs no device, in the
header's order, for all three calls; a refused call writes nothing; VIS_ABI_VERSION, vis_params and vis_homography_result unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import homography_polish_ref as hq
import homography_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_hpolish_params", "vis_homography_polish", "vis_homography_polish_batch", "vis_batch_homography_polish")
P_FIELDS = ("rounds", "refine_iters", "min_inliers", "reserved_", "select_chi2", "sigma_px")
R_FIELDS = ("H", "cost_first", "cost0", "cost1", "n_points", "n_set_first", "n_set_last", "n_changed", "rounds_run", "steps_run", "best_step", "flags")
H_FIELDS = ("H", "score_h", "score_e", "n_inliers", "n_points", "best_iter", "n_degenerate", "n_inliers_e", "model")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_hpolish_params, f)
#define R(f) (int)offsetof(vis_hpolish_result, f)
#define Q(f) (int)offsetof(vis_homography_result, f)
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_hpolish_params), P(rounds), P(refine_iters), P(min_inliers), P(reserved_), P(select_chi2), P(sigma_px));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_hpolish_result), R(H), R(cost_first), R(cost0), R(cost1), R(n_points),
           R(n_set_first), R(n_set_last), R(n_changed), R(rounds_run), R(steps_run), R(best_step), R(flags));
    printf("%d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_HPOL_POLISHED, (int)VIS_HPOL_REJECTED, (int)VIS_HPOL_FEW,
           (int)VIS_HPOL_NO_MODEL, (int)VIS_HPOL_SHRANK);
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_homography_result), Q(H), Q(score_h), Q(score_e), Q(n_inliers), Q(n_points), Q(best_iter),
           Q(n_degenerate), Q(n_inliers_e), Q(model));
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
    assert rows[1] == [128, 0, 72, 80, 88, 96, 100, 104, 108, 112, 116, 120, 124]
    for S in (vislam.HomographyPolishParams, hq.Params):
        assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    S = vislam.HomographyPolishResult
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in R_FIELDS] == rows[1]
    for d in (vislam.HPOLISH_RESULT_DTYPE, hq.RESULT_DTYPE):
        assert [d.itemsize] + [d.fields[k][1] for k in R_FIELDS] == rows[1]
    # no implicit padding: the fields fill the records
    assert sum(C.sizeof(t) for _, t in vislam.HomographyPolishParams._fields_) == 32 and sum(C.sizeof(t) for _, t in S._fields_) == 128
    assert rows[1][0] % 8 == 0                                     # records in an array stay 8-byte aligned
    assert rows[2][0] == 5                                         # VIS_ABI_VERSION: only new symbols and two new structs
    assert rows[2][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[2][2:] == [vislam.HPOL_POLISHED, vislam.HPOL_REJECTED, vislam.HPOL_FEW, vislam.HPOL_NO_MODEL, vislam.HPOL_SHRANK] == \
        [hq.POLISHED, hq.REJECTED, hq.FEW, hq.NO_MODEL, hq.SHRANK] == [1, 2, 4, 8, 16]
    # the record the polish starts from and writes
    for d in (vislam.HOMOGRAPHY_RESULT_DTYPE, hr.RESULT_DTYPE):
        assert rows[3] == [112, 0, 72, 80, 88, 92, 96, 100, 104, 108] == [d.itemsize] + [d.fields[k][1] for k in H_FIELDS]


def test_defaults(vislam):
    hp = vislam.default_hpolish_params()
    want = hq.default_params()
    assert [getattr(hp, f) for f in P_FIELDS] == [getattr(want, f) for f in P_FIELDS] == [3, 5, 8, 0, 5.991, 1.0]
    dflt = vislam.default_homography_params()                      # with the defaults the re-selection's threshold is the RANSAC's t_h
    assert hp.select_chi2 == dflt.chi2_h and hp.sigma_px == dflt.sigma_px and hq.t_sel(hr.Camera(), want) == hr.thresholds(hr.Camera(), hr.default_params())[2]
    junk = vislam.HomographyPolishParams(-1, -1, -1, -1, -1.0, -1.0)
    vislam.lib.vis_default_hpolish_params(C.byref(junk))           # every byte is set, the reserved ones to 0
    assert bytes(junk) == bytes(hp)
    vislam.lib.vis_default_hpolish_params(None)                    # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("homography_polish", "homography_polish_batch", "batch_homography_polish"):
        assert callable(getattr(vislam.Context, name)), name
    hdr = open(os.path.join(ROOT, "include", "vislam_hip.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr, s
    assert "a refit is not built" not in hdr


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some, odd8, odd4 = C.c_void_p(64), C.c_void_p(68), C.c_void_p(66)   # never dereferenced: the argument / context checks come first
    far = C.c_void_p(1 << 20)
    hp = vislam.default_hpolish_params()
    ok = C.byref(hp)
    rec = np.zeros(1, vislam.HPOLISH_RESULT_DTYPE)
    rec["best_step"] = 7
    out = rec.ctypes.data_as(C.c_void_p)
    mo = np.full(8, 0xEE, np.uint8)
    ho = np.zeros(1, vislam.HOMOGRAPHY_RESULT_DTYPE)
    ho["n_degenerate"] = 9
    one = lambda hp_=ok, h=some, p1=some, p2=some, m=8, mask=None, o=out, mk=mo.ctypes.data_as(C.c_void_p), q=ho.ctypes.data_as(C.c_void_p): \
        L.vis_homography_polish(None, hp_, h, p1, p2, m, mask, o, mk, q)
    batch = lambda hp_=ok, n=1, h=some, p1=some, p2=some, npts=some, mx=49, cap=49, mask=None, mk=far, o=some, q=None: \
        L.vis_homography_polish_batch(None, hp_, n, h, p1, p2, npts, mx, cap, mask, mk, o, q)
    plan = lambda hp_=ok, n=1, h=some, mcap=49, mask=None, cap=49, mk=far, o=some, q=None: L.vis_batch_homography_polish(None, hp_, n, h, mcap, mask, cap, mk, o, q)
    # valid arguments, no context -> VIS_E_STATE
    assert one() == -5 and one(mask=some) == -5 and one(q=None) == -5 and batch() == -5 and batch(mask=some) == -5 and batch(q=far) == -5
    assert plan() == -5 and plan(mask=some) == -5 and plan(q=far) == -5
    # what would be VIS_E_CAPACITY with a context: the context check comes first
    assert batch(cap=48) == -5 and plan(cap=1) == -5 and plan(mask=some, mcap=1) == -5
    # NULL pointers -> VIS_E_INVALID
    assert one(hp_=None) == -1 and one(h=None) == -1 and one(p1=None) == -1 and one(p2=None) == -1 and one(o=None) == -1 and one(mk=None) == -1
    assert batch(hp_=None) == -1 and batch(h=None) == -1 and batch(p1=None) == -1 and batch(p2=None) == -1 and batch(npts=None) == -1
    assert batch(o=None) == -1 and batch(mk=None) == -1
    assert plan(hp_=None) == -1 and plan(h=None) == -1 and plan(o=None) == -1 and plan(mk=None) == -1
    # misaligned device pointers (8 bytes for points and records, 4 for counts)
    assert batch(h=odd8) == -1 and batch(p1=odd8) == -1 and batch(p2=odd8) == -1 and batch(o=odd8) == -1 and batch(q=odd8) == -1 and batch(npts=odd4) == -1
    assert plan(h=odd8) == -1 and plan(o=odd8) == -1 and plan(q=odd8) == -1
    # negative sizes
    assert one(m=-1) == -1 and batch(n=-1) == -1 and batch(mx=-1) == -1 and batch(cap=-1) == -1
    assert plan(n=-1) == -1 and plan(cap=-1) == -1 and plan(mcap=-1) == -1
    # overlapping input and output: the mask rows (n x row_cap bytes each), the homography records (112 bytes)
    assert batch(mask=some, mk=some) == -1 and batch(mask=some, mk=C.c_void_p(64 + 48)) == -1 and batch(mask=some, mk=C.c_void_p(64 + 49)) == -5
    assert batch(mask=C.c_void_p(64 + 48), mk=some) == -1
    assert batch(q=some) == -1 and batch(q=C.c_void_p(64 + 104)) == -1 and batch(q=C.c_void_p(64 + 112)) == -5
    assert plan(mask=some, mk=some) == -1 and plan(mask=some, mcap=52, mk=C.c_void_p(64 + 48)) == -1 and plan(mask=some, mcap=52, mk=C.c_void_p(64 + 52)) == -5
    assert plan(mask=C.c_void_p(64 + 48), mk=some) == -1 and plan(q=some) == -1 and plan(q=C.c_void_p(64 + 104)) == -1 and plan(q=C.c_void_p(64 + 112)) == -5
    # every parameter, on the three calls
    nan, inf = float("nan"), float("inf")
    bad = [("rounds", -1), ("rounds", 9), ("refine_iters", 0), ("refine_iters", -1), ("refine_iters", 65), ("min_inliers", 4), ("min_inliers", -8),
           ("reserved_", 1)] + [(f, v) for f in ("select_chi2", "sigma_px") for v in (0.0, -1.0, nan, inf, -inf)]
    for f, v in bad:
        q = vislam.default_hpolish_params()
        setattr(q, f, v)
        assert one(hp_=C.byref(q)) == -1 and batch(hp_=C.byref(q)) == -1 and plan(hp_=C.byref(q)) == -1, (f, v)
    # the edges that are allowed
    for f, v in (("rounds", 0), ("rounds", 8), ("refine_iters", 1), ("refine_iters", 64), ("min_inliers", 5), ("select_chi2", 1e-300), ("select_chi2", 1e300),
                 ("sigma_px", 1e-300), ("sigma_px", 1e300)):
        q = vislam.default_hpolish_params()
        setattr(q, f, v)
        assert one(hp_=C.byref(q)) == -5 and batch(hp_=C.byref(q)) == -5 and plan(hp_=C.byref(q)) == -5, (f, v)
    assert one(m=0, p1=None, p2=None, mk=None) == -5 and batch(mx=0, p1=None, p2=None) == -5      # no points: no rows needed
    assert batch(n=0) == -5 and plan(n=0) == -5
    # VIS_E_INVALID comes before VIS_E_STATE: a bad argument beside the missing context
    q = vislam.default_hpolish_params()
    q.rounds = 9
    assert one(hp_=C.byref(q), m=-1) == -1 and batch(hp_=C.byref(q), cap=48) == -1 and plan(hp_=C.byref(q), cap=1) == -1
    # a refused call writes nothing
    assert int(rec["best_step"][0]) == 7 and not rec["H"].any() and (mo == 0xEE).all() and int(ho["n_degenerate"][0]) == 9 and not ho["H"].any()
