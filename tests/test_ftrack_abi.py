"""CPU: the feature-track entry points' place in the C ABI -- vis_ftrack_obs (16 bytes), vis_ftrack_frame (32), vis_ftrack_point (40),
vis_ftrack_tri_summary (32) and vis_ftrack_tri_params (32) in the C compiler's layout and in the ctypes / numpy bindings and the restatement,
the enums and defaults, the five symbols exported and listed, and every refusal that needs no device, in the header's order;
VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np

import ftrack_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_ftrack_link_rows", "vis_batch_ftrack", "vis_default_ftrack_tri_params", "vis_ftrack_triangulate_rows", "vis_batch_ftrack_triangulate")
O_FIELDS = ("birth_seq", "birth_kp", "len", "prev_kp")
F_FIELDS = ("seq", "n_keypoints", "n_continued", "n_started", "n_ended", "max_len", "sum_len", "flags")
P_FIELDS = ("X", "rms_reproj_px", "parallax_cos", "n_views", "flags")
S_FIELDS = ("n_ends", "n_points", "n_kept", "n_front", "n_reproj_ok", "n_parallax_ok", "n_few", "n_singular")
T_FIELDS = ("max_views", "min_views", "gn_iters", "reserved_", "max_reproj_px", "max_parallax_cos")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define O(f) (int)offsetof(vis_ftrack_obs, f)
#define F(f) (int)offsetof(vis_ftrack_frame, f)
#define P(f) (int)offsetof(vis_ftrack_point, f)
#define S(f) (int)offsetof(vis_ftrack_tri_summary, f)
#define T(f) (int)offsetof(vis_ftrack_tri_params, f)
int main(void) {
    printf("%d %d %d %d %d\n", (int)sizeof(vis_ftrack_obs), O(birth_seq), O(birth_kp), O(len), O(prev_kp));
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_ftrack_frame), F(seq), F(n_keypoints), F(n_continued), F(n_started), F(n_ended), F(max_len),
           F(sum_len), F(flags));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_ftrack_point), P(X), P(rms_reproj_px), P(parallax_cos), P(n_views), P(flags));
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_ftrack_tri_summary), S(n_ends), S(n_points), S(n_kept), S(n_front), S(n_reproj_ok),
           S(n_parallax_ok), S(n_few), S(n_singular));
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_ftrack_tri_params), T(max_views), T(min_views), T(gn_iters), T(reserved_), T(max_reproj_px),
           T(max_parallax_cos));
    printf("%d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_FT_NO_PAIR, (int)VIS_FT_NO_CARRY, (int)VIS_FT_SYM, (int)VIS_FT_GOOD);
    printf("%d %d %d %d %d %d\n", (int)VIS_FTP_FRONT, (int)VIS_FTP_REPROJ_OK, (int)VIS_FTP_PARALLAX_OK, (int)VIS_FTP_KEPT, (int)VIS_FTP_FEW,
           (int)VIS_FTP_SINGULAR);
    printf("%d %d %d\n", (int)VIS_KF_CARRIED, (int)VIS_KF_NOT_SAVED, (int)VIS_KF_FIRST);
    return 0;
}
"""


def test_layout_in_c_ctypes_numpy_and_the_restatement(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [16, 0, 4, 8, 12]
    assert rows[1] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert rows[2] == [40, 0, 24, 28, 32, 36]
    assert rows[3] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert rows[4] == [32, 0, 4, 8, 12, 16, 24]
    for fields, row, dts in ((O_FIELDS, rows[0], (vislam.FTRACK_OBS_DTYPE, fr.OBS_DTYPE)), (F_FIELDS, rows[1], (vislam.FTRACK_FRAME_DTYPE, fr.FRAME_DTYPE)),
                             (P_FIELDS, rows[2], (vislam.FTRACK_POINT_DTYPE, fr.POINT_DTYPE)),
                             (S_FIELDS, rows[3], (vislam.FTRACK_TRI_SUMMARY_DTYPE, fr.TRI_SUMMARY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    S = vislam.FtrackTriParams
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in T_FIELDS] == rows[4]
    assert rows[5][0] == 5                                         # VIS_ABI_VERSION: only new symbols and new structs
    assert rows[5][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[5][2:] == [vislam.FT_NO_PAIR, vislam.FT_NO_CARRY, vislam.FT_SYM, vislam.FT_GOOD] == [fr.FT_NO_PAIR, fr.FT_NO_CARRY, fr.FT_SYM, fr.FT_GOOD] == [1, 2, 0, 1]
    assert rows[6] == [vislam.FTP_FRONT, vislam.FTP_REPROJ_OK, vislam.FTP_PARALLAX_OK, vislam.FTP_KEPT, vislam.FTP_FEW, vislam.FTP_SINGULAR] == \
        [fr.FTP_FRONT, fr.FTP_REPROJ_OK, fr.FTP_PARALLAX_OK, fr.FTP_KEPT, fr.FTP_FEW, fr.FTP_SINGULAR] == [1, 2, 4, 8, 16, 32]
    assert rows[7] == [fr.KF_CARRIED, fr.KF_NOT_SAVED, fr.KF_FIRST] == [vislam.KF_CARRIED, vislam.KF_NOT_SAVED, vislam.KF_FIRST]
    assert vislam.DMATCH_DTYPE == fr.DMATCH_DTYPE


def test_defaults(vislam):
    tp, want = vislam.default_ftrack_tri_params(), fr.TriParams()
    assert [getattr(tp, f) for f in T_FIELDS] == [16, 2, 5, 0, 2.0, 0.9998476951563913]
    assert [getattr(tp, f) for f in T_FIELDS if f != "reserved_"] == [getattr(want, f) for f in T_FIELDS if f != "reserved_"]
    assert abs(tp.max_parallax_cos - np.cos(np.deg2rad(1.0))) < 1e-15
    vislam.lib.vis_default_ftrack_tri_params(None)                 # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("ftrack_link_rows", "batch_ftrack", "ftrack_triangulate_rows", "batch_ftrack_triangulate"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a16, a8, a4, odd16, odd8, odd4 = (C.c_void_p(v) for v in (64, 72, 68, 72, 68, 66))   # never dereferenced: the argument / context checks come first
    # ---- vis_ftrack_link_rows
    link = lambda n=1, prev=a4, nkp=a4, links=a16, nl=a4, lcap=8, mask=None, mcap=0, carry=None, seq0=0, cap=8, obs=a16, fr_=a4: \
        L.vis_ftrack_link_rows(None, n, prev, nkp, links, nl, lcap, mask, mcap, carry, seq0, cap, obs, fr_)
    assert link() == -5 and link(mask=a4, mcap=8) == -5 and link(carry=a16) == -5 and link(n=0) == -5 and link(links=None, lcap=0) == -5
    assert link(n=1 << 20, cap=1 << 20) == -5                      # the capacity refusal comes after the context's
    for k in ("prev", "nkp", "links", "nl", "obs", "fr_"):
        assert link(**{k: None}) == -1, k
    assert link(links=odd16) == -1 and link(carry=odd16) == -1 and link(obs=odd16) == -1
    assert link(prev=odd4) == -1 and link(nkp=odd4) == -1 and link(nl=odd4) == -1 and link(fr_=odd4) == -1
    assert link(n=-1) == -1 and link(lcap=-1) == -1 and link(mcap=-1) == -1 and link(cap=-1) == -1 and link(seq0=-1) == -1
    # ---- vis_batch_ftrack
    plan = lambda src=0, inl=0, n=1, mask=None, mcap=0, cap=8, obs=a16, fr_=a4: L.vis_batch_ftrack(None, src, inl, n, mask, mcap, cap, obs, fr_)
    assert plan() == -5 and plan(src=1) == -5 and plan(inl=1) == -5 and plan(mask=a4, mcap=8) == -5
    assert plan(obs=None) == -1 and plan(fr_=None) == -1 and plan(obs=odd16) == -1 and plan(fr_=odd4) == -1
    assert plan(n=-1) == -1 and plan(mcap=-1) == -1 and plan(cap=-1) == -1 and plan(src=2) == -1 and plan(src=-1) == -1
    assert plan(inl=1, mask=a4, mcap=8) == -1                      # the pose stage's mask excludes a caller's
    # ---- the triangulation
    tp = vislam.default_ftrack_tri_params()
    ok = C.byref(tp)
    rows = lambda tp_=ok, n=1, prev=a4, nkp=a4, obs=a16, cap=8, xy=a8, poses=a8, pts=a8, fl=a4, sm=a4: \
        L.vis_ftrack_triangulate_rows(None, tp_, n, prev, nkp, obs, cap, xy, poses, pts, fl, sm)
    btri = lambda tp_=ok, n=1, obs=a16, cap=8, poses=a8, pts=a8, fl=a4, sm=a4: L.vis_batch_ftrack_triangulate(None, tp_, n, obs, cap, poses, pts, fl, sm)
    assert rows() == -5 and btri() == -5 and rows(n=1 << 20, cap=1 << 20) == -5
    for k in ("tp_", "prev", "nkp", "obs", "xy", "poses", "pts", "fl", "sm"):
        assert rows(**{k: None}) == -1, k
    for k in ("tp_", "obs", "poses", "pts", "fl", "sm"):
        assert btri(**{k: None}) == -1, k
    assert rows(obs=odd16) == -1 and rows(xy=odd8) == -1 and rows(poses=odd8) == -1 and rows(pts=odd8) == -1
    assert rows(prev=odd4) == -1 and rows(nkp=odd4) == -1 and rows(sm=odd4) == -1 and rows(n=-1) == -1 and rows(cap=-1) == -1
    assert btri(obs=odd16) == -1 and btri(poses=odd8) == -1 and btri(pts=odd8) == -1 and btri(sm=odd4) == -1 and btri(n=-1) == -1 and btri(cap=-1) == -1
    nan, inf = float("nan"), float("inf")
    bad = [("max_views", 1), ("max_views", 33), ("min_views", 1), ("min_views", 17), ("gn_iters", -1), ("gn_iters", 11)]
    bad += [("max_reproj_px", v) for v in (0.0, -1.0, nan, inf, 1e7)] + [("max_parallax_cos", v) for v in (-1.0, 1.0000001, nan, inf)]
    for f, v in bad:
        q = vislam.default_ftrack_tri_params()
        setattr(q, f, v)
        assert rows(tp_=C.byref(q)) == -1 and btri(tp_=C.byref(q)) == -1, (f, v)
    for f, v in (("max_views", 2), ("max_views", 32), ("min_views", 16), ("gn_iters", 0), ("gn_iters", 10), ("max_reproj_px", 1e6), ("max_parallax_cos", 1.0)):
        q = vislam.default_ftrack_tri_params()
        setattr(q, f, v)
        assert rows(tp_=C.byref(q)) == -5 and btri(tp_=C.byref(q)) == -5, (f, v)
