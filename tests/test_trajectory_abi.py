"""CPU: the scale-link and trajectory entry points' place in the C ABI -- vis_scale_link_params (32 bytes), vis_scale_link (40) and vis_traj_pose
(128) in the C compiler's layout, in the ctypes / numpy bindings and in the restatements, the enums and defaults, the seven symbols exported and
listed, and every refusal that needs no device, in the header's order; VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import os
import subprocess

import scale_link_ref as sl
import trajectory_ref as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_scale_link_params", "vis_scale_link_rows", "vis_batch_scale_links", "vis_trajectory_rows", "vis_batch_trajectory",
           "vis_batch_trajectory_init")
P_FIELDS = ("require", "min_shared", "max_rel_spread", "min_scale", "max_scale")
L_FIELDS = ("scale", "q25", "q75", "n_shared", "q", "flags", "reserved_")
T_FIELDS = ("R", "t", "sigma", "segment_seq", "epoch_seq", "hops", "unit_edges", "parent", "flags")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_scale_link_params, f)
#define L(f) (int)offsetof(vis_scale_link, f)
#define T(f) (int)offsetof(vis_traj_pose, f)
int main(void) {
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_scale_link_params), P(require), P(min_shared), P(max_rel_spread), P(min_scale), P(max_scale));
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(vis_scale_link), L(scale), L(q25), L(q75), L(n_shared), L(q), L(flags), L(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_traj_pose), T(R), T(t), T(sigma), T(segment_seq), T(epoch_seq), T(hops), T(unit_edges),
           T(parent), T(flags));
    printf("%d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_TJ_MAX_FRAMES);
    printf("%d %d %d %d %d %d\n", (int)VIS_SL_OK, (int)VIS_SL_NO_PAIR, (int)VIS_SL_NO_DEPTH, (int)VIS_SL_FEW, (int)VIS_SL_SPREAD, (int)VIS_SL_RANGE);
    printf("%d %d %d %d %d %d\n", (int)VIS_TJ_ROOT, (int)VIS_TJ_NO_POSE, (int)VIS_TJ_NO_CARRY, (int)VIS_TJ_NOT_SAVED, (int)VIS_TJ_UNIT_EDGE,
           (int)VIS_TJ_OVERFLOW);
    printf("%d %d %d\n", (int)sizeof(vis_pose_result), (int)offsetof(vis_pose_result, R), (int)offsetof(vis_pose_result, t));
    return 0;
}
"""


def test_layout_in_c_ctypes_numpy_and_the_restatements(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [32, 0, 4, 8, 16, 24]
    assert rows[1] == [40, 0, 8, 16, 24, 28, 32, 36]
    assert rows[2] == [128, 0, 72, 96, 104, 108, 112, 116, 120, 124]
    S = vislam.ScaleLinkParams
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in P_FIELDS] == rows[0]
    T = vislam.TrajPose
    assert [C.sizeof(T)] + [getattr(T, f).offset for f in T_FIELDS] == rows[2]
    for fields, row, dts in ((L_FIELDS, rows[1], (vislam.SCALE_LINK_DTYPE, sl.LINK_DTYPE)), (T_FIELDS, rows[2], (vislam.TRAJ_POSE_DTYPE, tj.TRAJ_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert rows[3] == [5, 144, vislam.TJ_MAX_FRAMES] and C.sizeof(vislam.Params) == 144 and tj.TJ_MAX_FRAMES == 1024
    assert rows[4] == [vislam.SL_OK, vislam.SL_NO_PAIR, vislam.SL_NO_DEPTH, vislam.SL_FEW, vislam.SL_SPREAD, vislam.SL_RANGE] == \
        [sl.SL_OK, sl.SL_NO_PAIR, sl.SL_NO_DEPTH, sl.SL_FEW, sl.SL_SPREAD, sl.SL_RANGE] == [0, 1, 2, 4, 8, 16]
    assert rows[5] == [vislam.TJ_ROOT, vislam.TJ_NO_POSE, vislam.TJ_NO_CARRY, vislam.TJ_NOT_SAVED, vislam.TJ_UNIT_EDGE, vislam.TJ_OVERFLOW] == \
        [tj.TJ_ROOT, tj.TJ_NO_POSE, tj.TJ_NO_CARRY, tj.TJ_NOT_SAVED, tj.TJ_UNIT_EDGE, tj.TJ_OVERFLOW] == [1, 2, 4, 8, 16, 32]
    assert rows[6] == [sl.POSE_DTYPE.itemsize, sl.POSE_DTYPE.fields["R"][1], sl.POSE_DTYPE.fields["t"][1]] and sl.POSE_DTYPE == vislam.POSE_RESULT_DTYPE
    assert sl.MAP_POINT_DTYPE == vislam.MAP_POINT_DTYPE and sl.DMATCH_DTYPE == vislam.DMATCH_DTYPE and sl.MP_KEPT == vislam.MP_KEPT


def test_defaults(vislam):
    sp, want = vislam.default_scale_link_params(), sl.Params()
    assert [getattr(sp, f) for f in P_FIELDS] == [16, 8, 1.0, 1.0 / 64.0, 64.0] == [getattr(want, f) for f in P_FIELDS]
    vislam.lib.vis_default_scale_link_params(None)                 # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("scale_link_rows", "batch_scale_links", "trajectory_rows", "batch_trajectory", "batch_trajectory_init"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a16, a8, a4, odd16, odd8, odd4 = (C.c_void_p(v) for v in (64, 72, 68, 72, 68, 66))   # never dereferenced: the argument / context checks come first
    ok = C.byref(vislam.default_scale_link_params())
    # ---- vis_scale_link_rows
    rows = lambda sp=ok, n=1, prev=a4, links=a16, nl=a4, lcap=8, pose=a8, pts=a16, fl=a4, pcap=8, carry=None, cap=8, depth=a8, link=a8: \
        L.vis_scale_link_rows(None, sp, n, prev, links, nl, lcap, pose, pts, fl, pcap, carry, cap, depth, link)
    assert rows() == -5 and rows(carry=a8) == -5 and rows(n=0) == -5 and rows(links=None, pts=None, fl=None, lcap=0) == -5
    assert rows(links=None, pts=None, fl=None, pcap=0) == -5 and rows(n=1 << 20, cap=1 << 20) == -5 and rows(n=1 << 20, lcap=1 << 20) == -5
    for k in ("sp", "prev", "nl", "pose", "depth", "link", "links", "pts", "fl"):
        assert rows(**{k: None}) == -1, k
    assert rows(links=odd16) == -1 and rows(pts=odd16) == -1 and rows(pose=odd8) == -1 and rows(depth=odd8) == -1 and rows(carry=odd8) == -1
    assert rows(link=odd8) == -1 and rows(prev=odd4) == -1 and rows(nl=odd4) == -1
    assert rows(n=-1) == -1 and rows(lcap=-1) == -1 and rows(pcap=-1) == -1 and rows(cap=-1) == -1
    # ---- vis_batch_scale_links
    plan = lambda sp=ok, n=1, pts=a16, fl=a4, cap=8, link=a8: L.vis_batch_scale_links(None, sp, n, pts, fl, cap, link)
    assert plan() == -5
    for k in ("sp", "pts", "fl", "link"):
        assert plan(**{k: None}) == -1, k
    assert plan(pts=odd16) == -1 and plan(link=odd8) == -1 and plan(n=-1) == -1 and plan(cap=-1) == -1
    # ---- the parameters
    nan, inf = float("nan"), float("inf")
    bad = [("require", -1), ("require", 256), ("min_shared", 0), ("min_shared", (1 << 20) + 1), ("min_scale", 0.0), ("min_scale", -1.0), ("min_scale", 65.0)]
    bad += [("max_rel_spread", v) for v in (-0.5, nan, inf, 1e7)] + [("min_scale", v) for v in (nan, inf)] + [("max_scale", v) for v in (nan, inf, 0.001)]
    for f, v in bad:
        q = vislam.default_scale_link_params()
        setattr(q, f, v)
        assert rows(sp=C.byref(q)) == -1 and plan(sp=C.byref(q)) == -1, (f, v)
    for f, v in (("require", 0), ("require", 255), ("min_shared", 1), ("min_shared", 1 << 20), ("max_rel_spread", 0.0), ("max_rel_spread", 1e6), ("min_scale", 64.0)):
        q = vislam.default_scale_link_params()
        setattr(q, f, v)
        assert rows(sp=C.byref(q)) == -5 and plan(sp=C.byref(q)) == -5, (f, v)
    # ---- vis_trajectory_rows / vis_batch_trajectory / vis_batch_trajectory_init
    chain = lambda n=1, prev=a4, pose=a8, link=a8, carry=None, seq0=0, same=1, traj=a8, poses=None: \
        L.vis_trajectory_rows(None, n, prev, pose, link, carry, seq0, same, traj, poses)
    assert chain() == -5 and chain(carry=a8, poses=a8) == -5 and chain(n=0) == -5 and chain(same=0) == -5
    assert chain(n=vislam.TJ_MAX_FRAMES + 1) == -5                 # the capacity refusal comes after the context's
    for k in ("prev", "pose", "link", "traj"):
        assert chain(**{k: None}) == -1, k
    assert chain(pose=odd8) == -1 and chain(link=odd8) == -1 and chain(carry=odd8) == -1 and chain(traj=odd8) == -1 and chain(poses=odd8) == -1
    assert chain(prev=odd4) == -1 and chain(n=-1) == -1 and chain(seq0=-1) == -1
    bt = lambda n=1, link=a8, same=1, traj=a8, poses=None: L.vis_batch_trajectory(None, n, link, same, traj, poses)
    assert bt() == -5 and bt(poses=a8) == -5
    assert bt(link=None) == -1 and bt(traj=None) == -1 and bt(link=odd8) == -1 and bt(traj=odd8) == -1 and bt(poses=odd8) == -1 and bt(n=-1) == -1
    assert L.vis_batch_trajectory_init(None, None) == -5 and L.vis_batch_trajectory_init(None, C.byref(vislam.TrajPose())) == -5
