"""CPU: the map-point entry points' place in the C ABI -- vis_tri_params (16 bytes), vis_map_point (32), vis_tri_summary (16), the same in
the C compiler's layout and in the ctypes / numpy bindings; the VIS_MP_* flag values; the three symbols exported and listed; this
library's default thresholds; the argument and state errors that need no device; VIS_ABI_VERSION unchanged (only new symbols and structs)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    printf("%d %d %d %d %d\n", (int)sizeof(vis_tri_params), (int)offsetof(vis_tri_params, max_reproj_px), (int)offsetof(vis_tri_params, min_parallax_px),
           (int)offsetof(vis_tri_params, inliers_only), (int)offsetof(vis_tri_params, reserved_));
    printf("%d %d %d %d\n", (int)sizeof(vis_map_point), (int)offsetof(vis_map_point, X), (int)offsetof(vis_map_point, reproj_px),
           (int)offsetof(vis_map_point, parallax_px));
    printf("%d %d %d %d %d\n", (int)sizeof(vis_tri_summary), (int)offsetof(vis_tri_summary, n_points), (int)offsetof(vis_tri_summary, n_front),
           (int)offsetof(vis_tri_summary, n_kept), (int)offsetof(vis_tri_summary, mean_parallax_px));
    printf("%d %d %d %d %d %d %d\n", VIS_MP_INLIER, VIS_MP_FRONT, VIS_MP_REPROJ_OK, VIS_MP_PARALLAX_OK, VIS_MP_KEPT, VIS_ABI_VERSION, (int)sizeof(vis_params));
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
    assert rows[0] == [16, 0, 4, 8, 12]
    assert rows[1] == [32, 0, 24, 28]
    assert rows[2] == [16, 0, 4, 8, 12]
    T, M, S = vislam.TriParams, vislam.MapPoint, vislam.TriSummary
    assert [C.sizeof(T), T.max_reproj_px.offset, T.min_parallax_px.offset, T.inliers_only.offset, T.reserved_.offset] == rows[0]
    assert [C.sizeof(M), M.X.offset, M.reproj_px.offset, M.parallax_px.offset] == rows[1]
    assert [C.sizeof(S), S.n_points.offset, S.n_front.offset, S.n_kept.offset, S.mean_parallax_px.offset] == rows[2]
    d = vislam.MAP_POINT_DTYPE
    assert [d.itemsize, d.fields["X"][1], d.fields["reproj_px"][1], d.fields["parallax_px"][1]] == rows[1]
    d = vislam.TRI_SUMMARY_DTYPE
    assert [d.itemsize] + [d.fields[k][1] for k in ("n_points", "n_front", "n_kept", "mean_parallax_px")] == rows[2]
    assert rows[3][:5] == [1, 2, 4, 8, 16]
    assert (vislam.MP_INLIER, vislam.MP_FRONT, vislam.MP_REPROJ_OK, vislam.MP_PARALLAX_OK, vislam.MP_KEPT) == (1, 2, 4, 8, 16)
    assert rows[3][5] == 5                                         # VIS_ABI_VERSION: only new symbols and structs
    assert rows[3][6] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow


def test_symbols_exported_and_listed(vislam):
    for s in ("vis_default_tri_params", "vis_triangulate", "vis_batch_triangulate"):
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s


def test_default_tri_params(vislam):
    tp = vislam.default_tri_params()
    assert (tp.max_reproj_px, tp.min_parallax_px, tp.inliers_only, tp.reserved_) == (2.0, 0.0, 0, 0)
    vislam.lib.vis_default_tri_params(None)                        # tolerated


def test_errors_that_need_no_device(vislam):
    tp = vislam.default_tri_params()
    some = C.c_void_p(64)                                          # never dereferenced: the context / argument checks come first
    sm = vislam.TriSummary()
    # vis_batch_triangulate: VIS_E_STATE without a context, VIS_E_INVALID for NULL (or misaligned) outputs
    assert vislam.lib.vis_batch_triangulate(None, C.byref(tp), 1, 49, some, some, some) == -5
    assert vislam.lib.vis_batch_triangulate(None, C.byref(tp), 1, 49, None, some, some) == -1
    assert vislam.lib.vis_batch_triangulate(None, C.byref(tp), 1, 49, some, None, some) == -1
    assert vislam.lib.vis_batch_triangulate(None, C.byref(tp), 1, 49, some, some, None) == -1
    assert vislam.lib.vis_batch_triangulate(None, None, 1, 49, some, some, some) == -1
    assert vislam.lib.vis_batch_triangulate(None, C.byref(tp), 1, 49, C.c_void_p(72), some, some) == -1      # d_points: 16-byte aligned
    # vis_triangulate: VIS_E_INVALID without a context, like the other frame-at-a-time entry points
    assert vislam.lib.vis_triangulate(None, C.byref(tp), some, some, some, some, 1, None, some, some, C.byref(sm)) == -1
