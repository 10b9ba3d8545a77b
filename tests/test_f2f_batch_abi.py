"""CPU: the batched F2FRansac / FilterKeypoints entry points' place in the C ABI -- vis_f2f_result (32 bytes) in the C compiler's layout and in
the ctypes / numpy bindings; VIS_F2F_TILE; the five symbols exported and listed; every refusal that needs no device; VIS_ABI_VERSION and
vis_params unchanged (only new symbols and one new struct)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_f2f_batch", "vis_batch_f2f", "vis_filter_keypoints_batch", "vis_batch_filter_keypoints", "vis_filter_keypoints")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_f2f_result), (int)offsetof(vis_f2f_result, t), (int)offsetof(vis_f2f_result, count_max),
           (int)offsetof(vis_f2f_result, n_points), (int)offsetof(vis_f2f_result, best_iter), (int)offsetof(vis_f2f_result, n_degenerate),
           (int)offsetof(vis_f2f_result, flipped));
    printf("%d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_F2F_TILE);
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
    assert rows[0] == [32, 0, 12, 16, 20, 24, 28]
    F = vislam.F2fResult
    assert [C.sizeof(F), F.t.offset, F.count_max.offset, F.n_points.offset, F.best_iter.offset, F.n_degenerate.offset, F.flipped.offset] == rows[0]
    d = vislam.F2F_RESULT_DTYPE
    assert [d.itemsize] + [d.fields[k][1] for k in ("t", "count_max", "n_points", "best_iter", "n_degenerate", "flipped")] == rows[0]
    assert rows[1][0] == 5                                         # VIS_ABI_VERSION: only new symbols and a new struct
    assert rows[1][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[1][2] == vislam.F2F_TILE                           # the binding's constant is the kernel's tile


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("f2f_batch", "batch_f2f", "filter_keypoints", "filter_keypoints_batch", "batch_filter_keypoints"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some = C.c_void_p(64)                                          # never dereferenced: the argument / context checks come first
    nan, inf = float("nan"), float("inf")
    # NULL context -> VIS_E_STATE
    assert L.vis_f2f_batch(None, 1, some, some, some, 49, some, None, some, some) == -5
    assert L.vis_batch_f2f(None, 1, some, None, some, some) == -5
    assert L.vis_filter_keypoints_batch(None, 1, some, some, some, 49, some, some, 500.0, 49, some, some) == -5
    assert L.vis_batch_filter_keypoints(None, 1, some, some, 500.0, 49, some, some) == -5
    nk = C.c_int(7)
    assert L.vis_filter_keypoints(None, some, some, 1, some, some, 500.0, some, C.byref(nk)) == -5
    # NULL outputs (and the NULL inputs the header names) -> VIS_E_INVALID
    assert L.vis_f2f_batch(None, 1, some, some, some, 49, some, None, some, None) == -1
    assert L.vis_f2f_batch(None, 1, some, some, some, 49, None, None, some, some) == -1
    assert L.vis_f2f_batch(None, 1, some, some, some, 49, some, None, None, some) == -1
    assert L.vis_f2f_batch(None, 1, some, some, None, 49, some, None, some, some) == -1
    assert L.vis_f2f_batch(None, 1, None, some, some, 49, some, None, some, some) == -1
    assert L.vis_f2f_batch(None, 1, C.c_void_p(68), some, some, 49, some, None, some, some) == -1      # rows of (x, y): 8-byte aligned
    assert L.vis_f2f_batch(None, -1, some, some, some, 49, some, None, some, some) == -1
    assert L.vis_batch_f2f(None, 1, None, None, some, some) == -1
    assert L.vis_batch_f2f(None, 1, some, None, None, some) == -1
    assert L.vis_batch_f2f(None, 1, some, None, some, None) == -1
    assert L.vis_filter_keypoints_batch(None, 1, some, some, some, 49, some, some, 500.0, 49, None, some) == -1
    assert L.vis_filter_keypoints_batch(None, 1, some, some, some, 49, some, some, 500.0, 49, some, None) == -1
    assert L.vis_filter_keypoints_batch(None, 1, some, some, some, 49, some, None, 500.0, 49, some, some) == -1
    assert L.vis_batch_filter_keypoints(None, 1, some, some, 500.0, 49, None, some) == -1
    assert L.vis_batch_filter_keypoints(None, 1, some, some, 500.0, 49, some, None) == -1
    assert L.vis_batch_filter_keypoints(None, 1, None, some, 500.0, 49, some, some) == -1
    assert L.vis_filter_keypoints(None, some, some, 1, some, some, 500.0, None, C.byref(nk)) == -1
    assert L.vis_filter_keypoints(None, some, some, 1, some, some, 500.0, some, None) == -1
    # a threshold that is not finite -> VIS_E_INVALID
    for bad in (nan, inf, -inf):
        assert L.vis_filter_keypoints_batch(None, 1, some, some, some, 49, some, some, bad, 49, some, some) == -1
        assert L.vis_batch_filter_keypoints(None, 1, some, some, bad, 49, some, some) == -1
        assert L.vis_filter_keypoints(None, some, some, 1, some, some, bad, some, C.byref(nk)) == -1
    assert nk.value == 7                                           # a refused call writes nothing
